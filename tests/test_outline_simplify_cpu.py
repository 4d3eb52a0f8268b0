"""Host half of the outline simplifier: the sequential restatement (tests/simplify_ref.py), which the GPU tests hold
the kernels to, against the contract's hand-derived answers and its properties on random maps; cat_seg.vectorize on
simplified rings; the config keys and their refusal; the C ABI entries and their host-side argument checks; and the
kernels' logic (csrc/outline_simplify_logic.h) run sequentially on the host against a brute-force recursive
Douglas-Peucker (tools/outline_simplify_host.cpp, built with the address and undefined-behaviour sanitizers)."""
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import outlines_ref as O
import regions_ref as R
import simplify_ref as S
from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg.vectorize import outlines_to_geojson, rings_by_region

from conftest import ROOT
from test_boundary_cpu import tiny_cfg
from test_region_outlines_cpu import CASES, HOLE, random_map

STAIRS = np.array([[1, 1, 1, 1],
                   [2, 1, 1, 1],
                   [2, 2, 1, 1],
                   [2, 2, 2, 1]])
TOLERANCES = (0, 0.5, 1, 1.5, 3, 1000)


def simplified(m, t, conn=8):
    m = np.asarray(m)
    src = O.trace(m, conn)
    return src, S.simplify(m, src, t)


def rings(s):
    return [O.ring(s, j) for j in range(len(s["ring_value"]))]


# ------------------------------------------------------------------ the hand-derived answers of the contract
@pytest.mark.parametrize("t", TOLERANCES)
def test_single_pixel_keeps_its_four_map_corners(t):
    src, s = simplified([[7]], t)
    assert rings(s) == [[(0, 0), (1, 0), (1, 1), (0, 1)]]
    assert s["ring_value"].tolist() == [7] and s["ring_area2"].tolist() == [2] and s["ring_hole"].tolist() == [0]
    assert s["ring_offset"].dtype == np.int32 and s["ring_value"].dtype == np.int32
    assert s["ring_area2"].dtype == np.int64 and s["ring_hole"].dtype == np.uint8
    assert s["vertices"].dtype == np.int32 and s["vertices"].shape == (4, 2)


@pytest.mark.parametrize("t", TOLERANCES)
def test_t_junction_is_inserted_into_the_straight_edge(t):
    src, s = simplified([[1, 1], [2, 3]], t)
    assert src["ring_value"].tolist()[0] == 1 and O.ring(src, 0) == [(0, 0), (2, 0), (2, 1), (0, 1)]
    assert O.ring(s, 0) == [(0, 0), (2, 0), (2, 1), (1, 1), (0, 1)]
    assert s["ring_area2"][0] == 4


def test_hole_map():
    src = O.trace(HOLE, 8)             # rings: frame of 0s, its hole, the 5s, their hole, the inner 0
    assert src["ring_value"].tolist() == [0, 0, 5, 5, 0]
    s = S.simplify(HOLE, src, 1)
    assert O.ring(s, 4) == [(2, 2), (3, 3)] and O.ring(s, 3) == [(2, 2), (3, 3)]
    assert O.ring(s, 2) == [(1, 1), (4, 1), (4, 4), (1, 4)]
    assert s["ring_hole"].tolist() == [0, 1, 0, 1, 0]
    s = S.simplify(HOLE, src, 1.5)
    assert O.ring(s, 4) == [(2, 2)] and O.ring(s, 3) == [(2, 2)]
    assert s["ring_area2"].tolist()[3:] == [0, 0]
    s = S.simplify(HOLE, src, 2.5)
    assert O.ring(s, 2) == [(1, 1), (4, 4)] and O.ring(s, 1) == [(1, 1), (4, 4)]
    assert O.ring(s, 0) == [(0, 0), (5, 0), (5, 5), (0, 5)]              # the map's corners are anchors


def test_staircase():
    src = O.trace(STAIRS, 8)
    assert src["ring_value"].tolist() == [1, 2]
    s = S.simplify(STAIRS, src, 0.5)
    assert O.ring(s, 0) == [(0, 0), (4, 0), (4, 4), (3, 4), (2, 2), (1, 2), (1, 1), (0, 1)]
    assert O.ring(s, 1) == [(0, 1), (1, 1), (1, 2), (2, 2), (3, 4), (0, 4)]
    s = S.simplify(STAIRS, src, 1)
    assert O.ring(s, 0) == [(0, 0), (4, 0), (4, 4), (3, 4), (0, 1)]
    assert O.ring(s, 1) == [(0, 1), (3, 4), (0, 4)] and s["ring_area2"][1] == 9


def test_junctions_do_not_depend_on_connectivity():
    j = S.junctions(np.array([[0, 1], [1, 0]]))
    assert j[1, 1] and j.all()                     # the pinch has degree 4; every other vertex lies on the frame
    j = S.junctions(np.zeros((2, 3), int))
    assert j.sum() == 4 and j[0, 0] and j[0, 3] and j[2, 0] and j[2, 3]


def test_tolerance_rounding():
    assert [S.tol2_q4(t) for t in (0, 0.25, 0.5, 1, 1.5, 16384)] == [0, 1, 4, 16, 36, 16 * 16384 ** 2]
    assert S.tol2_q4(0.17) == 0 and S.tol2_q4(0.18) == 1


# ------------------------------------------------------------------ the properties on random maps
_DETAIL = {}


def detail(H, W, nlab, seed, conn, t):
    k = (H, W, nlab, seed, conn, t)
    if k not in _DETAIL:
        ids, _ = R.regions(random_map(np.random.default_rng(seed), H, W, nlab), conn)
        src = O.trace(ids, conn)
        _DETAIL[k] = (ids, src, S.detail(ids, src, t))
    return _DETAIL[k]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W,nlab,seed", CASES)
def test_properties_on_region_ids(H, W, nlab, seed, conn):
    for t in TOLERANCES:
        ids, src, det = detail(H, W, nlab, seed, conn, t)
        s = S.simplify(ids, src, t, det)
        twins = {}                                  # source node sequence of an arc -> its kept sequence
        for ring in det:
            nodes, n = ring["nodes"], len(ring["nodes"])
            assert all(i in ring["kept"] for i, p in enumerate(nodes) if p[2])              # anchors are kept
            if t == 0:
                assert ring["kept"] == list(range(n))                                        # t = 0 keeps every node
            for arc in ring["arcs"]:
                idx = [(arc["start"] + k) % n for k in range(arc["len"] + 1)]
                pos = arc["pos"]
                assert pos[0] == 0 and pos[-1] == arc["len"]
                P = np.asarray([nodes[i][:2] for i in idx], np.float64)
                if t == 1000:
                    assert pos == [0, arc["len"]]                                            # its two anchors
                for a, b in zip(pos, pos[1:]):      # every dropped node lies within t of its final segment's line
                    d, rel = P[b] - P[a], P[a + 1:b] - P[a]
                    L = math.hypot(*d)
                    dist = np.hypot(rel[:, 0], rel[:, 1]) if L == 0 else np.abs(d[0] * rel[:, 1] - d[1] * rel[:, 0]) / L
                    assert (dist <= t + 1e-9).all()
                if not arc["frame"]:
                    seq = tuple(nodes[i][:2] for i in idx)
                    assert seq not in twins
                    twins[seq] = tuple(seq[p] for p in pos)
        # every arc off the frame occurs once more, reversed, and keeps the same vertices there
        for seq, kept in twins.items():
            assert twins[seq[::-1]] == kept[::-1]
        if t == 0:                                  # as edges: each one exactly once more, reversed, in another ring
            edges = {}
            for j, pts in enumerate(rings(s)):
                for i, a in enumerate(pts):
                    edges.setdefault((a, pts[(i + 1) % len(pts)]), []).append(j)
            for (a, b), where in edges.items():
                assert len(where) == 1
                if not S.on_frame(a, b, H, W):
                    assert len(edges[(b, a)]) == 1 and edges[(b, a)] != where
                else:
                    assert (b, a) not in edges
        assert S.count_nodes(det) >= len(src["vertices"])
        assert np.array_equal(s["ring_hole"], src["ring_area2"] < 0) and np.array_equal(s["ring_value"], src["ring_value"])


# ------------------------------------------------------------------ cat_seg.vectorize on simplified rings
def test_geojson_uses_ring_hole_and_leaves_collapsed_rings_out():
    ids, table = R.regions(HOLE, 8, score=np.full(HOLE.shape, 0.5, np.float32))
    src = O.trace(ids, 8)
    # t = 1: the inner 0 (region 2) and the hole of the 5s collapse to two vertices
    s = S.simplify(ids, src, 1)
    g = rings_by_region(s)
    assert list(g) == [0, 1] and [len(v) for v in g.values()] == [2, 1]
    assert [x["hole"] for x in g[0]] == [False, True]
    fc = outlines_to_geojson(s, table)
    json.loads(json.dumps(fc))
    assert [f["properties"]["region"] for f in fc["features"]] == [0, 1]
    assert fc["features"][1]["geometry"]["coordinates"] == [[[1, 1], [4, 1], [4, 4], [1, 4], [1, 1]]]
    assert len(fc["features"][0]["geometry"]["coordinates"]) == 2
    # t = 2.5: the 5s collapse, and with them the hole they left in region 0; region 0 stays
    s = S.simplify(ids, src, 2.5)
    fc = outlines_to_geojson(s, table)
    assert [f["properties"]["region"] for f in fc["features"]] == [0]
    assert fc["features"][0]["geometry"]["coordinates"] == [[[0, 0], [5, 0], [5, 5], [0, 5], [0, 0]]]
    # ring_hole decides, not the sign: flip the sign of an exterior ring's area and it stays the exterior
    flipped = {**S.simplify(ids, src, 0)}
    flipped["ring_area2"] = -flipped["ring_area2"]
    assert [[x["hole"] for x in v] for v in rings_by_region(flipped).values()] == [[False, True], [False, True], [False]]
    assert len(outlines_to_geojson(flipped, table)["features"]) == 3
    # a zero-area ring of three vertices is left out too
    z = {"ring_offset": np.array([0, 3], np.int32), "ring_value": np.array([0], np.int32),
         "ring_area2": np.array([0], np.int64), "ring_hole": np.array([0], np.uint8),
         "vertices": np.array([[0, 0], [2, 2], [4, 4]], np.int32)}
    assert rings_by_region(z) == {}
    with pytest.raises(ValueError, match="region"):
        outlines_to_geojson(S.simplify(HOLE, O.trace(HOLE, 8), 0), table)


def test_unsimplified_dict_gives_the_same_json_as_before():
    """Without "ring_hole" the present code runs: the features equal those built here from the rings directly."""
    ids, table = R.regions(random_map(np.random.default_rng(5), 13, 13, 3), 8, score=np.full((13, 13), 0.25, np.float32))
    src = O.trace(ids, 8)
    fc = outlines_to_geojson(src, table)
    want = []
    for r in range(len(table["label"])):
        js = [j for j in range(len(src["ring_value"])) if src["ring_value"][j] == r]
        js = [j for j in js if src["ring_area2"][j] > 0] + [j for j in js if src["ring_area2"][j] < 0]
        coords = [[list(p) for p in O.ring(src, j)] + [list(O.ring(src, j)[0])] for j in js]
        want.append({"type": "Feature", "geometry": {"type": "Polygon", "coordinates": coords},
                     "properties": {"region": r, "label": int(table["label"][r]), "name": None,
                                    "area": int(table["area"][r]), "score": 0.25}})
    assert json.dumps(fc) == json.dumps({"type": "FeatureCollection", "features": want})
    assert all("hole" not in x for v in rings_by_region(src).values() for x in v)
    # and the simplified rings at t = 0 of a map without T-junctions inside edges describe the same polygons
    ids, table = R.regions(HOLE, 8)
    assert json.dumps(outlines_to_geojson(S.simplify(ids, O.trace(ids, 8), 0), table)) == \
        json.dumps(outlines_to_geojson(O.trace(ids, 8), table))


# ------------------------------------------------------------------ config
def test_config_keys_and_refusal():
    cfg = tiny_cfg()
    assert cfg.MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.ENABLED is False
    assert cfg.MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.TOLERANCE == 1.0
    m = build_model(cfg)
    assert m.regions_simplify is False and m.regions_simplify_tolerance == 1.0
    on = {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.OUTPUT": "labels",
          "MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.ENABLED": "True"}
    m = build_model(tiny_cfg(**on, **{"MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True",
                                      "MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.TOLERANCE": "2.5"}))
    assert m.regions_outlines is True and m.regions_simplify is True and m.regions_simplify_tolerance == 2.5
    with pytest.raises(ValueError, match="SIMPLIFY"):
        build_model(tiny_cfg(**on))                                      # without REGIONS.OUTLINES
    with pytest.raises(ValueError, match="TOLERANCE"):
        build_model(tiny_cfg(**on, **{"MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True",
                                      "MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.TOLERANCE": "-1.0"}))


# ------------------------------------------------------------------ the C ABI
NEW = ("catseg_outline_simplify_workspace", "catseg_outline_simplify_count", "catseg_outline_simplify_run",
       "catseg_outline_simplify_write")


def test_header_and_lib_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "catseg_hip_simplify.h")).read()
    declared = set(re.findall(r"\b(catseg_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    assert declared == set(NEW) == set(L.EXPORTED_INCLUDED)
    assert '#include "catseg_hip_simplify.h"' in open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    lib = L.load()
    for s in NEW:
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s


def test_workspace_and_argument_checks_without_gpu():
    """The host-side checks return before anything is launched: bad arguments are refused without a device."""
    lib = L.load()
    ws = lib.catseg_outline_simplify_workspace
    assert ws(0, 5, 4, -1) == 0 and ws(5, 0, 4, -1) == 0 and ws(5, 5, 0, -1) == 0
    assert ws(16384, 16384, 4, -1) > 0 and ws(16385, 8, 4, -1) == 0 and ws(8, 16385, 4, -1) == 0
    assert ws(2, 2, 36, -1) > 0 and ws(2, 2, 37, -1) == 0                  # more corners than 4 (H + 1) (W + 1)
    assert ws(2, 2, 8, 7) == 0 and ws(2, 2, 8, 8) > 0 and ws(2, 2, 8, 36) > 0 and ws(2, 2, 8, 37) == 0
    # 70 x 100 with 10 corners: 12 padded counts, one scan block (4 padded), 71 rows of 2 words and 101 columns of 2
    assert ws(70, 100, 10, -1) == 4 * (4 + 12 + 4 + 2 * 142 + 2 * 202)
    # 10 corners, 13 nodes: 12 ring starts, ten int columns of 16 (two of them the stack), 2 ints of anchor bits
    # padded to 8, one scan block (4 padded)
    assert ws(70, 100, 10, 13) == 4 * (4 + 12 + 10 * 16 + 8 + 4)
    nb, nn = ws(8, 8, 16, -1), ws(8, 8, 16, 20)
    p = 1 << 20                                     # an aligned non-null address, never dereferenced on these paths
    count = lambda *a: lib.catseg_outline_simplify_count(*a)
    assert count(None, 8, 8, 8, p, 4, p, 16, p, nb, None) == -1
    assert count(p, 8, 8, 7, p, 4, p, 16, p, nb, None) == -1               # ld < W
    assert count(p, 8, 16385, 16385, p, 4, p, 16, p, nb, None) == -1       # W > 16384
    assert b"16384" in lib.catseg_last_error()
    assert count(p, 8, 8, 8, None, 4, p, 16, p, nb, None) == -1            # no ring_offset
    assert count(p, 8, 8, 8, p, 4, None, 16, p, nb, None) == -1            # no vertices
    assert count(p, 8, 8, 8, p, 4, p + 4, 16, p, nb, None) == -1           # vertices not 8-byte aligned
    assert count(p, 8, 8, 8, p, 0, p, 16, p, nb, None) == -1               # no rings
    assert count(p, 8, 8, 8, p, 17, p, 16, p, nb, None) == -1              # more rings than corners
    assert count(p, 8, 8, 8, p, 4, p, 0, p, nb, None) == -1                # no corners
    assert count(p, 8, 8, 8, p, 4, p, 16, None, nb, None) == -1            # no workspace
    assert count(p, 8, 8, 8, p, 4, p, 16, p, nb - 4, None) == -1           # workspace too small
    assert count(p, 8, 8, 8, p, 4, p, 16, p + 4, nb, None) == -1           # workspace misaligned
    run = lambda *a: lib.catseg_outline_simplify_run(*a)
    assert run(p, 4, p, 16, 8, 8, -0.5, p, nb, 20, p, nn, None) == -1      # tolerance < 0
    assert b"tolerance" in lib.catseg_last_error()
    assert run(p, 4, p, 16, 8, 8, 16384.5, p, nb, 20, p, nn, None) == -1   # tolerance > 16384
    assert run(p, 4, p, 16, 8, 8, float("nan"), p, nb, 20, p, nn, None) == -1
    assert run(p, 4, p, 16, 8, 8, 1.0, p, nb, 15, p, nn, None) == -1       # fewer nodes than corners
    assert b"nodes" in lib.catseg_last_error()
    assert run(p, 4, p, 16, 8, 8, 1.0, p, nb, 4 * 81 + 1, p, 1 << 24, None) == -1
    assert run(p, 4, p, 16, 8, 8, 1.0, p, nb, 20, None, nn, None) == -1    # no node workspace
    assert run(p, 4, p, 16, 8, 8, 1.0, p, nb, 20, p, nn - 4, None) == -1   # node workspace too small
    assert run(p, 4, p, 16, 8, 8, 1.0, p, nb - 4, 20, p, nn, None) == -1   # map workspace too small
    assert run(None, 4, p, 16, 8, 8, 1.0, p, nb, 20, p, nn, None) == -1
    write = lambda *a: lib.catseg_outline_simplify_write(*a)
    good = (p, nn, 8, 8, 16, 20, 4, p, p, p, p, p, p, 4, p, 16, None)
    bad = lambda i, v: write(*(good[:i] + (v,) + good[i + 1:]))
    assert bad(0, None) == -1 and bad(1, nn - 4) == -1                     # node workspace
    assert bad(2, 16385) == -1 and bad(5, 15) == -1 and bad(6, 0) == -1    # H, nodes, rings
    assert bad(7, None) == -1 and bad(8, None) == -1 and bad(8, p + 4) == -1   # the source ring columns
    assert bad(9, None) == -1                                              # no ring_offset
    assert bad(10, None) == -1 and bad(11, None) == -1 and bad(12, None) == -1   # a null ring column
    assert bad(11, p + 4) == -1                                            # area2 not 8-byte aligned
    assert bad(13, -1) == -1 and bad(15, -1) == -1                         # capacities < 0
    assert bad(14, None) == -1 and bad(14, p + 4) == -1                    # vertices null / misaligned


def test_kernel_logic_on_the_host_against_brute_force(tmp_path):
    """tools/outline_simplify_host.cpp: the functions the kernels call, phase by phase and sequentially, on the GPU
    tests' shapes, against a brute-force recursive Douglas-Peucker, under the address and undefined-behaviour
    sanitizers.  A stand-alone program: nothing is loaded into this process."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "outline_simplify_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "outline_simplify_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])
