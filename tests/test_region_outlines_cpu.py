"""Host half of the region-outline feature: the sequential restatement (tests/outlines_ref.py), which the GPU tests
hold the kernels to, against the contract's known answers and its six properties on random maps; an independent
fill (matplotlib.path) of pixel centres; cat_seg.vectorize; the config key and its refusal; the C ABI entries and
their host-side argument checks; and the kernels' index logic (csrc/region_outlines_logic.h) run sequentially on
the host against a brute-force tracer (tools/region_outlines_host.cpp, built with the address and undefined-
behaviour sanitizers)."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import outlines_ref as O
import regions_ref as R
from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg.vectorize import outlines_to_geojson, rings_by_region

from conftest import ROOT
from test_boundary_cpu import tiny_cfg

HOLE = np.array([[0, 0, 0, 0, 0],
                 [0, 5, 5, 5, 0],
                 [0, 5, 0, 5, 0],
                 [0, 5, 5, 5, 0],
                 [0, 0, 0, 0, 0]])


def rings(t):
    return [O.ring(t, j) for j in range(len(t["ring_value"]))]


def test_single_pixel():
    t = O.trace([[7]])
    assert rings(t) == [[(0, 0), (1, 0), (1, 1), (0, 1)]]
    assert t["ring_value"].tolist() == [7] and t["ring_area2"].tolist() == [2] and t["ring_offset"].tolist() == [0, 4]
    assert t["ring_offset"].dtype == np.int32 and t["ring_value"].dtype == np.int32
    assert t["ring_area2"].dtype == np.int64 and t["vertices"].dtype == np.int32 and t["vertices"].shape == (4, 2)


def test_diagonal_pinch_turns_left_under_8_and_right_under_4():
    m = [[0, 1], [1, 0]]
    t = O.trace(m, 8)
    assert rings(t) == [[(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1)],
                        [(1, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2), (0, 1), (1, 1)]]
    assert t["ring_value"].tolist() == [0, 1] and t["ring_area2"].tolist() == [4, 4]
    t = O.trace(m, 4)
    assert rings(t) == [[(0, 0), (1, 0), (1, 1), (0, 1)], [(1, 0), (2, 0), (2, 1), (1, 1)],
                        [(0, 1), (1, 1), (1, 2), (0, 2)], [(1, 1), (2, 1), (2, 2), (1, 2)]]
    assert t["ring_value"].tolist() == [0, 1, 1, 0] and t["ring_area2"].tolist() == [2, 2, 2, 2]


@pytest.mark.parametrize("conn", [4, 8])
def test_ring_with_a_hole(conn):
    t = O.trace(HOLE, conn)
    assert rings(t) == [[(0, 0), (5, 0), (5, 5), (0, 5)],              # the frame of 0s, clockwise on screen
                        [(1, 1), (1, 4), (4, 4), (4, 1)],              # its hole (the 5s and the inner 0): the other way
                        [(1, 1), (4, 1), (4, 4), (1, 4)],              # the ring of 5s
                        [(2, 2), (2, 3), (3, 3), (3, 2)],              # its hole
                        [(2, 2), (3, 2), (3, 3), (2, 3)]]              # the inner 0
    assert t["ring_value"].tolist() == [0, 0, 5, 5, 0]
    assert t["ring_area2"].tolist() == [50, -18, 18, -2, 2]


def random_map(rng, H, W, nlab, p_keep=0.6):
    """Labels with horizontal smear, so that regions of many sizes, holes and pinches all occur."""
    m = rng.integers(0, nlab, (H, W))
    keep = rng.random((H, W)) < p_keep
    for x in range(1, W):
        m[:, x] = np.where(keep[:, x], m[:, x - 1], m[:, x])
    return m


CASES = [(1, 1, 2, 0), (1, 9, 2, 1), (7, 1, 2, 2), (2, 2, 2, 3), (5, 8, 2, 4), (13, 13, 3, 5), (24, 31, 3, 6),
         (40, 60, 4, 7), (37, 59, 2, 8)]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("H,W,nlab,seed", CASES)
def test_the_six_properties_on_region_ids(H, W, nlab, seed, conn):
    rng = np.random.default_rng(seed)
    ids, table = R.regions(random_map(rng, H, W, nlab), conn)
    t = O.trace(ids, conn)
    val, a2, off = t["ring_value"], t["ring_area2"], t["ring_offset"]
    n = len(table["area"])
    ext = np.flatnonzero(a2 > 0)
    # one exterior ring per region, in region order
    assert val[ext].tolist() == list(range(n))
    # which starts at the top-left corner of the region's first pixel, heading E: its first vertex is that
    # corner, and the next one lies to the right of it on the same lattice row
    for j, r in zip(ext, range(n)):
        fy, fx = divmod(int(table["first"][r]), W)
        pts = O.ring(t, j)
        assert pts[0] == (fx, fy) and pts[1][1] == fy and pts[1][0] > fx
    # signed areas sum to the pixel count
    assert np.bincount(val, weights=a2, minlength=n).astype(np.int64).tolist() == (2 * table["area"].astype(np.int64)).tolist()
    assert (a2 != 0).all()
    # even-odd fill reproduces every region
    for r in range(n):
        assert np.array_equal(O.fill(t, r, H, W), ids == r), r
    # corner bound, and collinear points are dropped: directions alternate between horizontal and vertical
    assert len(t["vertices"]) == off[-1] <= 4 * (H + 1) * (W + 1)
    for j in range(len(val)):
        pts = O.ring(t, j)
        assert len(pts) >= 4 and len(pts) % 2 == 0
        for i, (x0, y0) in enumerate(pts):
            x1, y1 = pts[(i + 1) % len(pts)]
            x2, y2 = pts[(i + 2) % len(pts)]
            assert (x0 == x1) != (y0 == y1) and (x1 == x2) != (y1 == y2) and (x0 == x1) != (x1 == x2)


def test_checkerboard_comes_close_to_the_corner_bound():
    H, W = 9, 12
    m = np.indices((H, W)).sum(0) & 1
    for conn in (4, 8):
        K = len(O.trace(m, conn)["vertices"])
        assert K == 4 * H * W <= 4 * (H + 1) * (W + 1)         # every pixel corner is a corner of its pixel's ring


@pytest.mark.parametrize("conn", [4, 8])
def test_pixel_centres_against_matplotlib_paths(conn):
    """An independent fill: pixel centres inside the exterior path and outside every hole path of the region."""
    mpath = pytest.importorskip("matplotlib.path")
    for seed, (H, W) in enumerate([(9, 14), (21, 17), (30, 40)]):
        rng = np.random.default_rng(100 + seed)
        ids, table = R.regions(random_map(rng, H, W, 3), conn)
        t = O.trace(ids, conn)
        yy, xx = np.mgrid[0:H, 0:W]
        centres = np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], 1)
        for r, group in rings_by_region(t).items():
            inside = np.zeros(H * W, bool)
            for g in group:                         # even-odd over the region's rings; a pinch vertex repeats
                v = g["vertices"].astype(np.float64)
                inside ^= mpath.Path(np.vstack([v, v[:1]]), closed=True).contains_points(centres)
            assert np.array_equal(inside.reshape(H, W), ids == r), (seed, r)


def test_rings_by_region_puts_the_exterior_first_and_keeps_start_order():
    ids, table = R.regions(HOLE, 8)
    t = O.trace(ids, 8)
    g = rings_by_region(t)
    assert list(g) == [0, 1, 2]
    assert [x["area2"] for x in g[0]] == [50, -18] and [x["area2"] for x in g[1]] == [18, -2]
    assert [x["area2"] for x in g[2]] == [2]
    assert g[1][1]["vertices"].tolist() == [[2, 2], [2, 3], [3, 3], [3, 2]]
    # two holes in one region: start order
    m = np.zeros((3, 7), int)
    m[1, 1] = m[1, 4] = 1
    ids, _ = R.regions(m, 4)
    g = rings_by_region(O.trace(ids, 4))
    assert [x["vertices"][0].tolist() for x in g[0]] == [[0, 0], [1, 1], [4, 1]]
    assert sum(x["area2"] for x in g[0]) == 2 * 19


def test_geojson_structure_holes_and_transform():
    ids, table = R.regions(HOLE, 8, score=np.full(HOLE.shape, 0.5, np.float32))
    t = O.trace(ids, 8)
    fc = outlines_to_geojson(t, table, class_names=["ground"] + ["?"] * 4 + ["roof"])
    json.loads(json.dumps(fc))                      # plain Python types throughout
    assert fc["type"] == "FeatureCollection" and len(fc["features"]) == 3
    f0, f1, f2 = fc["features"]
    assert [f["properties"]["label"] for f in (f0, f1, f2)] == [0, 5, 0]
    assert [f["properties"]["name"] for f in (f0, f1, f2)] == ["ground", "roof", "ground"]
    assert [f["properties"]["area"] for f in (f0, f1, f2)] == [16, 8, 1]
    assert [f["properties"]["score"] for f in (f0, f1, f2)] == [0.5, 0.5, 0.5]
    assert f1["geometry"] == {"type": "Polygon", "coordinates": [[[1, 1], [4, 1], [4, 4], [1, 4], [1, 1]],
                                                                 [[2, 2], [2, 3], [3, 3], [3, 2], [2, 2]]]}
    for f in fc["features"]:
        for ring in f["geometry"]["coordinates"]:
            assert ring[0] == ring[-1] and len(ring) >= 5
    assert len(f0["geometry"]["coordinates"]) == 2 and len(f2["geometry"]["coordinates"]) == 1
    # a north-up raster: 0.5 m pixels, origin (1000, 2000)
    fc = outlines_to_geojson(t, table, transform=(0.5, 0.0, 1000.0, 0.0, -0.5, 2000.0))
    assert fc["features"][1]["geometry"]["coordinates"][0] == [[1000.5, 1999.5], [1002.0, 1999.5], [1002.0, 1998.0],
                                                               [1000.5, 1998.0], [1000.5, 1999.5]]
    assert fc["features"][0]["properties"]["name"] is None
    with pytest.raises(ValueError, match="transform"):
        outlines_to_geojson(t, table, transform=(1, 0, 0))
    # rings that are not those of the table's regions are refused
    with pytest.raises(ValueError, match="region"):
        outlines_to_geojson(O.trace(HOLE, 8), table)


def test_config_key_and_refusal():
    cfg = tiny_cfg()
    assert cfg.MODEL.CATSEG_HIP.REGIONS.OUTLINES is False
    assert build_model(cfg).regions_outlines is False
    m = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.OUTPUT": "labels",
                                "MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True"}))
    assert m.regions is True and m.regions_outlines is True
    with pytest.raises(ValueError, match="OUTLINES"):
        build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True", "MODEL.CATSEG_HIP.OUTPUT": "labels"}))


NEW = ("catseg_region_outlines_workspace", "catseg_region_outlines_count", "catseg_region_outlines_rank",
       "catseg_region_outlines_write")


def test_header_and_lib_carry_the_symbols():
    declared = set(re.findall(r"\b(catseg_\w+)\s*\(", open(os.path.join(ROOT, "include", "catseg_hip.h")).read()))
    lib = L.load()
    for s in NEW:
        assert s in declared and s in L.EXPORTED and hasattr(lib, s), s


def test_workspace_and_argument_checks_without_gpu():
    """The host-side checks return before anything is launched: bad arguments are refused without a device."""
    lib = L.load()
    ws = lib.catseg_region_outlines_workspace
    assert ws(0, 5, -1) == 0 and ws(5, -1, -1) == 0 and ws(5, -1, 8) == 0
    assert ws(1 << 16, 1 << 15, -1) == 0                                   # H * W == 2^31
    assert ws(23169, 23169, -1) > 0 and ws(23169, 23170, -1) == 0          # 4 (H + 1) (W + 1) crosses 2^31
    # 70 x 100: 71 lattice rows of 2 words = 142 words -> 144 padded, one scan block (4 padded), 4 masks per
    # word, and 2 x 101 columns of 2 words of column bits
    assert ws(70, 100, -1) == 4 * (4 + 144 + 4 + 8 * 142 + 2 * (2 * 101 * 2))
    # 10 corners -> 12 padded: six int columns, one scan block (4 padded), two jump buffers of four ints
    assert ws(70, 100, 10) == 4 * (4 + 14 * 12 + 4)
    assert ws(2, 2, 36) > 0 and ws(2, 2, 37) == 0                          # more corners than 4 (H + 1) (W + 1)
    nb, nr = ws(8, 8, -1), ws(8, 8, 16)
    p = 1 << 20                                     # an aligned non-null address, never dereferenced on these paths
    count = lambda *a: lib.catseg_region_outlines_count(*a)
    assert count(None, 8, 8, 8, 8, p, nb, None) == -1
    assert count(p, 8, 8, 7, 8, p, nb, None) == -1                         # ld < W
    assert count(p, 8, 8, 8, 6, p, nb, None) == -1                         # connectivity 6
    assert count(p, 8, 8, 8, 8, p, nb - 4, None) == -1                     # workspace too small
    assert count(p, 8, 8, 8, 8, p + 4, nb, None) == -1                     # workspace misaligned
    assert count(p, 23169, 23170, 23170, 8, p, nb, None) == -1
    assert b"2^31" in lib.catseg_last_error()
    rank = lambda *a: lib.catseg_region_outlines_rank(*a)
    assert rank(p, 8, 8, 8, 8, p, nb, 0, p, nr, None) == -1                # no corners
    assert b"corners" in lib.catseg_last_error()
    assert rank(p, 8, 8, 8, 8, p, nb, 4 * 81 + 1, p, 1 << 20, None) == -1   # more than 4 (H + 1) (W + 1)
    assert rank(p, 8, 8, 8, 8, p, nb, 16, p, nr - 4, None) == -1           # ring workspace too small
    assert rank(p, 8, 8, 8, 8, p, nb, 16, p + 8, nr, None) == -1           # ring workspace misaligned
    assert rank(p, 8, 8, 8, 8, p, nb - 4, 16, p, nr, None) == -1           # map workspace too small
    assert rank(p, 8, 8, 8, 5, p, nb, 16, p, nr, None) == -1               # connectivity 5
    write = lambda *a: lib.catseg_region_outlines_write(*a)
    assert write(p, 8, 8, 8, p, nr, 16, None, p, p, 4, p, 16, None) == -1  # no ring_offset
    assert write(p, 8, 8, 8, p, nr, 16, p, None, p, 4, p, 16, None) == -1  # a null ring column
    assert write(p, 8, 8, 8, p, nr, 16, p, p, p, -1, p, 16, None) == -1    # capacity < 0
    assert write(p, 8, 8, 8, p, nr, 16, p, p, p, 4, None, 16, None) == -1  # no vertices
    assert write(p, 8, 8, 8, p, nr, 16, p, p, p, 4, p + 4, 16, None) == -1   # vertices not 8-byte aligned
    assert write(p, 8, 8, 8, p, nr, 16, p, p, p + 4, 4, p, 16, None) == -1   # area2 not 8-byte aligned
    assert write(p, 8, 8, 8, p, nr - 4, 16, p, p, p, 4, p, 16, None) == -1   # ring workspace too small
    assert write(p, 8, 8, 7, p, nr, 16, p, p, p, 4, p, 16, None) == -1     # ld < W


def test_kernel_logic_on_the_host_against_a_brute_force_tracer(tmp_path):
    """tools/region_outlines_host.cpp: the functions the kernels call per vertex and per corner, phase by phase in
    shuffled orders, on the GPU tests' shapes and patterns, under the address and undefined-behaviour sanitizers."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "region_outlines_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "region_outlines_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])
