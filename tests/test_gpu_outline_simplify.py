"""catseg_outline_simplify_* (ops.simplify_outlines) and MODEL.CATSEG_HIP.REGIONS.SIMPLIFY on the device.
Everything is exact equality against the sequential restatement (tests/simplify_ref.py): the node count N, ring
offsets, values, hole flags, the int64 shoelace sums and every vertex, in order.

Every map goes in as a row-strided view of a wider buffer with poisoned slack; the rings come back in sentinel-filled
buffers one element larger than needed, whose last element must be untouched."""
import os
import re

import numpy as np
import pytest
import torch

import outlines_ref as O
import poison
import simplify_ref as S
from cat_seg import _lib as L
from cat_seg import ops

from conftest import ROOT
from test_gpu_label_regions import _regions_model, strided_input
from test_region_outlines_cpu import random_map

pytestmark = pytest.mark.gpu

KEYS = ("ring_offset", "ring_value", "ring_area2", "ring_hole", "vertices")
DTYPES = {"ring_offset": torch.int32, "ring_value": torch.int32, "ring_area2": torch.int64, "ring_hole": torch.uint8,
          "vertices": torch.int32}
TOLERANCES = (0, 0.5, 1, 1.5, 3, 1000)
BLOCK_LEN = 512                                     # OS_BLOCK_LEN: arcs of at least this many edges take a workgroup


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


_SRC = {}


def source(key, m, conn):
    """The map's rings (the restatement's, computed once per case) on the host and on the device."""
    k = (key, conn)
    if k not in _SRC:
        src = O.trace(m, conn)
        _SRC[k] = (src, {n: torch.from_numpy(v).cuda() for n, v in src.items()})
    return _SRC[k]


def run(key, m, conn, tolerances=TOLERANCES):
    """count, run and write through their own entry points, into poisoned buffers, against the restatement; returns
    the restatement's detail of the last tolerance."""
    m = np.asarray(m).astype(np.int32)
    src, dev = source(key, m, conn)
    NR = len(src["ring_value"])
    buf, view = strided_input(m)
    ws = ops.simplify_outlines_count(view, dev)
    det = None
    for t in tolerances:
        what = (key, conn, t)
        det = S.detail(m, src, t)
        exp = S.simplify(m, src, t, det)
        N = int(ws[0].item())
        assert N == S.count_nodes(det), what
        nws = ops.simplify_outlines_run(view, dev, ws, N, t)
        K2 = int(nws[1].item())
        assert K2 == len(exp["vertices"]), what
        bufs = {"ring_offset": poison.filled((NR + 2,), torch.int32, "cuda"),
                "ring_value": poison.filled((NR + 1,), torch.int32, "cuda"),
                "ring_area2": poison.filled((NR + 1,), torch.int64, "cuda"),
                "ring_hole": poison.filled((NR + 1,), torch.uint8, "cuda"),
                "vertices": poison.filled((K2 + 1, 2), torch.int32, "cuda")}
        out = {"ring_offset": bufs["ring_offset"][:NR + 1], "ring_value": bufs["ring_value"][:NR],
               "ring_area2": bufs["ring_area2"][:NR], "ring_hole": bufs["ring_hole"][:NR],
               "vertices": bufs["vertices"][:K2]}
        ops.simplify_outlines_write(view, dev, nws, N, out)
        for k in KEYS:
            assert np.array_equal(out[k].cpu().numpy(), exp[k]), (what, k)
            poison.check_untouched_flat(bufs[k].flatten(), out[k].numel(), f"{what} {k}")
    assert torch.equal(buf, strided_input(m)[0]), "the input buffer changed"
    for n, v in src.items():
        assert np.array_equal(dev[n].cpu().numpy(), v), f"the source {n} changed"
    return det


SHAPES = [(1, 1), (1, 9), (7, 1), (13, 13), (24, 31), (37, 59), (40, 60), (3, 63), (3, 64), (3, 65), (3, 129), (63, 3),
          (64, 3), (65, 3), (129, 3), (70, 130)]


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_random_maps(shape, conn):
    """The shapes of the outlines tests, and widths and heights round the word edges of the row and column bitmaps."""
    H, W = shape
    run(("smear", shape), random_map(np.random.default_rng(H * 1000 + W), H, W, 3), conn)


@pytest.mark.parametrize("conn", [4, 8])
def test_pinch_and_hand_derived_maps(conn):
    run("pinch", [[0, 1], [1, 0]], conn)
    run("tee", [[1, 1], [2, 3]], conn)
    run("stairs", [[1, 1, 1, 1], [2, 1, 1, 1], [2, 2, 1, 1], [2, 2, 2, 1]], conn, (0.5, 1))
    hole = np.zeros((5, 5), int)
    hole[1:4, 1:4] = 5
    hole[2, 2] = 0
    run("hole", hole, conn, (0, 1, 1.5, 2.5))


def coast(W, heights, H=8):
    """Label 1 above label 2; column x has heights[x % len(heights)] rows of label 1."""
    h = np.asarray([heights[x % len(heights)] for x in range(W)])
    return np.where(np.arange(H)[:, None] < h[None, :], 1, 2)


def test_sawtooth_coastline_is_one_arc_of_thousands_of_nodes():
    m = coast(3000, (2, 3, 4, 5, 4, 3))
    det = run("sawtooth", m, 8)
    assert max(a["len"] for ring in det for a in ring["arcs"]) == 2 * 2999 + 1


def island(changes, H=8):
    """A region of label 2 inside label 1 whose top edge steps at `changes` places: a ring without anchors of
    2 * changes + 4 corners."""
    m = np.ones((H, changes + 3), int)
    for x in range(changes + 1):
        m[(3 if x % 2 == 0 else 4):6, 1 + x] = 2
    return m


@pytest.mark.parametrize("length", [BLOCK_LEN - 1, BLOCK_LEN, BLOCK_LEN + 1])
def test_arcs_at_the_workgroup_threshold(length):
    """An open arc between two frame junctions has an odd number of edges, a closed arc an even one."""
    src = open(os.path.join(ROOT, "cat-seg_amd", "csrc", "outline_simplify_logic.h")).read()
    assert int(re.search(r"OS_BLOCK_LEN = (\d+);", src).group(1)) == BLOCK_LEN
    if length % 2:
        m = coast((length - 1) // 2 + 1, (3, 4))
    else:
        m = island((length - 4) // 2)
    det = run(("threshold", length), m, 8)
    assert length in {a["len"] for ring in det for a in ring["arcs"]}


def test_composed_call_allocates_exactly_and_is_deterministic():
    m = random_map(np.random.default_rng(77), 70, 130, 4).astype(np.int32)
    ids = torch.from_numpy(m).cuda()
    outl = ops.region_outlines(ids)
    src = {k: v.cpu().numpy() for k, v in outl.items()}
    exp = S.simplify(m, src, 1.0)
    a, b = ops.simplify_outlines(ids, outl, 1.0), ops.simplify_outlines(ids, outl, 1.0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = ops.simplify_outlines(ids, outl, 1.0)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert set(a) == set(KEYS)
    for k in KEYS:
        assert a[k].is_cuda and a[k].dtype == DTYPES[k] and tuple(a[k].shape) == exp[k].shape, k
        assert np.array_equal(a[k].cpu().numpy(), exp[k]), k
        poison.check_bit_identical(a[k], b[k], k)
        poison.check_bit_identical(a[k], c[k], k)


def test_capacities_below_nr_and_k():
    """Nothing is stored beyond a capacity, and what lies below it is the restatement's."""
    m = random_map(np.random.default_rng(3), 40, 45, 3).astype(np.int32)
    src, dev = source("cap", m, 8)
    exp = S.simplify(m, src, 1.0)
    ids = torch.from_numpy(m).cuda()
    ws = ops.simplify_outlines_count(ids, dev)
    N = int(ws[0].item())
    nws = ops.simplify_outlines_run(ids, dev, ws, N, 1.0)
    NR, K2 = len(exp["ring_value"]), len(exp["vertices"])
    assert int(nws[1].item()) == K2
    slack = 5
    for rcap, vcap in ((NR - 1, K2 - 1), (NR // 2, K2 // 3), (1, 2), (0, 0), (NR + 3, K2 + 4)):
        bufs = {"ring_offset": poison.filled((rcap + 1 + slack,), torch.int32, "cuda"),
                "ring_value": poison.filled((rcap + slack,), torch.int32, "cuda"),
                "ring_area2": poison.filled((rcap + slack,), torch.int64, "cuda"),
                "ring_hole": poison.filled((rcap + slack,), torch.uint8, "cuda"),
                "vertices": poison.filled((vcap + slack, 2), torch.int32, "cuda")}
        out = {k: bufs[k][:(rcap + 1 if k == "ring_offset" else vcap if k == "vertices" else rcap)] for k in KEYS}
        ops.simplify_outlines_write(ids, dev, nws, N, out)
        nr, nv = min(NR, rcap), min(K2, vcap)
        what = f"capacities {rcap}, {vcap}"
        assert np.array_equal(bufs["ring_offset"][:nr + 1].cpu().numpy(), exp["ring_offset"][:nr + 1]), what
        for k in ("ring_value", "ring_hole"):
            assert np.array_equal(bufs[k][:nr].cpu().numpy(), exp[k][:nr]), (what, k)
            poison.check_untouched_flat(bufs[k], nr, f"{what} {k}")
        assert np.array_equal(bufs["vertices"][:nv].cpu().numpy(), exp["vertices"][:nv]), what
        # a ring's area is summed over all its kept vertices, whatever the vertex capacity
        assert np.array_equal(bufs["ring_area2"][:nr].cpu().numpy(), exp["ring_area2"][:nr]), what
        poison.check_untouched_flat(bufs["ring_offset"], nr + 1, what + " ring_offset")
        poison.check_untouched_flat(bufs["ring_area2"], nr, what + " ring_area2")
        poison.check_untouched_flat(bufs["vertices"].flatten(), 2 * nv, what + " vertices")


def test_argument_checks():
    good = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    outl = ops.region_outlines(good)
    for bad_ids in (good.cpu(), good.long(), good[None], good.flatten().as_strided((4, 8), (4, 1))):
        with pytest.raises(ValueError):
            ops.simplify_outlines(bad_ids, outl, 1.0)
    for t in (-0.1, 16384.5, float("nan")):
        with pytest.raises(ValueError, match="tolerance"):
            ops.simplify_outlines(good, outl, t)
    for k, bad in (("ring_offset", outl["ring_offset"].long()), ("vertices", outl["vertices"].cpu()),
                   ("vertices", outl["vertices"].flatten()), ("ring_area2", outl["ring_area2"][:0]),
                   ("ring_value", outl["ring_value"].repeat(9))):
        with pytest.raises(ValueError):
            ops.simplify_outlines(good, {**outl, k: bad}, 1.0)
    ws = ops.simplify_outlines_count(good, outl)
    with pytest.raises(ValueError, match="nodes"):
        ops.simplify_outlines_run(good, outl, ws, 3, 1.0)                    # fewer nodes than corners
    got = ops.simplify_outlines(good, outl, 1.0)                              # the constant map after all that
    assert got["vertices"].tolist() == [[0, 0], [8, 0], [8, 8], [0, 8]] and got["ring_area2"].tolist() == [128]
    assert got["ring_offset"].tolist() == [0, 4] and got["ring_value"].tolist() == [0] and got["ring_hole"].tolist() == [0]


# ------------------------------------------------------------------ MODEL.CATSEG_HIP.REGIONS.SIMPLIFY at the boundary
def test_model_simplified_outlines():
    gen = torch.Generator().manual_seed(3)
    a, b = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 384, 384), (3, 300, 352))]
    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    off = {"MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True"}
    on = {**off, "MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.ENABLED": "True", "MODEL.CATSEG_HIP.REGIONS.SIMPLIFY.TOLERANCE": "1.5"}
    plain, got = _regions_model(6, **off)(inputs), _regions_model(6, **on)(inputs)
    assert len(got) == len(plain) == 2
    for p, g in zip(plain, got):
        assert set(g) == set(p) | {"regions_outlines_simplified"}
        for k in ("sem_seg_labels", "sem_seg_score", "sem_seg_regions"):     # the key adds, and changes nothing
            poison.check_bit_identical(g[k], p[k], k)
        for k in p["regions_info"]:
            poison.check_bit_identical(g["regions_info"][k], p["regions_info"][k], k)
        for k in p["regions_outlines"]:
            poison.check_bit_identical(g["regions_outlines"][k], p["regions_outlines"][k], k)
        want = ops.simplify_outlines(g["sem_seg_regions"], g["regions_outlines"], 1.5)
        assert set(g["regions_outlines_simplified"]) == set(KEYS)
        for k in KEYS:
            poison.check_bit_identical(g["regions_outlines_simplified"][k], want[k], k)
    # the smaller image against the restatement too
    ids = got[0]["sem_seg_regions"].cpu().numpy()
    exp = S.simplify(ids, O.trace(ids, 8), 1.5)
    for k in KEYS:
        assert np.array_equal(got[0]["regions_outlines_simplified"][k].cpu().numpy(), exp[k]), k
