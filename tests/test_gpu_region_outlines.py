"""catseg_region_outlines_* (ops.region_outlines) and MODEL.CATSEG_HIP.REGIONS.OUTLINES on the device.  Everything
is exact equality against the sequential restatement (tests/outlines_ref.py): ring offsets, values, the int64
shoelace sums and every vertex, in order.

Every map goes in as a row-strided view of a wider buffer whose slack holds 0x7fffffff, negative values and values
of the map; the rings come back in sentinel-filled buffers whose slack must be untouched."""
import numpy as np
import pytest
import torch

import outlines_ref as O
import poison
from cat_seg import _lib as L
from cat_seg import ops
from cat_seg.vectorize import rings_by_region

from test_gpu_label_regions import _model, _regions_model, strided_input

pytestmark = pytest.mark.gpu

KEYS = ("ring_offset", "ring_value", "ring_area2", "vertices")
DTYPES = {"ring_offset": torch.int32, "ring_value": torch.int32, "ring_area2": torch.int64, "vertices": torch.int32}


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


_REF = {}


def ref(key, m, conn):
    """The restatement, computed once per case and shared (the tests only read it)."""
    k = (key, conn)
    if k not in _REF:
        _REF[k] = O.trace(m, conn)
    return _REF[k]


def check_equal(got, exp, what):
    assert set(got) == set(KEYS), what
    for k in KEYS:
        g = got[k]
        assert g.is_cuda and g.dtype == DTYPES[k] and tuple(g.shape) == exp[k].shape, (what, k, tuple(g.shape), exp[k].shape)
        assert np.array_equal(g.cpu().numpy(), exp[k]), (what, k)


def run(key, m, conn):
    """ops.region_outlines of the map as a strided view with poisoned surroundings, against the restatement."""
    m = np.asarray(m).astype(np.int32)
    exp = ref(key, m, conn)
    buf, view = strided_input(m)
    got = ops.region_outlines(view, connectivity=conn)
    check_equal(got, exp, (key, conn))
    assert torch.equal(buf, strided_input(m)[0]), "the input buffer changed"
    return exp


def checkerboard(H, W):
    yy, xx = np.mgrid[:H, :W]
    return (yy + xx) % 2


def meander(H, W):
    """A one-pixel-wide path of 1s through background 0: bands of three rows in which the odd columns are vertical
    bars joined alternately at the top and at the bottom, the bands joined at alternating ends.  Two regions; the
    path's ring turns about twice per column and band."""
    m = np.zeros((H, W), np.int32)
    last = W - 2 if (W - 2) % 2 == 1 else W - 3
    bands = [y0 for y0 in range(1, H - 3, 4)]
    for b, y0 in enumerate(bands):
        for x in range(1, last + 1):
            if x % 2 == 1:
                m[y0:y0 + 3, x] = 1
            else:
                m[y0 if (x // 2) % 2 == 0 else y0 + 2, x] = 1
        if b + 1 < len(bands):
            m[y0 + 3, last if b % 2 == 0 else 1] = 1
    return m


def frames(H, W):
    """Nested one-pixel frames of alternating value: holes inside holes."""
    yy, xx = np.mgrid[:H, :W]
    return np.minimum(np.minimum(yy, H - 1 - yy), np.minimum(xx, W - 1 - xx)) % 2


def speckle_ids(H, W, conn, seed):
    """The region numbers ops.label_regions gives a random 3-label map."""
    m = torch.from_numpy(np.random.default_rng(seed).integers(0, 3, (H, W)).astype(np.int32)).cuda()
    ids, table = ops.label_regions(m, connectivity=conn)
    return ids.cpu().numpy(), {k: v.cpu().numpy() for k, v in table.items()}


@pytest.mark.parametrize("shape", [(70, 130), (1, 200), (200, 1), (1, 1)])
def test_constant_maps_are_one_ring_of_four_vertices(shape):
    """Single runs that cross every word border of the row and column bitmaps."""
    H, W = shape
    for conn in (4, 8):
        exp = run(("const", shape), np.full(shape, 7), conn)
        assert exp["vertices"].tolist() == [[0, 0], [W, 0], [W, H], [0, H]] and exp["ring_area2"].tolist() == [2 * H * W]


@pytest.mark.parametrize("conn", [4, 8])
def test_checkerboard(conn):
    H, W = 33, 65
    exp = run("checker", checkerboard(H, W), conn)
    assert len(exp["vertices"]) == 4 * H * W                     # about four corners per vertex
    if conn == 8:                                                # two regions, pinched everywhere: one exterior ring each,
        assert (exp["ring_area2"] > 0).sum() == 2                # and their rings hold thousands of corners each
        per_value = np.bincount(exp["ring_value"], weights=np.diff(exp["ring_offset"]))
        assert len(per_value) == 2 and per_value.min() > 2000
    else:
        assert len(exp["ring_value"]) == H * W


@pytest.mark.parametrize("conn", [4, 8])
def test_meander_is_one_ring_of_more_than_2048_corners(conn):
    """The deepest ranking: 12 rounds of pointer jumping all act on one ring."""
    exp = run("meander", meander(96, 96), conn)
    assert np.diff(exp["ring_offset"]).max() > 2 ** 11


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(20, 27), (65, 64)])
def test_nested_frames(shape, conn):
    exp = run(("frames", shape), frames(*shape), conn)
    assert (exp["ring_area2"] < 0).sum() == min(shape) // 2 - (1 if min(shape) % 2 == 0 else 0)


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", [(67, 129), (130, 67)])
def test_speckle_region_ids_and_the_contracts_properties(shape, conn):
    H, W = shape
    ids, table = speckle_ids(H, W, conn, seed=H)
    exp = run(("speckle", shape), ids, conn)
    n = len(table["area"])
    ext = np.flatnonzero(exp["ring_area2"] > 0)
    assert exp["ring_value"][ext].tolist() == list(range(n))     # one exterior ring per region, in region order
    first = exp["vertices"][exp["ring_offset"][ext]]
    assert np.array_equal(first[:, 1] * W + first[:, 0], table["first"])
    sums = np.zeros(n, np.int64)
    np.add.at(sums, exp["ring_value"], exp["ring_area2"])
    assert np.array_equal(sums, 2 * table["area"].astype(np.int64))
    for r in (0, n // 2, n - 1):
        assert np.array_equal(O.fill(exp, r, H, W), ids == r)


def test_values_are_compared_as_any_int32():
    m = np.array([[-2 ** 31, 2 ** 31 - 1, 0], [-1, -1, 0]], np.int32)
    for conn in (4, 8):
        exp = run("extremes", m, conn)
        assert exp["ring_value"].tolist() == [-2 ** 31, 2 ** 31 - 1, 0, -1]


def test_capacities_below_nr_and_k():
    """Nothing is stored beyond a capacity: rings below the ring capacity and vertices below the vertex capacity are
    the restatement's, everything behind them keeps its sentinel."""
    ids, _ = speckle_ids(40, 45, 8, seed=11)
    exp = ref("cap", ids, 8)
    NR, K = len(exp["ring_value"]), len(exp["vertices"])
    m = torch.from_numpy(ids).cuda()
    ws = ops.region_outlines_count(m)
    assert int(ws[0].item()) == K
    rws = ops.region_outlines_rank(m, ws, K)
    assert int(rws[1].item()) == NR
    slack = 7
    for rcap, vcap in ((NR, K), (NR - 1, K - 1), (NR // 2, K // 3), (1, 4), (0, 0), (NR + 3, K + 5)):
        bufs = {"ring_offset": poison.filled((rcap + 1 + slack,), torch.int32, "cuda"),
                "ring_value": poison.filled((rcap + slack,), torch.int32, "cuda"),
                "ring_area2": poison.filled((rcap + slack,), torch.int64, "cuda"),
                "vertices": poison.filled((vcap + slack, 2), torch.int32, "cuda")}
        out = {"ring_offset": bufs["ring_offset"][:rcap + 1], "ring_value": bufs["ring_value"][:rcap],
               "ring_area2": bufs["ring_area2"][:rcap], "vertices": bufs["vertices"][:vcap]}
        ops.region_outlines_write(m, rws, K, out)
        nr, nv = min(NR, rcap), min(K, vcap)
        what = f"capacities {rcap}, {vcap}"
        assert np.array_equal(bufs["ring_offset"][:nr + 1].cpu().numpy(), exp["ring_offset"][:nr + 1]), what
        assert np.array_equal(bufs["ring_value"][:nr].cpu().numpy(), exp["ring_value"][:nr]), what
        assert np.array_equal(bufs["ring_area2"][:nr].cpu().numpy(), exp["ring_area2"][:nr]), what
        assert np.array_equal(bufs["vertices"][:nv].cpu().numpy(), exp["vertices"][:nv]), what
        poison.check_untouched_flat(bufs["ring_offset"], nr + 1, what + " ring_offset")
        poison.check_untouched_flat(bufs["ring_value"], nr, what + " ring_value")
        poison.check_untouched_flat(bufs["ring_area2"], nr, what + " ring_area2")
        poison.check_untouched_flat(bufs["vertices"].flatten(), 2 * nv, what + " vertices")


def test_deterministic_and_stream():
    ids, _ = speckle_ids(130, 200, 8, seed=4)
    m = torch.from_numpy(ids).cuda()
    a, b = ops.region_outlines(m), ops.region_outlines(m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = ops.region_outlines(m)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for other in (b, c):
        for k in KEYS:
            poison.check_bit_identical(a[k], other[k], k)


def test_the_halves_do_no_host_synchronisation():
    ids, _ = speckle_ids(67, 129, 8, seed=7)
    m = torch.from_numpy(ids).cuda()
    exp = ref("nosync", ids, 8)
    NR, K = len(exp["ring_value"]), len(exp["vertices"])
    out = {"ring_offset": torch.empty(NR + 1, dtype=torch.int32, device="cuda"),
           "ring_value": torch.empty(NR, dtype=torch.int32, device="cuda"),
           "ring_area2": torch.empty(NR, dtype=torch.int64, device="cuda"),
           "vertices": torch.empty(K, 2, dtype=torch.int32, device="cuda")}
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                # this build of torch has no such mode on ROCm
        pytest.skip(f"torch.cuda.set_sync_debug_mode unsupported: {e}")
    try:
        ws = ops.region_outlines_count(m)
        rws = ops.region_outlines_rank(m, ws, K)
        ops.region_outlines_write(m, rws, K, out)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(ws[0].item()) == K and int(rws[1].item()) == NR
    check_equal(out, exp, "halves")


def test_argument_checks():
    good = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.region_outlines(torch.zeros(8, 8, dtype=torch.int32))             # a CPU tensor
    with pytest.raises(ValueError):
        ops.region_outlines(good.long())                                      # not int32
    with pytest.raises(ValueError):
        ops.region_outlines(good[None])                                       # not 2-D
    with pytest.raises(ValueError):
        ops.region_outlines(good.flatten().as_strided((4, 8), (4, 1)))        # ld = 4 < W = 8
    with pytest.raises(ValueError):
        ops.region_outlines(good, connectivity=6)
    ws = ops.region_outlines_count(good)
    with pytest.raises(ValueError):
        ops.region_outlines_rank(good, ws, 0)
    with pytest.raises(ValueError):
        ops.region_outlines_rank(good, ws, 4 * 81 + 1)                        # more than 4 (H + 1) (W + 1)
    rws = ops.region_outlines_rank(good, ws, 4)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device="cuda")
    ok = {"ring_offset": i32(2), "ring_value": i32(1), "ring_area2": torch.zeros(1, dtype=torch.int64, device="cuda"),
          "vertices": i32(4, 2)}
    for k, bad in (("ring_offset", i32(1)), ("ring_area2", i32(1)), ("vertices", i32(4, 3)), ("ring_value", i32(1).cpu())):
        with pytest.raises(ValueError):
            ops.region_outlines_write(good, rws, 4, {**ok, k: bad})
    # the entry points themselves, by shape arguments only: nothing of that size is allocated or launched
    big = torch.zeros(1024, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.call("catseg_region_outlines_count", good.data_ptr(), 23169, 23170, 23170, 8, big.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="connectivity"):
        L.call("catseg_region_outlines_count", good.data_ptr(), 8, 8, 8, 6, big.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="ld"):
        L.call("catseg_region_outlines_count", good.data_ptr(), 8, 8, 7, 8, big.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="workspace"):
        L.call("catseg_region_outlines_count", good.data_ptr(), 8, 8, 8, 8, big.data_ptr(), 64, None)
    torch.cuda.synchronize()
    assert int(big.abs().sum().item()) == 0 and int(good.abs().sum().item()) == 0
    ops.region_outlines_write(good, rws, 4, ok)                               # the constant map after all that
    assert ok["vertices"].tolist() == [[0, 0], [8, 0], [8, 8], [0, 8]] and ok["ring_area2"].tolist() == [128]
    assert ok["ring_offset"].tolist() == [0, 4] and ok["ring_value"].tolist() == [0]


# ------------------------------------------------------------------ MODEL.CATSEG_HIP.REGIONS.OUTLINES at the boundary
def _check_model_outlines(plain, got, conn):
    assert set(got) == set(plain) | {"regions_outlines"}
    for k in ("sem_seg_labels", "sem_seg_score", "sem_seg_regions"):         # the key adds, and changes nothing
        poison.check_bit_identical(got[k], plain[k], k)
    for k in plain["regions_info"]:
        poison.check_bit_identical(got["regions_info"][k], plain["regions_info"][k], k)
    want = ops.region_outlines(got["sem_seg_regions"], connectivity=conn)
    for k in KEYS:
        poison.check_bit_identical(got["regions_outlines"][k], want[k], k)
    groups = rings_by_region(got["regions_outlines"])
    area = got["regions_info"]["area"].cpu().numpy()
    assert list(groups) == list(range(len(area)))
    assert [sum(g["area2"] for g in groups[r]) for r in range(len(area))] == (2 * area.astype(np.int64)).tolist()
    assert all(groups[r][0]["area2"] > 0 and all(g["area2"] < 0 for g in groups[r][1:]) for r in groups)


def test_model_outlines_plain():
    gen = torch.Generator().manual_seed(3)
    a, b = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 384, 384), (3, 300, 352))]
    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    plain = _regions_model(6)(inputs)
    got = _regions_model(6, **{"MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True"})(inputs)
    assert len(got) == 2
    for p, g in zip(plain, got):
        _check_model_outlines(p, g, 8)
    # the smaller image against the restatement too
    ids = got[0]["sem_seg_regions"].cpu().numpy()
    check_equal(got[0]["regions_outlines"], O.trace(ids, 8), "model")


def test_model_outlines_tiled():
    tiled = {"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": "64",
             "MODEL.CATSEG_HIP.TILED.STRIDE": "32", "MODEL.CATSEG_HIP.TILED.BATCH": "4",
             "MODEL.CATSEG_HIP.REGIONS.CONNECTIVITY": "4"}
    img = (torch.rand((3, 96, 96), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)   # 2 x 2 tiles
    plain = _regions_model(6, **tiled)([{"image": img}])[0]
    got = _regions_model(6, **{"MODEL.CATSEG_HIP.REGIONS.OUTLINES": "True", **tiled})([{"image": img}])[0]
    assert got["sem_seg_regions"].shape == (96, 96)
    _check_model_outlines(plain, got, 4)
    check_equal(got["regions_outlines"], O.trace(got["sem_seg_regions"].cpu().numpy(), 4), "tiled model")
