"""catseg_label_regions_* / catseg_sieve_labels (ops.label_regions, ops.sieve_labels) and MODEL.CATSEG_HIP.REGIONS
on the device.  Everything is exact equality against the numpy / scipy restatement (tests/regions_ref.py).

Every map goes in as a row-strided view of a wider buffer whose slack holds 0x7fffffff, negative values and a
label of the map; region ids, sieved maps and table columns come back in sentinel-filled buffers whose slack must
be untouched; the score's slack holds NaN."""
import os

import numpy as np
import pytest
import torch

import poison
import regions_ref as R
from cat_seg import build_model, ops
from cat_seg import _lib as L

from conftest import GOLDEN
from test_boundary_cpu import tiny_cfg
from test_label_regions_cpu import ONLY_SMALL, TIE

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 130), (130, 1), (64, 64), (65, 67), (127, 129), (200, 333)]
COLS = ("label", "area", "bbox", "first")


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def serpentine(H, W):
    """A one-pixel-wide path of label 1 through background 0: rows 1, 3, 5, ... from column 1 to W - 2, joined at
    alternating ends; the background stays one region (row 0 and the two outer columns): R = 2 for H, W >= 4."""
    m = np.zeros((H, W), np.int32)
    m[1::2, 1:W - 1] = 1
    for k, y in enumerate(range(2, H - 1, 2)):
        if W >= 3:
            m[y, W - 2 if k % 2 == 0 else 1] = 1
    return m


def blobs(H, W, n_labels, seed, cell=24, speckle=0.03):
    """Smooth blobs (a coarse random grid with wavy borders) with single-pixel speckle."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, n_labels, (H // cell + 3, W // cell + 3))
    yy = np.arange(H)[:, None] + 6 * np.sin(np.arange(W) / 11.0)[None, :] + 8
    xx = np.arange(W)[None, :] + 6 * np.cos(np.arange(H) / 9.0)[:, None] + 8
    m = coarse[(yy / cell).astype(int), (xx / cell).astype(int)]
    sp = rng.random((H, W)) < speckle
    m[sp] = rng.integers(0, n_labels, int(sp.sum()))
    return m.astype(np.int32)


def patterns(H, W):
    yy, xx = np.mgrid[:H, :W]
    rng = np.random.default_rng(H * 1000 + W)
    return {
        "uniform": np.full((H, W), 7),
        "checkerboard": (yy + xx) % 2,
        "vstripes1": xx % 2, "vstripes3": (xx // 3) % 2,
        "hstripes1": yy % 2, "hstripes3": (yy // 3) % 2,
        "rings": (np.maximum(abs(yy - H // 2), abs(xx - W // 2)) // 2) % 3,
        "serpentine": serpentine(H, W),
        "noise3": rng.integers(0, 3, (H, W)),
        "blobs": blobs(H, W, 5, seed=H + W),
    }


_REF = {}


def ref_regions(key, m, conn, clamp=-1, score=None):
    """The restatement, computed once per case and shared (the tests only read it)."""
    k = ("regions", key, conn, clamp, score is not None)
    if k not in _REF:
        _REF[k] = R.regions(m, conn, clamp, score)
    return _REF[k]


def ref_sieve(key, m, min_area, conn, clamp=-1):
    k = ("sieve", key, min_area, conn, clamp)
    if k not in _REF:
        _REF[k] = R.sieve(m, min_area, conn, clamp)
    return _REF[k]


def strided_input(m):
    """(buf, view): the int32 map as a view of a buffer 5 columns and 2 rows larger whose slack holds 0x7fffffff,
    negative values and a label that occurs in the map."""
    m = torch.as_tensor(np.ascontiguousarray(m), dtype=torch.int32)
    H, W = m.shape
    fill = torch.tensor([0x7fffffff, -1, int(m[0, 0]), -2 ** 31, int(m[-1, -1])], dtype=torch.int32)
    buf = fill[(torch.arange(H + 2)[:, None] + torch.arange(W + 5)[None, :]) % 5].contiguous()
    buf[:H, :W] = m
    buf = buf.cuda()
    return buf, buf[:H, :W]


def check_input_intact(buf, m):
    H, W = m.shape
    exp = strided_input(m)[0]
    assert torch.equal(buf, exp), "the input buffer changed"


def run_regions(key, m, conn, clamp=-1, score=None, capacity=None):
    """count + write into poisoned buffers against the restatement; returns R."""
    m = np.asarray(m).astype(np.int32)
    H, W = m.shape
    exp_ids, exp = ref_regions(key, m, conn, clamp, score)
    Rn = len(exp["area"])
    buf, view = strided_input(m)
    assert H == 1 or not view.is_contiguous()
    ws = ops.label_regions_count(view, connectivity=conn, clamp_pred=clamp)
    assert int(ws[0].item()) == Rn, (key, conn)
    cap = Rn if capacity is None else capacity
    ids_buf, ids = poison.out_buffer(H, W, 2, 5, torch.int32)
    bufs = {k: poison.filled((Rn + 16, 4) if k == "bbox" else (Rn + 16,), torch.int32, "cuda") for k in COLS}
    sview = None
    if score is not None:
        bufs["score_q16"] = poison.filled((Rn + 16,), torch.int64, "cuda")
        sview = poison.padded(torch.as_tensor(score, dtype=torch.float32).cuda(), 1, 3)[1]
    table = {k: b[:cap] for k, b in bufs.items()}
    ops.label_regions_write(view, ws, ids, table, clamp_pred=clamp, score=sview)
    torch.cuda.synchronize()
    assert int(ws[0].item()) == Rn                                   # R is reported in full whatever the capacity
    poison.check_untouched(ids_buf, H, W, f"region_ids {key}")
    assert np.array_equal(ids.cpu().numpy(), exp_ids), (key, conn)
    n = min(cap, Rn)
    for k, b in bufs.items():
        poison.check_untouched_flat(b.flatten(), n * (4 if k == "bbox" else 1), f"{k} {key} capacity {cap}")
        assert np.array_equal(b[:n].cpu().numpy(), exp[k][:n]), (key, conn, k)
    check_input_intact(buf, m)
    return Rn


def run_sieve(key, m, min_area, conn, clamp=-1):
    m = np.asarray(m).astype(np.int32)
    H, W = m.shape
    exp = ref_sieve(key, m, min_area, conn, clamp)
    buf, view = strided_input(m)
    out_buf, out = poison.out_buffer(H, W, 3, 7, torch.int32)
    assert ops.sieve_labels(view, min_area, connectivity=conn, clamp_pred=clamp, out=out) is out
    torch.cuda.synchronize()
    poison.check_untouched(out_buf, H, W, f"sieve {key}")
    assert np.array_equal(out.cpu().numpy(), exp), (key, min_area, conn)
    check_input_intact(buf, m)
    return out.cpu().numpy()


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_patterns_at_the_edges_of_the_tiling(shape, conn):
    H, W = shape
    for name, m in patterns(H, W).items():
        Rn = run_regions((shape, name), m, conn)
        if name == "uniform":
            assert Rn == 1
        if name == "checkerboard":
            assert Rn == (H * W if conn == 4 or min(H, W) == 1 else 2)      # the largest table: every pixel a root
        if name == "serpentine" and min(H, W) >= 4:
            assert Rn == 2                                                  # one equivalence chain across every border


@pytest.mark.parametrize("conn", [4, 8])
@pytest.mark.parametrize("shape", SHAPES)
def test_sieve_patterns(shape, conn):
    H, W = shape
    pats = patterns(H, W)
    for name in ("uniform", "checkerboard", "vstripes3", "rings", "serpentine", "noise3", "blobs"):
        for min_area in (1, 2, 8, H * W + 1):
            out = run_sieve((shape, name), pats[name], min_area, conn)
            if min_area in (1, H * W + 1):
                assert np.array_equal(out, pats[name])                      # the identity; nothing is large


def test_sieve_4_and_8_agree_where_the_restatement_does():
    m = blobs(127, 129, 5, seed=3)
    a, b = ref_sieve("agree", m, 8, 4), ref_sieve("agree", m, 8, 8)
    ga, gb = run_sieve("agree", m, 8, 4), run_sieve("agree", m, 8, 8)
    same = a == b
    assert 0.5 < same.mean() and np.array_equal(ga == gb, same)
    hs = np.full((65, 67), 1)
    hs[10:50, 5:60] = 2
    hs[20, 20] = 3                                                          # no diagonal contact decides anything
    assert np.array_equal(ref_sieve("agree2", hs, 4, 4), ref_sieve("agree2", hs, 4, 8))
    assert np.array_equal(run_sieve("agree2", hs, 4, 4), run_sieve("agree2", hs, 4, 8))


def test_sieve_tie_and_only_small_neighbours_across_a_tile_border():
    for conn in (4, 8):
        # the tie: column 64 (the first of the second tile column) holds pieces of area 2 between two regions of
        # equal area, 64 columns each, that lie in different tiles: the lower region number (the left one) wins
        m = np.empty((70, 129), np.int64)
        m[:, :64], m[:, 65:] = 1, 2
        m[:, 64] = 10 + np.arange(70) // 2
        out = run_sieve("tie", m, 6, conn)
        assert (out[:, :65] == 1).all() and (out[:, 65:] == 2).all()
        # only small neighbours: ONLY_SMALL across the corner of four tiles, ringed by a small moat
        m = np.full((70, 130), 8)
        m[61:67, 60:69] = np.arange(54).reshape(6, 9) + 100                 # a moat of single pixels, all small
        m[63:65, 63:66] = ONLY_SMALL
        out = run_sieve("only_small", m, 3, conn)
        assert np.array_equal(out[63:65, 63:66], ONLY_SMALL)
        # the CPU test's 3 x 3 tie, with its columns in two tiles
        m = np.full((66, 66), 7)
        m[62:65, 62:65] = TIE
        run_sieve("tie3", m, 3, conn)


def test_clamp_pred_fold_joins_across_what_were_borders():
    m = blobs(65, 67, 30, seed=5, cell=8, speckle=0.0)
    assert run_regions("fold", m, 8, clamp=20) < run_regions("fold", m, 8)
    run_regions("fold", m, 4, clamp=0)
    m = np.array([[20, 21, 3, 22]] * 66)
    assert run_regions("fold_cols", m, 4, clamp=20) == 3 and run_regions("fold_cols", m, 4) == 4
    for min_area in (2, 80):
        run_sieve("fold", blobs(65, 67, 30, seed=5, cell=8), min_area, 8, clamp=20)
    vals = np.array([-2 ** 31, -1, 0, 2 ** 31 - 1])
    ext = vals[np.random.default_rng(6).integers(0, 4, (67, 9))]
    run_regions("extreme", ext, 8)
    run_regions("extreme", ext, 4, clamp=0)


def test_score_sum_is_the_integer_sum_with_ties_to_even():
    H, W = 127, 129
    m = blobs(H, W, 5, seed=9)
    rng = np.random.default_rng(1)
    k = rng.integers(0, 65536, (H, W))
    score = ((k + 0.5) / 65536).astype(np.float32)                          # k + 0.5 over 65536: exact in fp32
    assert np.array_equal(score.astype(np.float64) * 65536, k + 0.5)
    score[rng.random((H, W)) < 0.2] = 0.0
    score[rng.random((H, W)) < 0.2] = 1.0
    score[rng.random((H, W)) < 0.2] = rng.random(1).astype(np.float32)[0]
    for conn in (4, 8):
        run_regions("score", m, conn, score=score)
    ids, table = ops.label_regions(torch.from_numpy(m).cuda(), score=torch.from_numpy(score).cuda())
    exp_ids, exp = ref_regions("score", m, 8, -1, score)
    assert set(table) == set(COLS) | {"score_q16", "score"}
    assert np.array_equal(ids.cpu().numpy(), exp_ids)
    for k2 in table:
        assert table[k2].shape[0] == len(exp["area"]) and np.array_equal(table[k2].cpu().numpy(), exp[k2]), k2
    assert table["score"].dtype == torch.float32 and table["score_q16"].dtype == torch.int64


def test_table_capacity_below_r():
    m = blobs(65, 67, 5, seed=2)
    Rn = len(ref_regions("cap", m, 8)[1]["area"])
    score = np.random.default_rng(3).random((65, 67)).astype(np.float32)
    for cap in (0, 1, Rn // 2, Rn - 1):
        assert run_regions("cap", m, 8, capacity=cap) == Rn
    run_regions("cap", m, 8, score=score, capacity=Rn // 3)


def test_deterministic_and_stream():
    m = torch.from_numpy(blobs(200, 333, 6, seed=4)).cuda()
    score = torch.rand(200, 333, device="cuda")
    a, b = ops.label_regions(m, score=score), ops.label_regions(m, score=score)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        c = ops.label_regions(m, score=score)
        sc = ops.sieve_labels(m, 8)
    torch.cuda.current_stream().wait_stream(s)
    sa, sb = ops.sieve_labels(m, 8), ops.sieve_labels(m, 8)
    torch.cuda.synchronize()
    for other in (b, c):
        poison.check_bit_identical(a[0], other[0], "region_ids")
        for k in a[1]:
            poison.check_bit_identical(a[1][k], other[1][k], k)
    poison.check_bit_identical(sa, sb, "sieve")
    poison.check_bit_identical(sa, sc, "sieve on a stream")


def test_no_host_synchronisation():
    m = torch.from_numpy(blobs(127, 129, 5, seed=7)).cuda()
    score = torch.rand(127, 129, device="cuda")
    Rn = ops.label_regions(m)[1]["area"].numel()
    table = {"label": torch.empty(Rn, dtype=torch.int32, device="cuda"), "area": torch.empty(Rn, dtype=torch.int32, device="cuda"),
             "bbox": torch.empty(Rn, 4, dtype=torch.int32, device="cuda"), "first": torch.empty(Rn, dtype=torch.int32, device="cuda"),
             "score_q16": torch.empty(Rn, dtype=torch.int64, device="cuda")}
    ids, out = torch.empty_like(m), torch.empty_like(m)
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except Exception as e:                                # this build of torch has no such mode on ROCm
        pytest.skip(f"torch.cuda.set_sync_debug_mode unsupported: {e}")
    try:
        ops.sieve_labels(m, 8, out=out)
        ws = ops.label_regions_count(m)
        ops.label_regions_write(m, ws, ids, table, score=score)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    exp_ids, exp = R.regions(m.cpu().numpy(), 8, -1, score.cpu().numpy())
    assert np.array_equal(ids.cpu().numpy(), exp_ids) and np.array_equal(table["score_q16"].cpu().numpy(), exp["score_q16"])
    assert np.array_equal(out.cpu().numpy(), R.sieve(m.cpu().numpy(), 8, 8))


def test_argument_checks():
    good = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    for fn in (ops.label_regions, lambda t, **k: ops.sieve_labels(t, 2, **k)):
        with pytest.raises(ValueError):
            fn(torch.zeros(8, 8, dtype=torch.int32))                          # a CPU tensor
        with pytest.raises(ValueError):
            fn(good.long())                                                   # not int32
        with pytest.raises(ValueError):
            fn(good.flatten().as_strided((4, 8), (4, 1)))                     # ld = 4 < W = 8
        with pytest.raises(ValueError):
            fn(good, connectivity=6)
    with pytest.raises(ValueError):
        ops.sieve_labels(good, 0)
    # the entry points themselves, by shape arguments only: nothing of that size is allocated or launched
    ws = torch.zeros(1024, dtype=torch.int32, device="cuda")
    out = torch.zeros(8, 8, dtype=torch.int32, device="cuda")
    assert L.load().catseg_label_regions_workspace(1 << 16, 1 << 15, 0) == 0
    assert L.load().catseg_label_regions_workspace(1 << 16, 1 << 15, 1) == 0
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.call("catseg_label_regions_count", good.data_ptr(), 1 << 16, 1 << 15, 1 << 15, -1, 8, ws.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="2\\^31"):
        L.call("catseg_sieve_labels", good.data_ptr(), 1 << 16, 1 << 15, 1 << 15, -1, 8, 2, out.data_ptr(), 1 << 15,
               ws.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="connectivity"):
        L.call("catseg_label_regions_count", good.data_ptr(), 8, 8, 8, -1, 6, ws.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="min_area"):
        L.call("catseg_sieve_labels", good.data_ptr(), 8, 8, 8, -1, 8, 0, out.data_ptr(), 8, ws.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="ld"):
        L.call("catseg_label_regions_count", good.data_ptr(), 8, 8, 7, -1, 8, ws.data_ptr(), 4096, None)
    with pytest.raises(RuntimeError, match="ld"):
        L.call("catseg_sieve_labels", good.data_ptr(), 8, 8, 7, -1, 8, 2, out.data_ptr(), 8, ws.data_ptr(), 4096, None)
    torch.cuda.synchronize()
    assert int(ws.abs().sum().item()) == 0 and int(good.abs().sum().item()) == 0 and int(out.abs().sum().item()) == 0


# ------------------------------------------------------------------ MODEL.CATSEG_HIP.REGIONS at the boundary
_MODELS = {}


def _model(**over):
    key = tuple(sorted(over.items()))
    if key not in _MODELS:
        m = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "labels", **over})).cuda().eval()
        m.sem_seg_head.predictor.set_class_tokens(dict(np.load(os.path.join(GOLDEN, "e2e_tiny_eval.npz")))["tokens"])
        _MODELS[key] = m
    return _MODELS[key]


def _regions_model(min_area, **over):
    return _model(**{"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": str(min_area), **over})


def _check_outputs(plain, got, min_area, conn=8):
    assert set(plain) == {"sem_seg_labels", "sem_seg_score"}                # a default model's keys, as they were
    assert set(got) == {"sem_seg_labels", "sem_seg_score", "sem_seg_regions", "regions_info"}
    want = ops.sieve_labels(plain["sem_seg_labels"], min_area, connectivity=conn) if min_area > 1 else plain["sem_seg_labels"]
    assert torch.equal(got["sem_seg_labels"], want)
    assert torch.equal(got["sem_seg_score"], plain["sem_seg_score"])
    lab = got["sem_seg_labels"].cpu().numpy()
    if min_area > 1:
        assert np.array_equal(lab, R.sieve(plain["sem_seg_labels"].cpu().numpy(), min_area, conn))
    exp_ids, exp = R.regions(lab, conn, -1, got["sem_seg_score"].cpu().numpy())
    assert got["sem_seg_regions"].dtype == torch.int32 and np.array_equal(got["sem_seg_regions"].cpu().numpy(), exp_ids)
    info = got["regions_info"]
    assert set(info) == {"label", "area", "bbox", "first", "score"}
    for k, v in info.items():
        assert v.is_cuda and np.array_equal(v.cpu().numpy(), exp[k]), k
    assert info["score"].dtype == torch.float32


@pytest.mark.parametrize("min_area", [0, 6])
def test_model_regions_graph_and_eager(min_area):
    gen = torch.Generator().manual_seed(3)
    a, b = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 384, 384), (3, 300, 352))]
    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    plain = _model()(inputs)
    outs = {}
    for graph in ("True", "False"):
        outs[graph] = _regions_model(min_area, **{"MODEL.CATSEG_HIP.GRAPH": graph})(inputs)
        assert len(outs[graph]) == 2
        for p, g in zip(plain, outs[graph]):
            _check_outputs(p, g, min_area)
    for g, e in zip(outs["True"], outs["False"]):
        for k in ("sem_seg_labels", "sem_seg_score", "sem_seg_regions"):
            poison.check_bit_identical(g[k], e[k], k)
        for k in g["regions_info"]:
            poison.check_bit_identical(g["regions_info"][k], e["regions_info"][k], k)


def test_model_regions_tiled():
    tiled = {"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": "64",
             "MODEL.CATSEG_HIP.TILED.STRIDE": "32", "MODEL.CATSEG_HIP.TILED.BATCH": "4"}
    img = (torch.rand((3, 96, 96), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)   # 2 x 2 tiles
    plain = _model(**tiled)([{"image": img}])[0]
    got = _regions_model(6, **{"MODEL.CATSEG_HIP.REGIONS.CONNECTIVITY": "4", **tiled})([{"image": img}])[0]
    assert got["sem_seg_labels"].shape == (96, 96)
    _check_outputs(plain, got, 6, conn=4)


def test_model_regions_reference_mode_and_sliding():
    """RETURN_ALL_IMAGES False returns one dict, TEST.SLIDING_WINDOW its 640 x 640 merge: both post-processed."""
    gen = torch.Generator().manual_seed(4)
    a, b = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 300, 352), (3, 384, 384))]
    one = {"MODEL.CATSEG_HIP.RETURN_ALL_IMAGES": "False"}
    plain, got = _model(**one)([{"image": a}, {"image": b}]), _regions_model(6, **one)([{"image": a}, {"image": b}])
    assert len(plain) == len(got) == 1
    _check_outputs(plain[0], got[0], 6)
    slide = {"TEST.SLIDING_WINDOW": "True"}
    inputs = [{"image": a}]                                                 # the 640 x 640 merge itself
    _check_outputs(_model(**slide)(inputs)[0], _regions_model(6, **slide)(inputs)[0], 6)


def test_model_regions_through_the_device_tta_merge():
    from cat_seg import SemanticSegmentorWithTTA
    from cat_seg.test_time_augmentation import DatasetMapperTTA
    img = (torch.rand((3, 60, 80), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)
    outs = []
    for over in ({}, {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.REGIONS.MIN_AREA": "6"}):
        cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", "MODEL.CATSEG_HIP.OUTPUT": "labels", **over})
        w = SemanticSegmentorWithTTA(cfg, _model(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", **over}),
                                     tta_mapper=DatasetMapperTTA(min_sizes=(48, 64), max_size=4000, flip=True))
        outs.append(w([{"image": img}])[0])
    assert outs[1]["sem_seg_labels"].shape == (60, 80)
    _check_outputs(outs[0], outs[1], 6)
