"""catseg_boundary_distance / catseg_boundary_confusion (ops.boundary_distance, ops.boundary_confusion) on the device.
Everything is exact integer equality against the numpy restatement (tests/boundary_ref.py), which
tests/test_boundary_eval_cpu.py ties to scipy's erosion, to the definition and to hand answers.

The distance has one path for every cap (the column pass reads as far as the distances in the map reach, never a
halo sized by cap), so no case below switches kernels; the caps still straddle the 64-pixel words of the row pass
(cap 40, 64, 100, 150, 300) and the distances run across several 64 x 4 workgroup tiles in both axes.  The counters
have two paths: N = 5 with up to 8 widths sums in LDS (8 * 51 counters); `test_counters_without_lds` takes the
global-atomic path with N = 40 and 8 widths (8 * 1801 > 8192 counters)."""
import numpy as np
import pytest
import torch

import boundary_ref as B
import poison
from cat_seg import _lib as L
from cat_seg import ops

from test_region_outlines_cpu import random_map

pytestmark = pytest.mark.gpu

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def dev(m):
    return torch.from_numpy(np.ascontiguousarray(m).astype(np.int32)).cuda()


def speckled(seed, H, W, nlab=3):
    rng = np.random.default_rng(seed)
    m = random_map(rng, H, W, nlab)
    return np.where(rng.random((H, W)) < 0.02, rng.integers(0, nlab, (H, W)), m)


def check_distance(m, cap, clamp_pred=-1, what=""):
    got = ops.boundary_distance(dev(m), cap, clamp_pred=clamp_pred)
    assert got.dtype == torch.int16 and tuple(got.shape) == np.asarray(m).shape
    exp = B.distance(m, cap, clamp_pred)
    got = got.cpu().numpy()
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, cap, len(bad), bad[:5].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
    return exp


# ------------------------------------------------------------------ the distance
@pytest.mark.parametrize("H,W", [(1, 1), (1, 130), (130, 1), (63, 64), (64, 65), (70, 100), (129, 67)])
def test_distance_on_random_maps(H, W):
    m = speckled(1000 * H + W, H, W)
    for cap in (1, 2, 7, 40):
        exp = check_distance(m, cap, what=(H, W))
        assert exp.min() == 1 and exp.max() <= cap


def test_distance_uniform_map():
    m = np.full((200, 150), 4)
    for cap in (5, 64, 300):                        # 300: larger than any distance in the map (max 75)
        exp = check_distance(m, cap, what="uniform")
        assert exp.max() == min(cap, 75)


def test_distance_checkerboard():
    yy, xx = np.mgrid[:33, :47]
    assert (check_distance((yy + xx) % 2, 9, what="checkerboard") == 1).all()


def test_distance_block_across_tiles():
    m = np.full((200, 210), 1)
    m[20:170, 30:180] = 2                           # 150 x 150: distances up to 75 across several tiles in both axes
    assert check_distance(m, 100, what="block").max() == 75


def test_distance_blocks_large_cap():
    yy, xx = np.mgrid[:400, :330]
    m = (yy // 60) * 7 + xx // 60                   # 60-pixel blocks; cap 150 > every distance (30)
    assert check_distance(m, 150, what="blocks").max() == 30


def test_distance_any_int32_is_a_label():
    rng = np.random.default_rng(5)
    vals = np.array([-1, 255, I32_MIN, I32_MAX, 0, I32_MAX - 1], np.int64)
    m = vals[random_map(rng, 66, 90, 6)]
    check_distance(m, 12, what="wild labels")


def test_distance_fold():
    m = speckled(8, 70, 100, 5)
    exp = check_distance(m, 9, clamp_pred=2, what="fold")
    assert not np.array_equal(exp, B.distance(m, 9))                  # the fold changes the answer
    assert np.array_equal(exp, B.distance(np.minimum(m, 2), 9))


def test_distance_strided_views_in_poisoned_buffers():
    """The map is a row-strided view whose slack holds a sentinel label (reading it would shorten distances), the
    result a row-strided view of a sentinel-filled int16 buffer (a store outside breaks a sentinel, an unwritten
    element keeps the fill, which is no distance: it is negative)."""
    m = speckled(11, 70, 100)
    exp = B.distance(m, 40)
    buf, view = poison.padded(dev(m), 3, 29)
    assert view.stride(0) == 129
    obuf, out = poison.out_buffer(70, 100, 2, 13, torch.int16)
    got = ops.boundary_distance(view, 40, out=out)
    assert got is out
    poison.check_untouched(obuf, 70, 100, "boundary_distance")
    poison.check_no_nan(out, "boundary_distance")
    assert np.array_equal(out.cpu().numpy(), exp)
    assert bool(poison.holds_fill(buf[70:]).all()) and bool(poison.holds_fill(buf[:, 100:]).all())
    # the same call twice: the same bytes
    again = ops.boundary_distance(view, 40)
    poison.check_bit_identical(again, out.contiguous(), "boundary_distance twice")
    with pytest.raises(ValueError):
        ops.boundary_distance(view, 0)
    with pytest.raises(ValueError):
        ops.boundary_distance(view, 16385)
    with pytest.raises(ValueError):
        ops.boundary_distance(view, 4, out=torch.empty((70, 100), dtype=torch.int32, device="cuda"))


# ------------------------------------------------------------------ the counters
N = 5
WIDTHS8 = [1, 2, 3, 5, 8, 13, 21, 34]


def confusion_case(H, W, seed, pred_max):
    """Ground truth of 12-pixel blocks (a 75 x 75 block at the origin when the map holds one) with rectangular
    ignore patches and one label that is neither a class nor the ignore label; the prediction is the ground truth
    shifted by (2, 1) with 5 % speckle of labels 0 .. pred_max."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    G = (yy // 12 + 2 * (xx // 12)) % N
    if H >= 100 and W >= 100:
        G[:75, :75] = 1
    P = np.roll(G, (2, 1), (0, 1))
    P = np.where(rng.random((H, W)) < 0.05, rng.integers(0, pred_max + 1, (H, W)), P)
    G[5:12, W - 20:W - 8] = 255                    # the patches and the stray label lie outside the 75 x 75 block
    G[H - 9:H - 2, W // 2:W // 2 + 7] = 255
    G[H - 1, 3] = 77
    return P, G


def check_counters(P, G, widths, clamp_pred, n=N):
    exp = B.counters(P, G, widths, n, 255, clamp_pred)
    dG = B.distance(G, max(widths) + 1)
    classes = (G >= 0) & (G < n)
    for w in widths:                                # no band is empty or the whole map, so neither can pass by accident
        assert (classes & (dG <= w)).any() and (classes & (dG > w)).any(), w
    got = torch.zeros(exp.size, dtype=torch.int64, device="cuda")
    ops.boundary_confusion(dev(P), dev(G), widths, got, num_classes=n, clamp_pred=clamp_pred)
    got = got.cpu().numpy()
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (widths, clamp_pred, bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
    return exp


@pytest.mark.parametrize("clamp_pred", [-1, N])
@pytest.mark.parametrize("H,W", [(40, 56), (65, 33), (128, 130)])
def test_counters(H, W, clamp_pred):
    """Widths [1] and [3, 1, 3] on every map; the eight widths up to 34 on 128 x 130, the one map with a region
    wide enough (75 x 75) to leave ground truth outside a 34-pixel band.  Predictions run to N + 1: without the
    fold those pixels (and N itself stays valid) are skipped as the confusion kernel's n_invalid, with
    clamp_pred = N they fold to N."""
    P, G = confusion_case(H, W, H + W, N + 1)
    assert (P > N).any() and B.confusion(P, G, N, 255, clamp_pred)[1] >= 1
    for widths in ([1], [3, 1, 3]) + ((WIDTHS8,) if H >= 100 else ()):
        exp = check_counters(P, G, widths, clamp_pred)
        per = B.counters_per_width(N)
        if widths == [3, 1, 3]:
            assert np.array_equal(exp[:per], exp[2 * per:]) and not np.array_equal(exp[:per], exp[per:2 * per])


def test_counters_fold_below_the_classes():
    P, G = confusion_case(65, 33, 3, N - 1)
    exp = check_counters(P, G, [3, 1], 2)
    assert not np.array_equal(exp, B.counters(P, G, [3, 1], N, 255, -1))


def test_counters_without_lds():
    n = 40
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[:128, :130]
    G = (yy // 12 + 3 * (xx // 12)) % n
    G[:75, :75] = 1
    G[90:100, 90:110] = 255
    P = np.where(rng.random(G.shape) < 0.05, rng.integers(0, n, G.shape), np.roll(G, (2, 1), (0, 1)))
    P[P == 255] = 0
    check_counters(P, G, WIDTHS8, -1, n)


def test_counters_accumulate_over_images():
    exp = None
    got = torch.zeros(2 * B.counters_per_width(N), dtype=torch.int64, device="cuda")
    for H, W in ((40, 56), (65, 33)):
        P, G = confusion_case(H, W, H, N)
        exp = B.counters(P, G, [2, 4], N, 255, -1, out=exp)
        ops.boundary_confusion(dev(P), dev(G), [2, 4], got, num_classes=N)
    assert np.array_equal(got.cpu().numpy(), exp)
    with pytest.raises(ValueError):
        ops.boundary_confusion(dev(P), dev(G), [], got, num_classes=N)
    with pytest.raises(ValueError):
        ops.boundary_confusion(dev(P), dev(G), [0, 4], got, num_classes=N)
