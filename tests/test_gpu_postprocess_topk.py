"""catseg_postprocess_topk (sigmoid + bilinear resize + the K best classes, the class mass and the reject rule in
one kernel) on the device.

Where catseg_postprocess / catseg_resize_bilinear run banded (`_banded`, as tests/test_gpu_postprocess_argmax.py)
the fused kernel forms every class value with the same taps and the same fmas: its planes must EQUAL the stable
descending sort of their output, cut at K, and its mass the class-order fp32 running sum of it, bit for bit.  For
other widths it is checked against an fp64 reference."""
import functools

import pytest
import torch
import torch.nn.functional as F

from cat_seg import _lib as L
from cat_seg import custom_ops  # noqa: F401  (registers torch.ops.catseg.*)
from cat_seg import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def _banded(ch, cw, H, W):
    """launch_post's rule (misc.hip): 48 output rows per band, the band's source rows in <= 64 KB of LDS."""
    rows = 48 * ch // H + 3
    return W % 4 == 0 and rows * cw * 4 <= 64 * 1024


def _levels(shape, seed):
    # a few levels: exact ties between classes are everywhere, so the index order among equals is exercised
    return torch.randint(-2, 2, shape, generator=torch.Generator().manual_seed(seed)).float()


def _volume(lg, H, W, crop, sigmoid):
    """The existing kernel's (B, T, H, W) output on the host."""
    out = torch.empty(lg.shape[0], lg.shape[1], H, W, device="cuda")
    (ops.postprocess if sigmoid else ops.resize_bilinear)(lg.cuda(), out, crop=crop)
    return out.cpu()


def _reference(out):
    """(sorted values, sorted classes, mass) of a host volume: the stable descending sort over the classes (NaNs
    first, in class order; equal values in class order) and the class-order fp32 running sum from 0."""
    vals, idx = torch.sort(out, dim=1, descending=True, stable=True)
    acc = torch.zeros_like(out[:, 0])
    for t in range(out.shape[1]):
        acc = acc + out[:, t]
    return vals, idx.int(), acc


def _bits(t):
    return t.contiguous().view(torch.int32)


def _topk(lg, K, H, W, crop, sigmoid, **kw):
    return {k: v.cpu() for k, v in ops.postprocess_topk(lg.cuda().contiguous(), K, crop=crop, sigmoid=sigmoid,
                                                        out_hw=(H, W), **kw).items()}


# ---------------------------------------------------------------- bit-exact against the banded kernels
EXACT = {  # id: B, T, h, w, crop, H, W, Ks
    "crop-both-axes": (2, 7, 24, 24, (20, 23), 48, 68, (1, 2, 4)),
    "patch-256-tail": (1, 18, 16, 32, None, 60, 72, (1, 2, 4)),     # 16 classes per chunk, the second runs past T
    "npp8-odd-T": (1, 5, 40, 54, None, 20, 72, (1, 2, 4)),          # two classes per chunk
    "npp16": (1, 3, 60, 72, None, 20, 72, (1, 2)),                  # one class per chunk
    "patch-4096": (1, 2, 64, 64, None, 16, 64, (1, 2)),
    "tile-tails": (2, 5, 12, 12, None, 52, 100, (1, 2, 4)),
    "T-equals-K": (1, 4, 8, 8, None, 32, 32, (4,)),
    "T1": (3, 1, 8, 8, None, 32, 32, (1,)),
    "identity": (1, 33, 24, 24, None, 24, 24, (1, 2, 4)),
}
EXACT_CASES = [pytest.param(name, K, sigmoid, id=f"{name}-K{K}-{'sig' if sigmoid else 'plain'}")
               for name, spec in EXACT.items() for K in spec[-1] for sigmoid in (True, False)]


@functools.lru_cache(maxsize=None)
def _exact_reference(name, sigmoid):
    """One volume and one sort per shape, shared by every K (never modified)."""
    B, T, h, w, crop, H, W, _ = EXACT[name]
    lg = _levels((B, T, h, w), seed=T + H)
    return (lg,) + _reference(_volume(lg, H, W, crop, sigmoid))


@pytest.mark.parametrize("name,K,sigmoid", EXACT_CASES)
def test_equals_sort_of_postprocess(name, K, sigmoid):
    B, T, h, w, crop, H, W, _ = EXACT[name]
    ch, cw = crop or (h, w)
    assert _banded(ch, cw, H, W)            # the existing kernel runs banded here: exact equality is owed
    lg, vals, idx, mass = _exact_reference(name, sigmoid)
    got = _topk(lg, K, H, W, crop, sigmoid)
    assert got["topk_labels"].shape == (B, K, H, W) and got["topk_labels"].dtype == torch.int32
    assert torch.equal(got["topk_labels"], idx[:, :K])
    assert torch.equal(_bits(got["topk_score"]), _bits(vals[:, :K]))
    assert torch.equal(_bits(got["mass"]), _bits(mass))
    if T > 1:       # ties are everywhere: the rank-0 class is not always the first
        assert 0 < (idx[:, 0] > 0).float().mean() < 1


@pytest.mark.parametrize("sigmoid", [True, False])
@pytest.mark.parametrize("K", [1, 2, 4])
def test_plane0_equals_postprocess_argmax(K, sigmoid):
    lg = _levels((2, 7, 24, 24), seed=55).cuda()
    labels = torch.empty(2, 48, 68, dtype=torch.int32, device="cuda")
    score = torch.empty(2, 48, 68, device="cuda")
    ops.postprocess_argmax(lg, labels, score, crop=(20, 23), sigmoid=sigmoid)
    got = ops.postprocess_topk(lg, K, crop=(20, 23), sigmoid=sigmoid, out_hw=(48, 68))
    assert torch.equal(got["topk_labels"][:, 0], labels)
    assert torch.equal(_bits(got["topk_score"][:, 0]), _bits(score))


# ---------------------------------------------------------------- NaN / inf
def _check_nan(lg, H, W, sigmoid, two_nans, inf_then_nan):
    out = _volume(lg, H, W, None, sigmoid)
    vals, idx, _ = _reference(out)
    got = _topk(lg, 4, H, W, None, sigmoid)
    assert torch.equal(got["topk_labels"], idx[:, :4])
    assert torch.equal(got["topk_score"].isnan(), vals[:, :4].isnan())
    assert torch.allclose(got["topk_score"], vals[:, :4], rtol=0, atol=0, equal_nan=True)
    y, x = two_nans             # two NaNs at one pixel: ranks 0 and 1 in class order
    assert got["topk_labels"][0, :2, y, x].tolist() == [2, 5] and bool(got["topk_score"][0, :2, y, x].isnan().all())
    assert not bool(got["topk_score"][0, 2, y, x].isnan())
    if sigmoid:                 # +inf (sigmoid: 1) ranks behind the NaN of a later class; without the sigmoid the
        y, x = inf_then_nan     # interpolation itself turns +inf into a NaN (0 * -inf), in both kernels
        assert got["topk_labels"][0, :2, y, x].tolist() == [8, 7]
        assert bool(got["topk_score"][0, 0, y, x].isnan()) and float(got["topk_score"][0, 1, y, x]) == 1.0
    # the mass is NaN exactly where a NaN reaches the pixel
    reaches = out.isnan().any(1)
    assert torch.equal(got["mass"].isnan(), reaches) and 0 < int(reaches.sum()) < reaches.numel()


@pytest.mark.parametrize("sigmoid", [True, False])
def test_nan_ranks_first_in_class_order(sigmoid):
    """The planted pattern of test_gpu_postprocess_argmax.py::test_nan_ranks_highest_first_nan_wins (identity
    resize, the planted values reach the output as they are)."""
    lg = _levels((1, 9, 24, 24), seed=7)
    lg[0, 3, 0, :5] = float("nan")
    lg[0, 5, 1, :] = float("nan")
    lg[0, 2, 1, ::2] = float("nan")
    lg[0, 0, 2, :3] = float("nan")
    lg[0, 7, 3, 4] = float("inf")
    lg[0, 8, 3, 4] = float("nan")
    lg[0, 6, 5, 6] = float("inf")
    _check_nan(lg, 24, 24, sigmoid, two_nans=(1, 4), inf_then_nan=(3, 4))


@pytest.mark.parametrize("sigmoid", [True, False])
def test_nan_one_class_per_chunk(sigmoid):
    """Its twin at 60 x 72 -> 20 x 72, where a chunk holds one class: the values planted in source row 3 r + 1
    reach output row r as they are."""
    lg = _levels((1, 9, 60, 72), seed=7)
    lg[0, 3, 1, :5] = float("nan")
    lg[0, 5, 4, :] = float("nan")
    lg[0, 2, 4, ::2] = float("nan")
    lg[0, 0, 7, :3] = float("nan")
    lg[0, 7, 10, 4] = float("inf")
    lg[0, 8, 10, 4] = float("nan")
    lg[0, 6, 16, 6] = float("inf")
    assert _banded(60, 72, 20, 72)
    _check_nan(lg, 20, 72, sigmoid, two_nans=(1, 4), inf_then_nan=(3, 4))


# ---------------------------------------------------------------- widths the existing kernel does not band
FP64 = {  # id: T, h, w, crop, H, W, sigmoid, Ks
    "odd-width-cropped": (7, 24, 24, (20, 23), 50, 67, True, (2, 4)),
    "T150": (150, 96, 96, (96, 72), 127, 171, True, (2, 4)),
    "downsample": (19, 24, 24, None, 17, 19, True, (2, 4)),
    "no-sigmoid": (33, 40, 40, None, 30, 42, False, (2, 4)),
    "npp8": (5, 40, 54, None, 19, 70, True, (2, 4)),
    "npp8-no-sigmoid": (5, 40, 54, None, 19, 70, False, (2, 4)),
    "T847": (847, 24, 24, None, 61, 45, True, (2,)),
}


@functools.lru_cache(maxsize=None)
def _fp64_reference(name):
    T, h, w, crop, H, W, sigmoid, _ = FP64[name]
    g = torch.Generator().manual_seed(1000 + T)
    lg = 3 * torch.randn(1, T, h, w, generator=g) if sigmoid else torch.rand(1, T, h, w, generator=g)
    ch, cw = crop or (h, w)
    src = lg.double()[..., :ch, :cw]
    ref = F.interpolate(src.sigmoid() if sigmoid else src, size=(H, W), mode="bilinear", align_corners=False)[0]
    vals, idx = torch.sort(ref, dim=0, descending=True, stable=True)
    return lg, ref, vals[:5].clone(), idx[:5].clone(), ref.sum(0)


@pytest.mark.parametrize("name,K", [pytest.param(n, K, id=f"{n}-K{K}") for n, s in FP64.items() for K in s[-1]])
def test_against_fp64_reference(name, K):
    """fp64 on the host: sigmoid of the cropped logits, then F.interpolate(bilinear, align_corners=False).  A pixel
    is contested when any gap between consecutive fp64 ranks 0 .. K is below 1e-5 (the project's tolerance from
    test_gpu_postprocess_argmax.py::test_against_fp64_reference, about twice torch's fp32 distance from fp64).
    Uncontested pixels carry the fp64 top-K classes in order, contested ones classes whose fp64 value is within 1e-5
    of that rank's, every score is within 1e-5 of its rank's fp64 value, the mass within T 2^-23 mass + 1e-5 of the
    fp64 sum (the bound of a sequential fp32 sum), and at most 0.5 % of the pixels may be contested."""
    T, h, w, crop, H, W, sigmoid, _ = FP64[name]
    lg, ref, vals, idx, total = _fp64_reference(name)
    n_gaps = K if T > K else K - 1
    gaps = vals[:n_gaps] - vals[1:n_gaps + 1]
    contested = (gaps < 1e-5).any(0)
    got = _topk(lg, K, H, W, crop, sigmoid)
    lab, sc, mass = got["topk_labels"][0].long(), got["topk_score"][0].double(), got["mass"][0].double()
    assert int(lab.min()) >= 0 and int(lab.max()) < T
    picked = ref.gather(0, lab)
    share = contested.float().mean().item()
    print(f"{name} K={K}: contested {100 * share:.3f} %, max |score - fp64| {(sc - vals[:K]).abs().max().item():.2e}, "
          f"max |fp64 of the class - fp64 of the rank| {(picked - vals[:K]).abs().max().item():.2e}, "
          f"max |mass - fp64| {(mass - total).abs().max().item():.2e}")
    assert share <= 0.005
    assert torch.equal(lab[:, ~contested], idx[:K][:, ~contested])
    assert ((picked - vals[:K]).abs()[:, contested] <= 1e-5).all()
    assert (sc - vals[:K]).abs().max().item() <= 1e-5
    assert ((mass - total).abs() <= T * 2.0 ** -23 * mass + 1e-5).all()


# ---------------------------------------------------------------- the reject rule
@pytest.mark.parametrize("K", [1, 2, 4])
def test_reject_rule(K):
    g = torch.Generator().manual_seed(21)
    lg = 3 * torch.randn(2, 7, 24, 24, generator=g)
    plain = _topk(lg, K, 48, 68, (20, 23), True)
    s0 = plain["topk_score"][:, 0]
    # thresholds read off the kernel's own planes (a float32 survives the trip through a Python float): the median
    # score, and half the median lead over rank 1
    min_score = float(s0.median())
    min_margin = float((s0 - plain["topk_score"][:, 1]).median()) / 2 if K >= 2 else 0.25
    got = _topk(lg, K, 48, 68, (20, 23), True, reject=(min_score, min_margin, 7))
    for key in plain:           # with labels=None no other output changes
        assert torch.equal(_bits(got[key]), _bits(plain[key])), key
    rejected = s0 < torch.tensor(min_score, dtype=torch.float32)
    if K >= 2:
        rejected |= (s0 - got["topk_score"][:, 1]) < torch.tensor(min_margin, dtype=torch.float32)
    expect = torch.where(rejected, torch.full_like(got["topk_labels"][:, 0], 7), got["topk_labels"][:, 0])
    assert torch.equal(got["labels"], expect)
    assert 0.10 <= rejected.float().mean().item() <= 0.90


def test_nan_winner_is_kept():
    lg = _levels((1, 9, 24, 24), seed=7)
    lg[0, 5, 1, :] = float("nan")
    got = _topk(lg, 2, 24, 24, None, True, reject=(2.0, 2.0, 9))       # every number is rejected
    nan0 = got["topk_score"][0, 0].isnan()
    assert 0 < int(nan0.sum()) < nan0.numel()
    assert bool((got["labels"][0][nan0] == 5).all()) and bool((got["labels"][0][~nan0] == 9).all())


# ---------------------------------------------------------------- batch, untouched memory, the registered operator
def test_batch_invariance():
    g = torch.Generator().manual_seed(5)
    lg = 3 * torch.randn(3, 11, 24, 24, generator=g)
    all3 = _topk(lg, 4, 50, 67, (20, 23), True, reject=(0.9, 0.05, 11))
    for b in range(3):
        one = _topk(lg[b:b + 1], 4, 50, 67, (20, 23), True, reject=(0.9, 0.05, 11))
        for key in all3:
            assert torch.equal(_bits(all3[key][b]), _bits(one[key][0])), key


def test_outputs_not_passed_are_not_touched():
    """The entry itself, with mass and labels null: nothing but the two top-k tensors is written (guards round them
    stay, and so do a pre-filled mass and label map that are not passed)."""
    B, T, K, H, W = 2, 5, 2, 52, 100
    lg = _levels((B, T, 12, 12), seed=3).cuda()
    n = B * K * H * W
    pool_l = torch.full((n + 512,), -7, dtype=torch.int32, device="cuda")
    pool_s = torch.full((n + 512,), -7.0, device="cuda")
    mass = torch.full((B, H, W), -7.0, device="cuda")
    labels = torch.full((B, H, W), -7, dtype=torch.int32, device="cuda")
    tl, ts = pool_l[256:256 + n], pool_s[256:256 + n]
    L.call("catseg_postprocess_topk", lg.data_ptr(), B, T, 12, 12, 12, 12, 1, K, tl.data_ptr(), ts.data_ptr(), None, None,
           0.5, 0.5, 3, H, W, torch.cuda.current_stream().cuda_stream)
    ref = ops.postprocess_topk(lg, K, out_hw=(H, W), mass=False)
    assert set(ref) == {"topk_labels", "topk_score"}
    assert torch.equal(tl.view(B, K, H, W), ref["topk_labels"]) and torch.equal(ts.view(B, K, H, W), ref["topk_score"])
    for pool in (pool_l, pool_s):
        assert bool((pool[:256] == -7).all()) and bool((pool[256 + n:] == -7).all())
    assert bool((mass == -7.0).all()) and bool((labels == -7).all())


def test_opcheck_postprocess_topk():
    lg = _levels((2, 5, 24, 24), seed=11).cuda()
    torch.library.opcheck(torch.ops.catseg.postprocess_topk, (lg, 2, 48, 48, 24, 24, True))
    tl, ts, mass = torch.ops.catseg.postprocess_topk(lg, 2, 48, 48, 24, 24, True)
    vals, idx, acc = _reference(_volume(lg.cpu(), 48, 48, None, True))
    assert torch.equal(tl.cpu(), idx[:, :2]) and torch.equal(ts.cpu(), vals[:, :2]) and torch.equal(mass.cpu(), acc)
