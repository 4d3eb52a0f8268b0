"""catseg_postprocess_argmax (sigmoid + bilinear resize + argmax over the classes in one kernel) and
catseg_semseg_confusion_labels on the device.

Where catseg_postprocess / catseg_resize_bilinear run one of their banded kernels (post_sep_kernel or
post_band_kernel of misc.hip, which agree bit for bit), the fused kernel forms every class value with the same
taps and the same fmas, so its labels and scores must EQUAL the argmax / max of their output.  launch_post
takes a banded path when W % 4 == 0 and the band's source rows fit LDS (`_banded` restates its rule);
for other widths it falls back to a kernel with other arithmetic, and the fused kernel is checked against an
fp64 reference instead."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cat_seg import _lib as L
from cat_seg import custom_ops  # noqa: F401  (registers torch.ops.catseg.*)
from cat_seg import ops
from oracle import semseg_eval as OE

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def _banded(ch, cw, H, W):
    """launch_post's rule (misc.hip): 48 output rows per band, the band's source rows in <= 64 KB of LDS
    (with the horizontally interpolated rows for the separable kernel, alone for the direct one)."""
    rows = 48 * ch // H + 3
    return W % 4 == 0 and rows * cw * 4 <= 64 * 1024


def _existing(lg, H, W, crop, sigmoid):
    """The existing kernel's (B, T, H, W) output, argmax / max taken on the host (torch.argmax: first
    maximum, NaN above every number)."""
    out = torch.empty(lg.shape[0], lg.shape[1], H, W, device="cuda")
    (ops.postprocess if sigmoid else ops.resize_bilinear)(lg.cuda(), out, crop=crop)
    out = out.cpu()
    return out.argmax(1).int(), out.max(1).values


def _fused(lg, H, W, crop, sigmoid, with_score=True):
    B = lg.shape[0]
    labels = torch.full((B, H, W), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B, H, W), -7.0, device="cuda") if with_score else None
    ops.postprocess_argmax(lg.cuda().contiguous(), labels, score, crop=crop, sigmoid=sigmoid)
    return labels.cpu(), (score.cpu() if with_score else None)


def _levels(shape, seed):
    # a few levels: exact ties between classes are common, so the first-maximum rule is exercised
    return torch.randint(-2, 2, shape, generator=torch.Generator().manual_seed(seed)).float()


# ---------------------------------------------------------------- A / B: bit-exact against the banded kernels
EXACT = [  # B, T, h, w, crop, H, W
    pytest.param(2, 7, 24, 24, (20, 23), 48, 68, id="crop-both-axes"),
    pytest.param(1, 150, 96, 96, (96, 72), 128, 172, id="crop-T150"),
    pytest.param(3, 1, 8, 8, None, 32, 32, id="T1"),
    pytest.param(1, 33, 24, 24, None, 24, 24, id="identity"),
    pytest.param(1, 19, 40, 40, None, 28, 36, id="downsample"),
    pytest.param(2, 5, 12, 12, None, 52, 100, id="tile-tails"),
    # the source patch of a tile is 8 x 32 = 256 floats: the last size served by the 16-classes-per-chunk
    # kernel; 18 classes: a second chunk that runs past T
    pytest.param(1, 18, 16, 32, None, 60, 72, id="patch-256"),
    # larger patches: 8 passes of 256 elements (two classes per chunk, read as pairs), 16 passes (one class
    # per chunk, scalar reads), and the 64 x 64 = 4096-float patch that is the last to fit the LDS stage
    pytest.param(1, 5, 40, 54, None, 20, 72, id="npp8"),
    pytest.param(1, 3, 60, 72, None, 20, 72, id="npp16"),
    pytest.param(1, 2, 64, 64, None, 16, 64, id="patch-4096"),
]


@pytest.mark.parametrize("B,T,h,w,crop,H,W", EXACT)
def test_equals_argmax_of_postprocess(B, T, h, w, crop, H, W):
    ch, cw = crop or (h, w)
    assert _banded(ch, cw, H, W)            # the existing kernel runs banded here: exact equality is owed
    lg = _levels((B, T, h, w), seed=T + H)
    ref_l, ref_s = _existing(lg, H, W, crop, True)
    lab, sc = _fused(lg, H, W, crop, True)
    assert torch.equal(lab, ref_l)
    assert torch.equal(sc, ref_s)
    if T > 1:
        assert 0 < (ref_l > 0).float().mean() < 1


@pytest.mark.parametrize("T,h,w,H,W", [
    pytest.param(33, 40, 40, 30, 44, id="30-44"),
    pytest.param(33, 40, 40, 40, 40, id="40-40"),
    pytest.param(5, 40, 54, 20, 72, id="npp8"),
    pytest.param(3, 60, 72, 20, 72, id="npp16"),
    pytest.param(2, 64, 64, 16, 64, id="patch-4096"),
])
def test_equals_argmax_of_resize_bilinear(T, h, w, H, W):
    assert _banded(h, w, H, W)
    lg = _levels((1, T, h, w), seed=H)
    ref_l, ref_s = _existing(lg, H, W, None, False)
    lab, sc = _fused(lg, H, W, None, False)
    assert torch.equal(lab, ref_l)
    assert torch.equal(sc, ref_s)


# ---------------------------------------------------------------- C: NaN / inf
@pytest.mark.parametrize("sigmoid", [True, False])
def test_nan_ranks_highest_first_nan_wins(sigmoid):
    """Identity resize, so the planted values reach the output as they are (sigmoid(NaN) = NaN,
    sigmoid(+inf) = 1); planted as tests/test_gpu_eval.py::test_confusion_kernel_nan_ranks_highest does."""
    lg = _levels((1, 9, 24, 24), seed=7)
    lg[0, 3, 0, :5] = float("nan")         # NaN at a class index > 0
    lg[0, 5, 1, :] = float("nan")
    lg[0, 2, 1, ::2] = float("nan")        # two NaNs at one pixel: the first (class 2) wins
    lg[0, 0, 2, :3] = float("nan")         # NaN at class 0
    lg[0, 7, 3, 4] = float("inf")
    lg[0, 8, 3, 4] = float("nan")          # NaN after +inf at one pixel
    lg[0, 6, 5, 6] = float("inf")          # +inf alone
    ref_l, ref_s = _existing(lg, 24, 24, None, sigmoid)
    lab, sc = _fused(lg, 24, 24, None, sigmoid)
    # (a NaN also reaches the pixels whose second tap it is, as 0 * NaN, in both kernels)
    assert int(ref_l[0, 2, 0]) == 0 and int(ref_l[0, 0, 23]) == 5
    assert torch.equal(lab, ref_l)
    assert torch.equal(sc.isnan(), ref_s.isnan()) and int(sc.isnan().sum()) >= 5 + 24 + 3 + 1
    assert torch.allclose(sc, ref_s, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize("sigmoid", [True, False])
def test_nan_one_class_per_chunk(sigmoid):
    """The same planted values at 60 x 72 -> 20 x 72, where a chunk holds one class: output row y reads
    source row 3 y + 1 with weight 1 (and row 3 y + 2 with weight 0), output column x reads column x, so
    the values planted in source row 3 r + 1 reach output row r as they are."""
    lg = _levels((1, 9, 60, 72), seed=7)
    lg[0, 3, 1, :5] = float("nan")         # NaN at a class index > 0
    lg[0, 5, 4, :] = float("nan")
    lg[0, 2, 4, ::2] = float("nan")        # two NaNs at one pixel: the first (class 2) wins
    lg[0, 0, 7, :3] = float("nan")         # NaN at class 0
    lg[0, 7, 10, 4] = float("inf")
    lg[0, 8, 10, 4] = float("nan")         # NaN after +inf at one pixel
    lg[0, 6, 16, 6] = float("inf")         # +inf alone
    assert _banded(60, 72, 20, 72)
    ref_l, ref_s = _existing(lg, 20, 72, None, sigmoid)
    lab, sc = _fused(lg, 20, 72, None, sigmoid)
    assert int(ref_l[0, 2, 0]) == 0 and int(ref_l[0, 1, 0]) == 2 and int(ref_l[0, 1, 71]) == 5
    assert torch.equal(lab, ref_l)
    assert torch.equal(sc.isnan(), ref_s.isnan()) and int(sc.isnan().sum()) >= 5 + 72 + 3 + 1
    assert torch.allclose(sc, ref_s, rtol=0, atol=0, equal_nan=True)


# ---------------------------------------------------------------- D: widths the existing kernel does not band
FP64 = [  # T, h, w, crop, H, W, sigmoid
    pytest.param(7, 24, 24, (20, 23), 50, 67, True, id="odd-width-cropped"),
    pytest.param(150, 96, 96, (96, 72), 127, 171, True, id="T150"),
    pytest.param(19, 24, 24, None, 17, 19, True, id="downsample"),
    pytest.param(33, 40, 40, None, 30, 42, False, id="no-sigmoid"),
    pytest.param(847, 24, 24, None, 61, 45, True, id="T847"),
    # two classes per chunk (8 passes over the patch) and one (16 passes), at an odd width
    pytest.param(5, 40, 54, None, 19, 70, True, id="npp8"),
    pytest.param(5, 40, 54, None, 19, 70, False, id="npp8-no-sigmoid"),
    pytest.param(3, 60, 72, None, 19, 70, True, id="npp16"),
    pytest.param(3, 60, 72, None, 19, 70, False, id="npp16-no-sigmoid"),
]


@pytest.mark.parametrize("T,h,w,crop,H,W,sigmoid", FP64)
def test_against_fp64_reference(T, h, w, crop, H, W, sigmoid):
    """fp64 on the host: sigmoid of the cropped logits, then F.interpolate(bilinear, align_corners=False).
    A pixel is contested when its fp64 top-two gap is below 1e-5 (torch's own fp32 path is within 5.3e-6 of
    fp64 on these inputs, so 1e-5 is about twice that).  Uncontested pixels must carry the fp64 argmax,
    contested ones a label whose fp64 probability is within 1e-5 of the maximum, every score is within
    1e-5 of the fp64 maximum, and at most 0.5 % of the pixels may be contested."""
    g = torch.Generator().manual_seed(1000 + T)
    lg = 3 * torch.randn(1, T, h, w, generator=g) if sigmoid else torch.rand(1, T, h, w, generator=g)
    ch, cw = crop or (h, w)
    src = lg.double()[..., :ch, :cw]
    ref = F.interpolate(src.sigmoid() if sigmoid else src, size=(H, W), mode="bilinear", align_corners=False)[0]
    top2 = ref.topk(2, dim=0).values
    contested = (top2[0] - top2[1]) < 1e-5
    lab, sc = _fused(lg, H, W, crop, sigmoid)
    lab, sc = lab[0].long(), sc[0].double()
    assert int(lab.min()) >= 0 and int(lab.max()) < T
    picked = ref.gather(0, lab[None])[0]
    share = contested.float().mean().item()
    print(f"T={T} {H}x{W}: contested {100 * share:.3f} %, max |score - fp64| {(sc - top2[0]).abs().max().item():.2e}, "
          f"max fp64 shortfall of the label {(top2[0] - picked).max().item():.2e}")
    assert share <= 0.005
    assert torch.equal(lab[~contested], ref.argmax(0)[~contested])
    assert ((top2[0] - picked)[contested] <= 1e-5).all()
    assert (sc - top2[0]).abs().max().item() <= 1e-5


# ---------------------------------------------------------------- E / F
def test_score_none_writes_only_labels():
    lg = _levels((2, 5, 12, 12), seed=3).cuda()
    labels = torch.empty(2, 52, 100, dtype=torch.int32, device="cuda")
    both = torch.empty_like(labels)
    score = torch.full((2, 52, 100), -7.0, device="cuda")      # allocated, pre-filled, NOT passed
    ops.postprocess_argmax(lg, labels, None)
    ops.postprocess_argmax(lg, both, torch.empty(2, 52, 100, device="cuda"))
    assert torch.equal(labels, both)
    assert bool((score == -7.0).all())


def test_batch_invariance():
    g = torch.Generator().manual_seed(5)
    lg = 3 * torch.randn(3, 11, 24, 24, generator=g)
    lab3, sc3 = _fused(lg, 50, 67, (20, 23), True)
    for b in range(3):
        lab1, sc1 = _fused(lg[b:b + 1], 50, 67, (20, 23), True)
        assert torch.equal(lab3[b], lab1[0]) and torch.equal(sc3[b], sc1[0])


# ---------------------------------------------------------------- G: confusion from labels
def _case(T, H, W, seed, n_levels=4):
    g = torch.Generator().manual_seed(seed)
    probs = torch.randint(0, n_levels, (T, H, W), generator=g).float() / n_levels
    gt = torch.randint(0, T, (H, W), generator=g).int()
    gt[torch.rand(H, W, generator=g) < 0.1] = 255
    return probs, gt


@pytest.mark.parametrize("T,H,W,clamp", [(150, 97, 131, -1), (21, 48, 64, 20), (1, 5, 7, -1)])
def test_confusion_labels_equals_confusion_and_oracle(T, H, W, clamp):
    probs, gt = _case(T, H, W, seed=T + H)
    labels = probs.argmax(0).int()
    N = T
    n1 = N + 1
    conf = torch.zeros(n1 * n1, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    conf_p, bad_p = torch.zeros_like(conf), torch.zeros_like(bad)
    ref = np.zeros((n1, n1), np.int64)
    for _ in range(2):       # accumulates across calls
        ops.semseg_confusion_labels(labels.cuda(), gt.cuda(), conf, bad, num_classes=N, ignore_label=255,
                                    clamp_pred=clamp)
        ops.semseg_confusion(probs.cuda(), gt.cuda(), conf_p, bad_p, num_classes=N, ignore_label=255, clamp_pred=clamp)
        OE.confusion_update(ref, probs.numpy(), gt.numpy(), N, 255, clamp_pred=clamp)
    assert int(bad.item()) == 0 and int(bad_p.item()) == 0
    assert torch.equal(conf, conf_p)
    assert np.array_equal(conf.cpu().numpy().reshape(n1, n1), ref)
    assert int(conf.sum().item()) == 2 * H * W


def test_confusion_labels_counts_invalid():
    probs, gt = _case(5, 8, 8, seed=3)
    labels = probs.argmax(0).int()
    gt[0, 0] = 7          # not a class, not ignore
    gt[1, 1] = -2
    labels[2, 2] = 6      # beyond num_classes
    labels[3, 3] = -1
    conf = torch.zeros(36, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    ops.semseg_confusion_labels(labels.cuda(), gt.cuda(), conf, bad, num_classes=5, ignore_label=255)
    assert int(bad.item()) == 4 and int(conf.sum().item()) == 60
    # with the VOC-b fold a label beyond the classes folds to clamp_pred first, as the probability form's argmax does
    conf.zero_(), bad.zero_()
    ops.semseg_confusion_labels(labels.cuda(), gt.cuda(), conf, bad, num_classes=5, ignore_label=255, clamp_pred=4)
    assert int(bad.item()) == 3 and int(conf.sum().item()) == 61


# ---------------------------------------------------------------- H
def test_opcheck_postprocess_argmax():
    lg = _levels((2, 5, 24, 24), seed=11).cuda()
    torch.library.opcheck(torch.ops.catseg.postprocess_argmax, (lg, 48, 48, 24, 24, True))
    lab, sc = torch.ops.catseg.postprocess_argmax(lg, 48, 48, 24, 24, True)
    ref_l, ref_s = _existing(lg.cpu(), 48, 48, None, True)
    assert torch.equal(lab.cpu(), ref_l) and torch.equal(sc.cpu(), ref_s)
