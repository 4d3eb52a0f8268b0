"""catseg_postprocess_tta on the device: the merge of K test-time-augmentation views (sigmoid + bilinear
resize per view, mirrored views flipped back, fp32 sum in view order, scale by the fp32 reciprocal of K)
as probabilities and as the label map of their argmax.

Where catseg_postprocess runs banded for every view (W % 4 == 0 and the band rule `_banded` restates) the
kernel forms every view's value with the same taps and fmas, so its output must EQUAL the composition of
the existing kernels; at other widths it is checked against an fp64 reference.  For every shape the label
form must equal the argmax / max of the kernel's own probability form."""
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
    # a few levels: exact ties between classes are common, so the first-maximum rule is exercised
    return torch.randint(-2, 2, shape, generator=torch.Generator().manual_seed(seed)).float()


def _views(K, h, w, crops, flips):
    crops = crops if crops is not None else [(h, w)] * K
    flips = flips if flips is not None else [k % 2 for k in range(K)]
    assert len(crops) == K and len(flips) == K
    return [(c[0], c[1], f) for c, f in zip(crops, flips)]


def _composition(lg, views, H, W):
    """What the parent's wrapper computes from the existing kernel: per view ops.postprocess with its crop,
    .flip(-1) if mirrored, sequential fp32 adds in view order, then a MULTIPLY by fp32 1 / K."""
    lg = lg.cuda()
    acc = None
    for k, (ch, cw, fl) in enumerate(views):
        out = torch.empty(1, lg.shape[1], H, W, device="cuda")
        ops.postprocess(lg[k:k + 1].contiguous(), out, crop=(ch, cw))
        p = out[0].flip(-1) if fl else out[0]
        acc = p if acc is None else acc + p
    rk = torch.tensor(1.0, dtype=torch.float32) / len(views)
    return (acc * rk.cuda()).cpu()


def _fused(lg, views, H, W, *, probs=True, labels=True, score=True):
    T = lg.shape[1]
    p = torch.full((T, H, W), -7.0, device="cuda") if probs else None
    lab = torch.full((H, W), -7, dtype=torch.int32, device="cuda") if labels else None
    sc = torch.full((H, W), -7.0, device="cuda") if score else None
    ops.postprocess_tta(lg.cuda().contiguous(), views, probs=p, labels=lab, score=sc)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (p, lab, sc))


# ---------------------------------------------------------------- bit-exact against the existing kernels
EXACT = [  # K, T, h, w, crops, flips, H, W
    pytest.param(1, 7, 24, 24, [(20, 23)], [0], 48, 68, id="single-view"),
    pytest.param(1, 7, 24, 24, [(20, 23)], [1], 48, 68, id="single-view-flipped"),
    pytest.param(4, 18, 16, 32, [(16, 32), (12, 32), (16, 20), (9, 17)], [0, 1, 0, 1], 60, 72, id="patch-256"),
    pytest.param(3, 5, 12, 12, None, [1, 0, 1], 52, 100, id="flipped-tile-tails"),
    pytest.param(2, 19, 40, 40, None, [1, 0], 28, 36, id="downsample"),
    pytest.param(18, 150, 96, 96, [(96, 96)] * 16 + [(96, 72), (80, 96)], None, 128, 172, id="K18-T150"),
    pytest.param(32, 3, 8, 8, None, None, 32, 32, id="K32"),
    # larger patches: 8 passes of 256 elements (two classes per chunk, read as pairs), 16 passes (one class
    # per chunk, scalar reads), and the 64 x 64 = 4096-float patch that is the last to fit the LDS stage
    pytest.param(3, 5, 40, 54, [(40, 54), (33, 54), (40, 41)], [1, 0, 1], 20, 72, id="npp8"),
    pytest.param(2, 3, 60, 72, None, [0, 1], 20, 72, id="npp16"),
    pytest.param(1, 2, 64, 64, [(64, 64)], [0], 16, 64, id="patch-4096"),
]


@pytest.mark.parametrize("K,T,h,w,crops,flips,H,W", EXACT)
def test_equals_the_composition_of_existing_kernels(K, T, h, w, crops, flips, H, W):
    views = _views(K, h, w, crops, flips)
    assert all(_banded(ch, cw, H, W) for ch, cw, _ in views)     # exact equality is owed
    lg = _levels((K, T, h, w), seed=T + H + K)
    ref = _composition(lg, views, H, W)
    p, lab, sc = _fused(lg, views, H, W)
    assert torch.equal(p, ref)
    assert torch.equal(lab, ref.argmax(0).int())
    assert torch.equal(sc, ref.max(0).values)
    assert 0 < (lab > 0).float().mean() < 1
    if K == 1 and flips == [0]:
        # one unflipped view is the existing single-view kernels, exactly
        out = torch.empty(1, T, H, W, device="cuda")
        ops.postprocess(lg.cuda(), out, crop=crops[0])
        assert torch.equal(p, out[0].cpu())
        l1 = torch.empty(1, H, W, dtype=torch.int32, device="cuda")
        s1 = torch.empty(1, H, W, device="cuda")
        ops.postprocess_argmax(lg.cuda(), l1, s1, crop=crops[0])
        assert torch.equal(lab, l1[0].cpu()) and torch.equal(sc, s1[0].cpu())


# ---------------------------------------------------------------- fp64 reference at widths that do not band
FP64 = [  # K, T, h, w, crops, flips, H, W
    pytest.param(4, 150, 96, 96, [(96, 72), (96, 96), (80, 96), (64, 48)], [0, 1, 0, 1], 127, 171, id="T150"),
    pytest.param(3, 7, 24, 24, [(20, 23), (24, 24), (12, 17)], [1, 0, 1], 50, 67, id="odd-width-cropped"),
    pytest.param(6, 847, 24, 24, [(24, 24), (20, 23)] * 3, None, 61, 45, id="T847"),
    pytest.param(5, 19, 40, 40, None, None, 17, 19, id="downsample"),
    pytest.param(3, 5, 40, 54, None, [1, 0, 1], 19, 70, id="npp8"),
    pytest.param(3, 3, 60, 72, None, [0, 1, 1], 19, 70, id="npp16"),
]


def _fp64_inputs(K, T, h, w, crops, flips):
    lg = 3 * torch.randn(K, T, h, w, generator=torch.Generator().manual_seed(2000 + T + K))
    return lg, _views(K, h, w, crops, flips)


@pytest.mark.parametrize("K,T,h,w,crops,flips,H,W", FP64)
def test_label_form_equals_probability_form(K, T, h, w, crops, flips, H, W):
    lg, views = _fp64_inputs(K, T, h, w, crops, flips)
    p, _, _ = _fused(lg, views, H, W, labels=False, score=False)
    _, lab, sc = _fused(lg, views, H, W, probs=False)
    assert torch.equal(lab, p.argmax(0).int())
    assert torch.equal(sc, p.max(0).values)


@pytest.mark.parametrize("K,T,h,w,crops,flips,H,W", FP64)
def test_against_fp64_reference(K, T, h, w, crops, flips, H, W):
    """fp64 on the host: per view the sigmoid of the cropped logits, F.interpolate(bilinear,
    align_corners=False), the flip back, the mean.  The rule of
    test_gpu_postprocess_argmax.py::test_against_fp64_reference, unchanged: a pixel is contested when its
    fp64 top-two gap is below 1e-5; uncontested pixels carry the fp64 argmax, contested ones a label within
    1e-5 of the maximum; scores and probabilities are within 1e-5; at most 0.5 % of the pixels are contested."""
    lg, views = _fp64_inputs(K, T, h, w, crops, flips)
    ref = 0
    for k, (ch, cw, fl) in enumerate(views):
        r = F.interpolate(lg[k:k + 1].double()[..., :ch, :cw].sigmoid(), size=(H, W), mode="bilinear",
                          align_corners=False)[0]
        ref = ref + (r.flip(-1) if fl else r)
    ref = ref / K
    top2 = ref.topk(2, dim=0).values
    contested = (top2[0] - top2[1]) < 1e-5
    p, lab, sc = _fused(lg, views, H, W)
    lab, sc = lab.long(), sc.double()
    assert int(lab.min()) >= 0 and int(lab.max()) < T
    picked = ref.gather(0, lab[None])[0]
    share = contested.float().mean().item()
    print(f"K={K} T={T} {H}x{W}: contested {100 * share:.3f} %, max |probs - fp64| "
          f"{(p.double() - ref).abs().max().item():.2e}, max |score - fp64| {(sc - top2[0]).abs().max().item():.2e}, "
          f"max fp64 shortfall of the label {(top2[0] - picked).max().item():.2e}")
    assert share <= 0.005
    assert torch.equal(lab[~contested], ref.argmax(0)[~contested])
    assert ((top2[0] - picked)[contested] <= 1e-5).all()
    assert (sc - top2[0]).abs().max().item() <= 1e-5
    assert (p.double() - ref).abs().max().item() <= 1e-5


# ---------------------------------------------------------------- NaN / inf
def test_nan_ranks_highest_first_nan_wins():
    """Identity resize, K = 2: NaN planted in one view, +inf in the other (sigmoid(NaN) = NaN,
    sigmoid(+inf) = 1; NaN + x = NaN)."""
    lg = _levels((2, 9, 24, 24), seed=7)
    lg[0, 3, 0, :5] = float("nan")         # NaN at a class index > 0
    lg[0, 5, 1, :] = float("nan")
    lg[0, 2, 1, ::2] = float("nan")        # two NaNs at one pixel: the first (class 2) wins
    lg[1, 7, 3, 4] = float("inf")
    lg[1, 6, 5, 6] = float("inf")
    lg[1, 1, 0, 2] = float("inf")          # +inf in the other view at a pixel with a NaN
    views = [(24, 24, 0), (24, 24, 0)]
    ref = _composition(lg, views, 24, 24)
    p, lab, sc = _fused(lg, views, 24, 24)
    # (a NaN also reaches the pixels whose second tap it is, as 0 * NaN, in both kernels)
    assert int(ref.argmax(0)[1, 0]) == 2 and int(ref.argmax(0)[1, 23]) == 5
    assert torch.equal(lab, ref.argmax(0).int())
    assert torch.equal(p.isnan(), ref.isnan()) and int(p.isnan().sum()) >= 5 + 24 + 12
    assert torch.equal(sc.isnan(), ref.max(0).values.isnan())
    assert torch.allclose(p, ref, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(sc, ref.max(0).values, rtol=0, atol=0, equal_nan=True)


# ---------------------------------------------------------------- outputs not passed are not written
def test_outputs_not_passed_are_not_written():
    lg = _levels((2, 5, 12, 12), seed=3).cuda()
    views = [(12, 12, 0), (10, 12, 1)]
    vol = torch.full((5, 20, 24), -7.0, device="cuda")
    score = torch.full((20, 24), -7.0, device="cuda")
    labels = torch.full((20, 24), -7, dtype=torch.int32, device="cuda")
    ops.postprocess_tta(lg, views, labels=labels)
    torch.cuda.synchronize()
    assert int(labels.min()) >= 0
    assert bool((vol == -7).all()) and bool((score == -7).all())
    ops.postprocess_tta(lg, views, probs=vol)
    torch.cuda.synchronize()
    assert bool((vol >= 0).all()) and bool((score == -7).all())


# ---------------------------------------------------------------- operators
def test_operators_opcheck():
    lg = _levels((2, 5, 24, 24), seed=11).cuda()
    args = (lg, 48, 48, [24, 20], [24, 23], [0, 1])
    torch.library.opcheck(torch.ops.catseg.postprocess_tta.default, args)
    torch.library.opcheck(torch.ops.catseg.postprocess_tta_argmax.default, args)
    p = torch.ops.catseg.postprocess_tta(*args)
    lab, sc = torch.ops.catseg.postprocess_tta_argmax(*args)
    assert torch.equal(lab, p.argmax(0).int()) and torch.equal(sc, p.max(0).values)
