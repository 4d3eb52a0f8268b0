"""The four entry points of csrc/train_topk.hip (training with more classes than pad_len, model.py:691-725)
with poisoned padding, as tests/test_gpu_train_poison.py: every operand and output is a view of a larger
NaN (int: sentinel) buffer, every byte outside the defined output must be untouched, and every result is
compared BIT FOR BIT with its definition formed on the host -- these kernels move values or add them in a
fixed order, so there is no tolerance anywhere in this file except the loss case's, which is the existing
gate of tests/test_gpu_training_loss.py.

  class_inverse          vs a host loop
  class_rows_reduce      vs the same fp32 sum in ascending image order (scalar path: cols 7 / ld 9; vector
                         path: cols 256), beta 0 and 1, a class picked by every image, by exactly one, by none
  class_planes_scatter   vs torch.full(-100.).scatter_, class_planes_gather vs torch.gather, and
                         gather(scatter(x)) == x: P = 15 (no 16-byte path) and 96*96, dense / strided /
                         misaligned-base views
  bce_onehot_loss        the existing loss kernels on a scattered volume (-100 planes, ground truth in
                         unselected classes), which they had never seen

Marked gpu: runs on the MI355X box only."""
import pytest
import torch

import poison as P
from cat_seg import _lib as L
from cat_seg import ops
from cat_seg import train_ops as TO
from test_gpu_training_loss import reference_grad, reference_loss

pytestmark = pytest.mark.gpu

dev = "cuda"
F32, I32 = torch.float32, torch.int32
SLACK = 64


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def selection(B, T0, k, seed):
    """classes (B, k) int32: k distinct classes per image in random order, and the host-loop inverse."""
    gen = torch.Generator().manual_seed(seed)
    classes = torch.stack([torch.randperm(T0, generator=gen)[:k] for _ in range(B)]).to(I32)
    return classes, host_inverse(classes, T0)


def host_inverse(classes, T0):
    B, k = classes.shape
    inv = torch.full((B, T0), -1, dtype=I32)
    for b in range(B):
        for j in range(k):
            inv[b, int(classes[b, j])] = j
    return inv


def idx_dev(t):
    """An int32 index tensor on the device with sentinel slack behind it."""
    return P.flat_padded(t, SLACK, device=dev)[1]


def planes(B, n, Pn, mode, data=None):
    """(buf, view, mask): a [B][n][Pn] fp32 view of a 1-D NaN buffer and the mask of the elements it names.
    dense: contiguous, no slack.  strided: plane stride Pn + 8, 12 floats between images, 64 behind (every
    16-byte condition of the dense call still holds).  misaligned: the strided view one float further on
    (no 16-byte access is possible)."""
    ts = Pn if mode == "dense" else Pn + 8
    bs = n * ts if mode == "dense" else n * ts + 12
    off = 1 if mode == "misaligned" else 0
    size = off + (B - 1) * bs + (n - 1) * ts + Pn + (0 if mode == "dense" else SLACK)
    buf = P.filled((size,), F32, dev)
    view = buf.as_strided((B, n, Pn), (bs, ts, 1), off)
    mask = torch.zeros(size, dtype=torch.bool, device=dev)
    mask.as_strided((B, n, Pn), (bs, ts, 1), off).fill_(True)
    if data is not None:
        view.copy_(data)
    return buf, view, mask


def check_outside(buf, mask, what):
    assert bool(torch.isnan(buf[~mask]).all()), f"{what}: an element outside the output was written"


# ============================================================================= catseg_class_inverse
@pytest.mark.parametrize("B,T0,k", [(3, 13, 5), (1, 2048, 256)])
def test_class_inverse(B, T0, k):
    classes, ref = selection(B, T0, k, seed=T0)
    buf, out = P.flat_out_buffer((B, T0), SLACK, I32, dev)
    TO.class_inverse(idx_dev(classes), T0, out=out)
    torch.cuda.synchronize()
    P.check_untouched_flat(buf, B * T0, "class_inverse")
    assert torch.equal(out.cpu(), ref)
    assert int((out >= 0).sum()) == B * k


def test_class_inverse_skips_out_of_range_ids():
    """A class id outside [0, T0) is a caller bug: it is skipped, nothing is written out of bounds."""
    B, T0, k = 2, 13, 5
    classes, ref = selection(B, T0, k, seed=3)
    bad = classes.clone()
    bad[0, 1], bad[1, 4] = T0, -7
    ref[0, classes[0, 1]] = ref[1, classes[1, 4]] = -1
    buf, out = P.flat_out_buffer((B, T0), SLACK, I32, dev)
    TO.class_inverse(idx_dev(bad), T0, out=out)
    torch.cuda.synchronize()
    P.check_untouched_flat(buf, B * T0, "class_inverse")
    assert torch.equal(out.cpu(), ref)


# ============================================================================= catseg_class_rows_reduce
# class 0 picked by every image, class 1 by image 1 alone, classes 8..12 by none; positions differ per image
ROWS_CLASSES = torch.tensor([[0, 2, 3, 4, 5], [6, 1, 0, 2, 7], [3, 4, 7, 6, 0]], dtype=I32)


@pytest.mark.parametrize("beta", [0, 1])
@pytest.mark.parametrize("cols,pad", [(7, 2), (256, 8)])
def test_class_rows_reduce(cols, pad, beta):
    B, T0, k = 3, 13, 5
    inv = host_inverse(ROWS_CLASSES, T0)
    picked = (inv >= 0).sum(0)
    assert picked[0] == B and picked[1] == 1 and (picked[8:] == 0).all()
    gen = torch.Generator().manual_seed(cols + beta)
    d = torch.randn(B * k, cols, generator=gen)
    init = torch.randn(T0, cols, generator=gen)
    # the definition: the fp32 sum over the images in ascending order, then (beta) added to what was there
    acc = torch.zeros(T0, cols)
    for b in range(B):
        for t in range(T0):
            if inv[b, t] >= 0:
                acc[t] = acc[t] + d[b * k + int(inv[b, t])]
    ref = init + acc if beta else acc
    ref[picked == 0] = init[picked == 0] if beta else 0.0

    dbuf, dview = P.padded(d, 3, pad, device=dev)
    obuf, oview = P.out_buffer(T0, cols, 5, pad, F32, dev)
    if beta:
        oview.copy_(init)
    assert dview.stride(0) == cols + pad
    TO.class_rows_reduce(dview, idx_dev(inv), oview, k=k, beta=beta)
    torch.cuda.synchronize()
    P.check_untouched(obuf, T0, cols, "class_rows_reduce")
    P.check_no_nan(oview, "class_rows_reduce")
    P.check_bit_identical(oview.cpu().contiguous(), ref, "class_rows_reduce vs the host sum")
    if not beta:
        assert not oview[8:].cpu().abs().max().item()


# ============================================================================= planes scatter / gather
@pytest.mark.parametrize("mode", ["dense", "strided", "misaligned"])
@pytest.mark.parametrize("Pn", [15, 96 * 96])
def test_class_planes_scatter_and_gather(Pn, mode):
    B, T0, k = 2, 13, 5
    classes, inv = selection(B, T0, k, seed=Pn % 97)
    gen = torch.Generator().manual_seed(Pn)
    x = torch.randn(B, k, Pn, generator=gen)
    idx = classes.long()[..., None].expand(-1, -1, Pn)
    full_ref = torch.full((B, T0, Pn), -100.0).scatter_(1, idx, x)

    # scatter: x (B, k, P) -> (B, T0, P), -100 where no class was selected
    _, xv, _ = planes(B, k, Pn, mode, x)
    fbuf, fv, fmask = planes(B, T0, Pn, mode)
    TO.class_planes_scatter(xv, idx_dev(inv), fv, -100.0)
    torch.cuda.synchronize()
    check_outside(fbuf, fmask, "class_planes_scatter")
    P.check_bit_identical(fv.cpu().contiguous(), full_ref, "class_planes_scatter vs full().scatter_")

    # gather of an independent volume: vs torch.gather
    y = torch.randn(B, T0, Pn, generator=gen)
    _, yv, _ = planes(B, T0, Pn, mode, y)
    gbuf, gv, gmask = planes(B, k, Pn, mode)
    TO.class_planes_gather(yv, idx_dev(classes), gv)
    torch.cuda.synchronize()
    check_outside(gbuf, gmask, "class_planes_gather")
    P.check_bit_identical(gv.cpu().contiguous(), torch.gather(y, 1, idx), "class_planes_gather vs torch.gather")

    # gather(scatter(x)) == x
    rbuf, rv, rmask = planes(B, k, Pn, mode)
    TO.class_planes_gather(fv, idx_dev(classes), rv)
    torch.cuda.synchronize()
    check_outside(rbuf, rmask, "class_planes_gather(scatter)")
    P.check_bit_identical(rv.cpu().contiguous(), x, "gather(scatter(x)) vs x")


def test_class_planes_4d_views_through_the_wrappers():
    """The wrappers take (B, n, h, w) maps (the head's logits) and derive the plane strides."""
    B, T0, k, h = 2, 13, 5, 6
    classes, inv = selection(B, T0, k, seed=1)
    x = torch.randn(B, k, h, h, generator=torch.Generator().manual_seed(2))
    out = TO.class_planes_scatter(x.to(dev), inv.to(dev), torch.empty(B, T0, h, h, device=dev), -100.0)
    idx = classes.long()[..., None, None].expand(-1, -1, h, h)
    assert torch.equal(out.cpu(), torch.full((B, T0, h, h), -100.0).scatter_(1, idx, x))
    back = TO.class_planes_gather(out, classes.to(dev), torch.empty(B, k, h, h, device=dev))
    assert torch.equal(back.cpu(), x)


# ============================================================================= the loss on -100 planes
def test_bce_onehot_loss_on_a_scattered_volume():
    """catseg_bce_onehot_loss / _backward on what the top-k branch hands them: -100 in every unselected
    plane (softplus(-100) per element, softplus(100) where the ground-truth class was not selected), gates of
    tests/test_gpu_training_loss.py (loss 1e-5 * |ref| + 1e-6, gradient 2e-5 * max |ref|)."""
    B, T0, k, h, H = 2, 13, 5, 24, 96
    classes, inv = selection(B, T0, k, seed=8)
    gen = torch.Generator().manual_seed(8)
    sel = torch.randn(B, k, h, h, generator=gen) * 3
    targets = torch.randint(0, T0, (B, H, H), generator=gen, dtype=I32)
    targets[:, :3] = 255
    for b in range(B):       # ground truth in selected and in unselected classes
        gt = set(targets[b].unique().tolist()) - {255}
        chosen = set(classes[b].tolist())
        assert gt & chosen and gt - chosen
    vol = TO.class_planes_scatter(sel.to(dev), inv.to(dev), torch.empty(B, T0, h, h, device=dev), -100.0)
    vol_cpu = vol.cpu()
    assert int((vol_cpu == -100.0).all(-1).all(-1).sum()) == B * (T0 - k)
    ref = reference_loss(vol_cpu, targets, 255)
    got = ops.bce_onehot_loss(vol, targets.to(dev), 255).item()
    print(f"loss on -100 planes: hip {got!r} ref {ref!r} rel {abs(got - ref) / abs(ref):.3e}")
    assert got == got and abs(got) != float("inf")
    assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-6, (got, ref)
    gref = reference_grad(vol_cpu, targets, 255)
    ggot = ops.bce_onehot_loss_backward(vol, targets.to(dev), 255).cpu().double()
    assert bool(torch.isfinite(ggot).all())
    err, tol = (ggot - gref).abs().max().item(), 2e-5 * gref.abs().max().item()
    print(f"gradient on -100 planes: max err {err:.3e} gate {tol:.3e}")
    assert err <= tol, (err, tol)
