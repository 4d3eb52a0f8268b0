"""Training with ATTENTION_TYPE "full": catseg_full_attention_backward (the class softmax attention's
backward over the padded class axis, class-major rows) against torch fp64 autograd of the oracle's
FullAttention on the explicitly padded axis, the training forward catseg_full_attention_train_forward
against the same oracle, then both through head_train_forward and CATSeg.train().

Gates: the kernel at tests/test_gpu_train_ops.py's rule, max |hip - ref| <= 1e-4 * max |ref| per
output; the head and the model at tests/test_gpu_train_head.py's own gates (logits 1e-4, loss 1e-5
relative, gradients by compare_grads / max(1e-4, 8 x the reference's own fp32 error)).  The class
layers' attention.k.bias gradients are zero in exact arithmetic (the bias shifts every score of a
softmax row, the pad column included): they are held to 1e-5 of the k weight's gradient scale, as the
Swin k biases are.
"""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from cat_seg import build_model, ops, train_ops as TO  # noqa: E402
from cat_seg.training import head_train_forward  # noqa: E402
from cat_seg.weights import synthesize_state_dict  # noqa: E402
from oracle import catseg_oracle as O  # noqa: E402

from conftest import ROOT  # noqa: E402
from test_boundary_cpu import tiny_cfg  # noqa: E402
from test_gpu_train_head import CASES, TOL, compare_grads, head_keys, ref_head, ref_loss  # noqa: E402
from test_gpu_train_ops import close, dev, g  # noqa: E402

DEV = "cuda"
B, HW, NH, D = 2, 9, 4, 128
HD = D // NH

# (T, n_pad, q scale, pad scale)
KERNEL_CASES = [(20, 236, 1, 1), (171, 85, 1, 1), (256, 0, 1, 1), (37, 0, 1, 1), (10, 6, 1, 1), (16, 1, 1, 1),
                (1, 3, 1, 1), (300, 0, 1, 1), (65, 191, 1, 1),
                (20, 236, 8, 1),        # peaked softmax: the running-max path
                (20, 236, 1, 3),        # pad column dominant
                (171, 85, 4, 3)]


@functools.lru_cache(maxsize=None)
def reference(T, n_pad, qs, ps):
    """Inputs, the fp64 autograd gradients and the fp64 attention output:
    (qkv, kv_pad, dy, dq, dk, dv, dk_pad, dv_pad, out)."""
    R = B * T * HW
    qkv = g(R, 3 * D, seed=25)
    qkv[:, :D] *= qs
    kv_pad = g(2, D, seed=26) * ps
    dy = g(R, D, seed=27)
    qr, kr, vr = (qkv[:, i * D:(i + 1) * D].clone().requires_grad_(True) for i in range(3))
    kp, vp = (kv_pad[i].clone().requires_grad_(True) for i in range(2))

    def seq(t, pad):      # rows (b, t, p) -> (b*p, T + n_pad, nh, hd)
        t = t.reshape(B, T, HW, D).permute(0, 2, 1, 3)
        if n_pad:
            t = torch.cat([t, pad.reshape(1, 1, 1, D).expand(B, HW, n_pad, D)], 2)
        return t.reshape(B * HW, T + n_pad, NH, HD)

    out = O.full_attention(seq(qr, kp), seq(kr, kp), seq(vr, vp))[:, :T]
    out = out.reshape(B, HW, T, D).permute(0, 2, 1, 3).reshape(R, D)
    out.backward(dy)
    return (qkv, kv_pad, dy, qr.grad, kr.grad, vr.grad, kp.grad if n_pad else None, vp.grad if n_pad else None,
            out.detach())


def run_kernel(qkv, dy, dqkv, kv_pad, T, n_pad):
    dkp = torch.full((D,), 7.0, device=DEV)
    dvp = torch.full((D,), 7.0, device=DEV)
    kw = dict(k_pad=dev(kv_pad[0]), v_pad=dev(kv_pad[1]), dk_pad=dkp, dv_pad=dvp) if n_pad else {}
    TO.full_attention_backward(qkv, dy, dqkv, B=B, T=T, HW=HW, n_heads=NH, head_dim=HD, n_pad=n_pad, **kw)
    return dkp, dvp


@pytest.mark.parametrize("T,n_pad,qs,ps", KERNEL_CASES)
def test_full_attention_backward(T, n_pad, qs, ps):
    qkv, kv_pad, dy, dq, dk, dv, dkp_r, dvp_r, _ = reference(T, n_pad, qs, ps)
    dqkv = torch.empty(B * T * HW, 3 * D, device=DEV)
    dkp, dvp = run_kernel(dev(qkv), dev(dy), dqkv, kv_pad, T, n_pad)
    close(dqkv[:, :D], dq)
    close(dqkv[:, D:2 * D], dk)
    close(dqkv[:, 2 * D:], dv)
    if n_pad:
        close(dkp, dkp_r)
        close(dvp, dvp_r)


@pytest.mark.parametrize("T,n_pad,qs,ps", KERNEL_CASES)
def test_full_attention_train_forward(T, n_pad, qs, ps):
    """y = x + attention on the class-major rows (catseg_full_attention_train_forward, scores on the f64
    MFMA) against the fp64 oracle, at test_gpu_train_ops.py's forward gate (1e-5 of the largest value);
    x and y as column slices of wider buffers, y's slack keeps its sentinel."""
    qkv, kv_pad, _, _, _, _, _, _, out = reference(T, n_pad, qs, ps)
    R = B * T * HW
    x = g(R, D, seed=28)
    wx = torch.full((R, D + 8), float("nan"), device=DEV)
    wx[:, 4:4 + D] = dev(x)
    wy = torch.full((R, D + 8), -1234.5, device=DEV)
    kw = dict(k_pad=dev(kv_pad[0]), v_pad=dev(kv_pad[1])) if n_pad else {}
    TO.full_attention_forward(dev(qkv), wx[:, 4:4 + D], wy[:, 4:4 + D], B=B, T=T, HW=HW, n_heads=NH, head_dim=HD,
                              n_pad=n_pad, **kw)
    close(wy[:, 4:4 + D] - wx[:, 4:4 + D], out, 1e-5)
    assert torch.equal(wy[:, :4], torch.full_like(wy[:, :4], -1234.5))
    assert torch.equal(wy[:, 4 + D:], torch.full_like(wy[:, 4 + D:], -1234.5))


def test_full_attention_backward_strided_buffers_and_determinism():
    """q / k / v, dy and the outputs as column slices of wider buffers (row strides larger than the
    payload): the slack columns of the inputs hold NaN and are never read, those of the outputs keep
    their sentinel, the results equal the dense-buffer run's gates, and a second run into fresh buffers
    is bit-identical for all five outputs."""
    T, n_pad = 65, 191
    qkv, kv_pad, dy, dq, dk, dv, dkp_r, dvp_r, _ = reference(T, n_pad, 1, 1)
    R = B * T * HW
    SENT = -1234.5
    wq = torch.full((R, 3 * D + 24), float("nan"), device=DEV)
    wq[:, 8:8 + 3 * D] = dev(qkv)
    wy = torch.full((R, D + 12), float("nan"), device=DEV)
    wy[:, 4:4 + D] = dev(dy)
    runs = []
    for _ in range(2):
        wd = torch.full((R, 3 * D + 20), SENT, device=DEV)
        dkp, dvp = run_kernel(wq[:, 8:8 + 3 * D], wy[:, 4:4 + D], wd[:, 12:12 + 3 * D], kv_pad, T, n_pad)
        assert torch.equal(wd[:, :12], torch.full_like(wd[:, :12], SENT))
        assert torch.equal(wd[:, 12 + 3 * D:], torch.full_like(wd[:, 12 + 3 * D:], SENT))
        runs.append((wd[:, 12:12 + D], wd[:, 12 + D:12 + 2 * D], wd[:, 12 + 2 * D:12 + 3 * D], dkp, dvp))
    for got, ref in zip(runs[0], (dq, dk, dv, dkp_r, dvp_r)):
        close(got, ref)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def _class_k_bias(k):
    return ".swin_block." not in k and k.endswith(".attention.attention.k.bias")


def _check_class_k_biases(keys, got, wscale):
    """got(k) -> gradient, wscale(k) -> max |reference gradient| of the matching k weight."""
    kb = [k for k in keys if _class_k_bias(k)]
    assert kb
    for k in kb:
        a = got(k).detach().double().abs().max().item()
        s = wscale(k[:-len("bias")] + "weight")
        assert a <= 1e-5 * s, (k, a, s)


@pytest.mark.parametrize("case", list(CASES))
def test_head_backward_full_attention_matches_oracle_autograd(case):
    """test_gpu_train_head.test_head_backward_matches_oracle_autograd with attention_type "full".

    The forward is catseg_full_attention_train_forward (scores on the f64 MFMA).  With the eval path's fp32
    flash forward instead, tiny_pool1_pad missed this gate on 7 parameters (worst 5.54e-4 against
    5.37e-4): peaked softmax rows multiply the fp32 rounding of a score, DESIGN section 9."""
    arch, Bh, T = CASES[case]
    arch = arch.replace(attention_type="full")
    sd = synthesize_state_dict(arch, seed=0)
    keys = head_keys(sd)
    L_ = arch.grid ** 2 + 1
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(Bh, L_, arch.embed_dim, generator=gen, dtype=torch.float64)
    hooks = [torch.randn(Bh, L_, arch.vision_width, generator=gen, dtype=torch.float64) for _ in range(2)]
    text = F.normalize(torch.randn(T, arch.embed_dim, generator=gen, dtype=torch.float64), dim=-1)
    R = 4 * arch.grid
    targets = torch.randint(0, T, (Bh, R, R), generator=gen, dtype=torch.int32)
    targets[:, :3] = 255

    ref_grads = {}
    for dt, store in ((torch.float64, ref_grads), (torch.float32, {})):
        sdr = {k: v.detach().clone().to(dt).requires_grad_(k in keys) for k, v in sd.items()}
        lg = ref_head(arch, sdr, feats.to(dt), [h.permute(1, 0, 2).to(dt) for h in hooks], text.to(dt))
        l_ = ref_loss(lg, targets)
        l_.backward()
        store.update({k: sdr[k].grad for k in keys})
        if dt == torch.float64:
            ref_logits, rl = lg, l_
        else:
            ref32 = store

    P = {k: v.detach().cuda().requires_grad_(k in keys) for k, v in sd.items()}
    logits = head_train_forward(arch, P, feats.reshape(Bh * L_, -1).float().cuda(),
                                [h.reshape(Bh * L_, -1).float().cuda() for h in hooks], text.float().cuda())
    assert logits.shape == (Bh, T, R, R) and logits.requires_grad
    assert (logits.detach().cpu().double() - ref_logits.detach()).abs().max().item() < 1e-4
    loss = ops.BCEOneHotLoss.apply(logits, targets.cuda(), 255)
    assert abs(loss.item() - rl.item()) <= 1e-5 * abs(rl.item())
    loss.backward()
    _check_class_k_biases(keys, lambda k: P[k].grad, lambda k: ref_grads[k].double().abs().max().item())
    rest = [k for k in keys if not _class_k_bias(k)]
    compare_grads({k: P[k].grad for k in rest}, ref_grads, rest, ref32=ref32)


def test_catseg_train_step_full_attention_matches_reference_gradients():
    """The whole training step with ATTENTION_TYPE "full" pinned to the REFERENCE's own modules:
    tests/golden/train_tiny_full_pool2.npz (tests/golden/make_golden_train_full.py: the reference's
    model_vpt.CLIP and Aggregator(attention_type="full") in float64 / float32).  Its inputs are those of
    train_tiny_pool2.npz, where the two images are kept.  Then one torch.optim.AdamW step and an eval
    forward on the updated weights against the oracle."""
    g_ = np.load(os.path.join(ROOT, "tests", "golden", "train_tiny_full_pool2.npz"))
    base = np.load(os.path.join(ROOT, "tests", "golden", "train_tiny_pool2.npz"))
    assert np.array_equal(g_["tokens"], base["tokens"]) and np.array_equal(g_["targets"], base["targets"])
    cfg = tiny_cfg(**{"MODEL.SEM_SEG_HEAD.POOLING_SIZES": "[2,2]", "MODEL.SEM_SEG_HEAD.ATTENTION_TYPE": "full"})
    model = build_model(cfg).cuda()
    toks = torch.from_numpy(g_["tokens"])
    model.sem_seg_head.predictor.set_class_tokens(toks)
    ims = [torch.from_numpy(base["image0"]).float(), torch.from_numpy(base["image1"]).float()]
    tg = torch.from_numpy(g_["targets"]).long()
    model.train()
    loss = model([{"image": ims[i], "sem_seg": tg[i]} for i in range(2)])["loss_sem_seg"]
    loss.backward()
    l64 = float(g_["loss64"])
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64), (loss.item(), l64)
    named = dict(model.named_parameters())
    names = [str(k) for k in g_["names"]]
    assert {k for k, p in named.items() if p.requires_grad} == set(names) | {str(k) for k in g_["none"]}
    _check_class_k_biases(names, lambda k: named[k].grad, lambda k: float(g_["m_" + k][0]))
    for k in names:
        mx, e32 = (float(v) for v in g_["m_" + k])
        got = named[k].grad.detach().double().cpu().reshape(-1)
        if _class_k_bias(k):
            continue
        if ".swin_block." in k and k.endswith("attn.k.bias"):
            scale = float(g_["m_" + k[:-len("bias")] + "weight"][0])
            assert got.abs().max().item() <= 1e-5 * scale, k
            continue
        if mx == 0.0:                 # the dense block's dead q / k projections
            assert got.abs().max().item() == 0.0, k
            continue
        idx = torch.from_numpy(g_["i_" + k])
        err = max((got[idx] - torch.from_numpy(g_["g_" + k])).abs().max().item() / mx,
                  abs(got.abs().max().item() - mx) / mx)
        assert err <= max(TOL, 8 * e32), f"{k}: {err:.3e} (reference fp32 {e32:.3e})"

    # an optimizer step on the real parameters; eval then runs on the new weights
    before = model.engine.w.ce_b.clone()
    opt = torch.optim.AdamW([p for p in model.parameters() if p.requires_grad and p.grad is not None], lr=1e-3)
    opt.step()
    model.eval()
    with torch.no_grad():
        out = model([{"image": ims[0]}])[0]["sem_seg"]
    assert not torch.equal(model.engine.w.ce_b, before)
    arch = model.arch
    sd_new = {k: v.detach().cpu() for k, v in model.named_parameters()}
    ref = O.catseg_forward(arch, sd_new, [{"image": ims[0]}], O.text_embeds(arch, sd_new, toks))[0]["sem_seg"]
    assert (out.cpu() - ref).abs().max().item() < 1e-3
