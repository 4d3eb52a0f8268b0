"""Training with visual prompt tuning (CLIP_FINETUNE "prompt", model_vpt.py:243-266) on the device.

catseg_vpt_rows_forward / _backward (the prompt rows of the vision stream: expand, in-place rewrite,
strip, and the fixed-order batch reduction of their gradient) against torch fp64; then
clip_image_train_forward with prompts against fp64 autograd through the oracle, the whole
CATSeg.train() step against tests/golden/train_tiny_vpt.npz (the REFERENCE's own modules,
tests/golden/make_golden_train_vpt.py), CLIP_FINETUNE "none" on prompt-carrying features, the
PROMPT_DEPTH refusal, and the PROMPT_LENGTH 0 step unchanged.

Gates: copies exact (torch.equal); the reduction at tests/test_gpu_train_ops.py's rule, max |hip - ref|
<= 1e-4 * max |ref|; features and hooks at tests/test_gpu_train_head.py's forward gate (1e-4), the loss
1e-5 relative, gradients by compare_grads / max(1e-4, 8 x the reference's own fp32 error).
"""
import functools
import hashlib
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from cat_seg import build_model, train_ops as TO  # noqa: E402
from cat_seg.arch import TINY  # noqa: E402
from cat_seg.weights import CLIP, synthesize_state_dict  # noqa: E402
from oracle import catseg_oracle as O  # noqa: E402

from conftest import ROOT  # noqa: E402
from test_boundary_cpu import tiny_cfg  # noqa: E402
from test_gpu_train_head import TOL, compare_grads, head_keys, ref_head, ref_loss  # noqa: E402
from test_gpu_train_ops import close, g  # noqa: E402

DEV = "cuda"
SENT = -1234.5
NAN = float("nan")
PROMPTS = CLIP + "visual.transformer.prompt_tokens"
VPT_ARCH = TINY.replace(prompt_depth=4, prompt_length=3, pooling_size=(2, 2))
W_TINY = TINY.vision_width

# (B, L0, P, W): one image / one prompt; odd L0 with several images; the ViT-L width; ViT-B/16@384's
# 577-token sequences with 10 prompts (several workgroups per launch, P*W/4 > 256 in the reduction)
SHAPES = [(1, 5, 1, W_TINY), (2, 17, 3, W_TINY), (3, 17, 3, 1024), (2, 577, 10, 1024)]


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))


def vpt_cfg(finetune="prompt", depth=4, length=3, **over):
    return tiny_cfg(**{"MODEL.SEM_SEG_HEAD.POOLING_SIZES": "[2,2]", "MODEL.SEM_SEG_HEAD.PROMPT_DEPTH": str(depth),
                       "MODEL.SEM_SEG_HEAD.PROMPT_LENGTH": str(length),
                       "MODEL.SEM_SEG_HEAD.CLIP_FINETUNE": finetune, **over})


# ------------------------------------------------------------------------------------- kernels
def wide(t, left, right, fill):
    """t (rows, W) as the column slice [left : left + W] of a wider device buffer filled with `fill`."""
    rows, W = t.shape
    buf = torch.full((rows, left + W + right), fill, device=DEV, dtype=torch.float32)
    buf[:, left:left + W] = t.float().to(DEV)
    return buf, buf[:, left:left + W]


def slack_kept(buf, left, W):
    return (torch.equal(buf[:, :left], torch.full_like(buf[:, :left], SENT))
            and torch.equal(buf[:, left + W:], torch.full_like(buf[:, left + W:], SENT)))


@functools.lru_cache(maxsize=None)
def kernel_data(B, L0, P, W):
    """fp64 inputs: body (B, L0, W), stream (B, Ls, W), prompt (P, W), dx (B, Ls, W), dprompt0 (P, W)."""
    return (g(B, L0, W, seed=31), g(B, L0 + P, W, seed=32), g(P, W, seed=33), g(B, L0 + P, W, seed=34),
            g(P, W, seed=35))


@pytest.mark.parametrize("B,L0,P,W", SHAPES)
def test_vpt_rows_forward_expand_rewrite_strip(B, L0, P, W):
    body, stream, prompt, _, _ = kernel_data(B, L0, P, W)
    Ls = L0 + P
    _, src = wide(body.reshape(B * L0, W), 4, 8, NAN)
    _, pr = wide(prompt, 8, 4, NAN)
    # expand: body rows + this layer's prompts in every image's tail
    dbuf, dst = wide(torch.full((B * Ls, W), SENT), 12, 4, SENT)
    TO.vpt_rows(dst, B=B, L0=L0, P=P, src=src, prompt=pr)
    want = torch.cat([body, prompt.unsqueeze(0).expand(B, P, W)], 1).reshape(B * Ls, W).float().to(DEV)
    assert torch.equal(dst, want)
    assert slack_kept(dbuf, 12, W)
    # expand with zero tails (the strip's backward)
    zbuf, zdst = wide(torch.full((B * Ls, W), SENT), 4, 4, SENT)
    TO.vpt_rows(zdst, B=B, L0=L0, P=P, src=src)
    wz = torch.cat([body, torch.zeros(B, P, W, dtype=body.dtype)], 1).reshape(B * Ls, W).float().to(DEV)
    assert torch.equal(zdst, wz)
    assert slack_kept(zbuf, 4, W)
    # in-place rewrite: only the tail rows change
    sbuf, st = wide(stream.reshape(B * Ls, W), 8, 12, SENT)
    TO.vpt_rows(st, B=B, L0=L0, P=P, prompt=pr)
    ws = stream.clone()
    ws[:, L0:] = prompt
    assert torch.equal(st, ws.reshape(B * Ls, W).float().to(DEV))
    assert slack_kept(sbuf, 8, W)
    # strip: the inverse copy
    _, full = wide(stream.reshape(B * Ls, W), 4, 4, NAN)
    obuf, out = wide(torch.full((B * L0, W), SENT), 8, 8, SENT)
    TO.vpt_strip(full, out, B=B, L0=L0, P=P)
    assert torch.equal(out, stream[:, :L0].reshape(B * L0, W).float().to(DEV))
    assert slack_kept(obuf, 8, W)


@pytest.mark.parametrize("B,L0,P,W", SHAPES)
def test_vpt_rows_backward_reduces_and_zeroes(B, L0, P, W):
    _, _, _, dx, dp0 = kernel_data(B, L0, P, W)
    Ls = L0 + P
    dx32 = dx.float()                                    # what the kernel reads
    ref = dx32.double()[:, L0:].sum(0)                   # fp64 sum of the fp32 inputs
    body = dx32[:, :L0].to(DEV)
    runs = []
    for beta in (0, 1, 0):
        xbuf, x = wide(dx32.reshape(B * Ls, W), 8, 4, SENT)
        init = dp0.float() if beta else torch.full((P, W), NAN)      # overwrite never reads dprompt
        pbuf, dp = wide(init, 4, 12, SENT)
        TO.vpt_rows_backward(x, dp, B=B, L0=L0, P=P, beta=beta)
        close(dp, ref + dp0.float().double() if beta else ref)
        x3 = x.reshape(B, Ls, W)
        assert torch.equal(x3[:, :L0], body)             # body rows untouched
        assert torch.equal(x3[:, L0:], torch.zeros(B, P, W, device=DEV))
        assert slack_kept(xbuf, 8, W) and slack_kept(pbuf, 4, W)
        runs.append(dp.clone())
    assert torch.equal(runs[0], runs[2])                 # fresh buffers, bit-identical
    # the fixed order b = 0..B-1 in fp32, exactly
    seq = torch.zeros(P, W)
    for b in range(B):
        seq = seq + dx32[b, L0:]
    assert torch.equal(runs[0].cpu(), seq)
    # frozen prompts: the rows are zeroed, nothing else is written
    xbuf, x = wide(dx32.reshape(B * Ls, W), 4, 4, SENT)
    TO.vpt_rows_backward(x, None, B=B, L0=L0, P=P)
    x3 = x.reshape(B, Ls, W)
    assert torch.equal(x3[:, :L0], body) and not x3[:, L0:].any().item()
    assert slack_kept(xbuf, 4, W)


# ------------------------------------------------------------------------------------- image encoder
CLIP_B = 2


def _block_keys(sd):
    return [k for k in sd if k.startswith(CLIP + "visual.transformer.resblocks")]


def _qv_keys(sd):
    return [k for k in _block_keys(sd) if "q_proj" in k or "v_proj" in k]


@functools.lru_cache(maxsize=None)
def clip_reference():
    """Images, the random linear loss' coefficients, and through the oracle (model_vpt.py:243-266,
    288-314): fp64 feats / hooks and the gradients of the prompt tokens and every visual block parameter
    in fp64 and in torch fp32."""
    arch = VPT_ARCH
    sd = synthesize_state_dict(arch, seed=0)
    keys = [PROMPTS] + _block_keys(sd)
    gen = torch.Generator().manual_seed(4)
    ims = [torch.randint(0, 256, (3, 384, 384), generator=gen).float() for _ in range(CLIP_B)]
    L0 = arch.grid ** 2 + 1
    rf = torch.randn(CLIP_B, L0, arch.embed_dim, generator=gen, dtype=torch.float64)
    rh = [torch.randn(CLIP_B, L0, arch.vision_width, generator=gen, dtype=torch.float64) for _ in range(2)]
    refs, outs = {}, None
    for dt in (torch.float64, torch.float32):
        sdr = {k: v.detach().clone().to(dt).requires_grad_(k in keys) for k, v in sd.items()}
        clip_ims, _ = O.preprocess(arch, ims)
        feats, hooks = O.encode_image_dense(arch, sdr, clip_ims.to(dt))
        loss = (feats * rf.to(dt)).sum()
        for h, r in zip(hooks, rh):
            loss = loss + (h.permute(1, 0, 2) * r.to(dt)).sum()
        loss.backward()
        refs[dt] = {k: sdr[k].grad for k in keys}
        if dt == torch.float64:
            outs = (feats.detach(), [h.detach().permute(1, 0, 2) for h in hooks])
    return sd, ims, rf, rh, refs, outs


@pytest.mark.parametrize("mode", ["prompt", "attention", "full"])
def test_clip_image_train_forward_with_prompts_matches_oracle_autograd(mode):
    """The image encoder with 3 prompt rows in each of TINY's 4 blocks, B = 2, on a random linear loss of
    the features and both hooks: "prompt" trains the prompt tokens alone, "attention" the q / v projections
    with the prompts frozen (no reduction launch), "full" every block parameter and the prompts."""
    from cat_seg.engine import CatSegEngine
    from cat_seg.training import clip_image_train_forward
    arch = VPT_ARCH
    sd, ims, rf, rh, refs, (ref_feats, ref_hooks) = clip_reference()
    keys = {"prompt": [PROMPTS], "attention": _qv_keys(sd), "full": [PROMPTS] + _block_keys(sd)}[mode]
    L0 = arch.grid ** 2 + 1
    eng = CatSegEngine(arch, sd, dtype=torch.float32, device=DEV)
    P = {k: v.detach().to(DEV).requires_grad_(k in keys) for k, v in sd.items()}
    raw = torch.stack(ims).to(DEV)
    sizes = torch.tensor([[384, 384]] * CLIP_B, dtype=torch.int32, device=DEV)
    launches = []
    real_bwd = TO.vpt_rows_backward
    TO.vpt_rows_backward = lambda dx, dprompt, **kw: (launches.append(dprompt is not None), real_bwd(dx, dprompt, **kw))[1]
    try:
        feats, hooks = clip_image_train_forward(arch, P, eng, raw, sizes)
        assert feats.shape == (CLIP_B * L0, arch.embed_dim) and all(h.shape == (CLIP_B * L0, arch.vision_width) for h in hooks)
        ef = (feats.detach().cpu().double().reshape(ref_feats.shape) - ref_feats).abs().max().item()
        eh = [(h.detach().cpu().double().reshape(r.shape) - r).abs().max().item() for h, r in zip(hooks, ref_hooks)]
        print(f"vpt {mode}: feats err {ef:.3e}, hooks err {eh[0]:.3e} {eh[1]:.3e}")
        assert ef < 1e-4 and max(eh) < 1e-4
        loss = (feats * rf.reshape(CLIP_B * L0, -1).float().to(DEV)).sum()
        for h, r in zip(hooks, rh):
            loss = loss + (h * r.reshape(CLIP_B * L0, -1).float().to(DEV)).sum()
        loss.backward()
    finally:
        TO.vpt_rows_backward = real_bwd
    rows = compare_grads({k: P[k].grad for k in keys}, refs[torch.float64], keys, ref32=refs[torch.float32])
    print(f"vpt {mode}: worst gradients {rows[:3]}")
    if mode != "attention":
        # one reduction per prompt-carrying block (the dense block runs on stripped rows)
        assert launches == [True] * (arch.vision_layers - 1)
        pg = P[PROMPTS].grad
        assert pg.shape == (4, 3, arch.vision_width)
        assert not pg[arch.vision_layers - 1].any().item()           # == 0, as in the reference
        assert refs[torch.float64][PROMPTS][arch.vision_layers - 1].abs().max().item() == 0.0
        if mode == "prompt":
            assert all(P[k].grad is None for k in _block_keys(sd))
    else:
        # frozen prompts: no gradient and no reduction, the tail rows of dx are only zeroed
        assert P[PROMPTS].grad is None
        assert launches and not any(launches)


# ------------------------------------------------------------------------------------- the whole step
def _train_inputs():
    base = golden("train_tiny_pool2")
    ims = [torch.from_numpy(base["image0"]).float(), torch.from_numpy(base["image1"]).float()]
    return ims, torch.from_numpy(base["tokens"]), torch.from_numpy(base["targets"]).long()


def test_catseg_train_step_prompt_mode_matches_reference_gradients():
    """CATSeg.train() with CLIP_FINETUNE "prompt" pinned to the REFERENCE's own modules
    (tests/golden/train_tiny_vpt.npz), then one build_optimizer AdamW step and an eval forward on the
    updated weights against the oracle: the eval engine must have picked up the new prompt tokens."""
    from cat_seg.optim import AdamW, build_optimizer
    g_ = golden("train_tiny_vpt")
    ims, toks, tg = _train_inputs()
    assert np.array_equal(g_["tokens"], toks.numpy()) and np.array_equal(g_["targets"], tg.numpy())
    cfg = vpt_cfg(**{"SOLVER.BASE_LR": "0.01", "SOLVER.CLIP_MULTIPLIER": "0.1"})
    model = build_model(cfg).to(DEV)
    model.sem_seg_head.predictor.set_class_tokens(toks)
    model.train()
    loss = model([{"image": ims[i], "sem_seg": tg[i]} for i in range(2)])["loss_sem_seg"]
    loss.backward()
    l64 = float(g_["loss64"])
    print(f"vpt step: loss {loss.item():.9g} reference {l64:.9g}")
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64), (loss.item(), l64)
    named = dict(model.named_parameters())
    names = [str(k) for k in g_["names"]]
    assert {k for k, p in named.items() if p.requires_grad} == set(names) | {str(k) for k in g_["none"]}
    assert all(named[k].grad is None for k in named if k not in names)
    worst = (0.0, 0.0, "")
    for k in names:
        mx, e32 = (float(v) for v in g_["m_" + k])
        got = named[k].grad.detach().double().cpu().reshape(-1)
        if ".swin_block." in k and k.endswith("attn.k.bias"):
            scale = float(g_["m_" + k[:-len("bias")] + "weight"][0])
            assert got.abs().max().item() <= 1e-5 * scale, k
            continue
        if mx == 0.0:
            assert got.abs().max().item() == 0.0, k
            continue
        idx = torch.from_numpy(g_["i_" + k])
        err = max((got[idx] - torch.from_numpy(g_["g_" + k])).abs().max().item() / mx,
                  abs(got.abs().max().item() - mx) / mx)
        worst = max(worst, (err / max(TOL, 8 * e32), err, k))
        assert err <= max(TOL, 8 * e32), f"{k}: {err:.3e} (reference fp32 {e32:.3e})"
    print(f"vpt step: worst gradient (fraction of its gate, rel err, key) {worst}")
    # the whole prompt gradient, the last layer's slice exactly zero
    pg = named[PROMPTS].grad.detach().double().cpu()
    rp = torch.from_numpy(g_["prompt_grad"])
    mx, e32 = (float(v) for v in g_["m_" + PROMPTS])
    assert (pg - rp).abs().max().item() / mx <= max(TOL, 8 * e32)
    assert not pg[3].any().item()

    before = model.engine.w.vpt.clone()
    opt = build_optimizer(cfg, model)
    assert isinstance(opt, AdamW)
    grp = [x for x in opt.param_groups if any(q is named[PROMPTS] for q in x["params"])]
    assert len(grp) == 1 and grp[0]["lr"] == pytest.approx(0.01 * 0.1) and grp[0]["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY
    opt.step()
    model.eval()
    with torch.no_grad():
        out = model([{"image": ims[0]}])[0]["sem_seg"]
    after = model.engine.w.vpt
    assert not torch.equal(after, before)
    assert torch.equal(after, named[PROMPTS].detach().reshape(4, -1))
    arch = model.arch
    sd_new = {k: v.detach().cpu() for k, v in model.named_parameters()}
    ref = O.catseg_forward(arch, sd_new, [{"image": ims[0]}], O.text_embeds(arch, sd_new, toks))[0]["sem_seg"]
    assert (out.cpu() - ref).abs().max().item() < 1e-3


def test_catseg_train_step_frozen_clip_with_prompts():
    """CLIP_FINETUNE "none" with prompts configured: the engine's features carry the prompt rows and are
    stripped for the head; the head's gradients against the oracle fed with the oracle's own
    prompt-carrying CLIP features."""
    ims, toks, tg = _train_inputs()
    T = 4                                  # the first classes only: the fp64 / fp32 reference head scales with T
    toks, tg = toks[:T], torch.where(tg == 255, tg, tg % T)
    model = build_model(vpt_cfg("none")).to(DEV)
    model.sem_seg_head.predictor.set_class_tokens(toks)
    model.train()
    loss = model([{"image": ims[i], "sem_seg": tg[i]} for i in range(2)])["loss_sem_seg"]
    loss.backward()
    named = dict(model.named_parameters())
    keys = [k for k, p in named.items() if p.requires_grad]
    assert set(keys) == set(head_keys(named))
    assert all(named[k].grad is None for k in named if k not in keys)
    arch = model.arch

    def reference(dt):
        sdr = {k: v.detach().cpu().clone().to(dt).requires_grad_(k in keys) for k, v in named.items()}
        with torch.no_grad():
            clip_ims, _ = O.preprocess(arch, ims)
            feats, hooks = O.encode_image_dense(arch, sdr, clip_ims.to(dt))
            text = O.text_embeds(arch, sdr, toks)[:, 0]
        rl = ref_loss(ref_head(arch, sdr, feats, hooks, text), tg.int())
        rl.backward()
        return {k: sdr[k].grad for k in keys}, rl.item()

    ref64, rl64 = reference(torch.float64)
    assert abs(loss.item() - rl64) <= 1e-5 * abs(rl64), (loss.item(), rl64)
    got = {k: named[k].grad for k in keys}
    try:
        # within 1e-4 everywhere is within max(1e-4, 8 x the fp32 reference's error): the fp32 reference
        # pass is only run when a gradient needs that allowance
        compare_grads(got, ref64, keys)
    except AssertionError:
        compare_grads(got, ref64, keys, ref32=reference(torch.float32)[0])


def test_prompt_depth_below_the_layer_count_stays_refused():
    ims, toks, tg = _train_inputs()
    model = build_model(vpt_cfg(depth=2)).to(DEV)
    model.sem_seg_head.predictor.set_class_tokens(toks)
    model.train()
    with pytest.raises(NotImplementedError, match="PROMPT_DEPTH"):
        model([{"image": ims[0], "sem_seg": tg[0]}])


def step_digest(model, ims, tg):
    """Loss bits and a SHA-256 over every gradient of one training step (parameter order)."""
    loss = model([{"image": ims[i], "sem_seg": tg[i]} for i in range(2)])["loss_sem_seg"]
    loss.backward()
    h = hashlib.sha256()
    for k, p in model.named_parameters():
        if p.grad is not None:
            h.update(k.encode())
            h.update(p.grad.detach().cpu().contiguous().numpy().tobytes())
    return float(loss.item()).hex(), h.hexdigest()


def test_step_without_prompts_is_unchanged(monkeypatch):
    """PROMPT_LENGTH 0 (the tiny CLIP_FINETUNE "attention" step): no prompt-row kernel runs, the step is
    the one tests/golden/train_tiny_pool2.npz gates (tests/test_gpu_train_head.py's rule), and two runs
    agree bit for bit.  The printed digest is the figure compared across commits on one box."""
    def boom(*a, **k):
        raise AssertionError("a prompt-row kernel ran without prompts")
    for name in ("vpt_rows", "vpt_strip", "vpt_rows_backward"):
        monkeypatch.setattr(TO, name, boom, raising=False)
    g_ = golden("train_tiny_pool2")
    ims, toks, tg = _train_inputs()
    digests = []
    for _ in range(2):
        model = build_model(tiny_cfg(**{"MODEL.SEM_SEG_HEAD.POOLING_SIZES": "[2,2]"})).to(DEV)
        model.sem_seg_head.predictor.set_class_tokens(toks)
        model.train()
        digests.append(step_digest(model, ims, tg))
    print(f"no-prompt attention step: loss bits {digests[0][0]} gradient sha256 {digests[0][1]}")
    assert digests[0] == digests[1]
    l64 = float(g_["loss64"])
    assert abs(float.fromhex(digests[0][0]) - l64) <= 1e-5 * abs(l64)
    named = dict(model.named_parameters())
    for k in (str(k) for k in g_["names"]):
        mx, e32 = (float(v) for v in g_["m_" + k])
        got = named[k].grad.detach().double().cpu().reshape(-1)
        if ".swin_block." in k and k.endswith("attn.k.bias"):
            assert got.abs().max().item() <= 1e-5 * float(g_["m_" + k[:-len("bias")] + "weight"][0]), k
            continue
        if mx == 0.0:
            assert got.abs().max().item() == 0.0, k
            continue
        idx = torch.from_numpy(g_["i_" + k])
        err = max((got[idx] - torch.from_numpy(g_["g_" + k])).abs().max().item() / mx,
                  abs(got.abs().max().item() - mx) / mx)
        assert err <= max(TOL, 8 * e32), f"{k}: {err:.3e} (reference fp32 {e32:.3e})"
