"""Training with more classes than pad_len: the head's per-image top-k branch (model.py:691-725) on the
device against torch autograd through the pinned oracle in float64, as tests/test_gpu_train_head.py does
for T <= pad_len (its helpers and every gate are imported from there: logits 1e-4 absolute, loss 1e-5
relative, gradients max(1e-4, 8 x torch-fp32 error) with the k-bias rule), and the whole training step
against the REFERENCE's own modules (tests/golden/train_tiny_topk.npz, tests/golden/make_golden_topk.py).

T0 = 31 classes, pad_len 24, B = 2: each image keeps its own 24 classes, the sets differ and overlap, the
targets are drawn over all 31 classes, so ground truth in unselected classes occurs (softplus(100) there).
`text` is a requires_grad leaf on both sides: its gradient is the one tensor that goes through both uses
of catseg_class_rows_reduce (the text guidance rows and the normalized text rows of the cost volume).
Every test first asserts on the CPU that the selection is well separated (gap >= 1e-3 between the 24th and
25th class maximum: ~6000 x the fp32-vs-fp64 deviation of the maxima), so that the device's fp32 summation
order cannot legitimately select another set."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cat_seg import build_model, ops, training
from cat_seg.arch import TINY
from cat_seg.training import head_train_forward
from cat_seg.weights import synthesize_state_dict

from test_boundary_cpu import tiny_cfg
from test_gpu_train_head import TOL, _write_report, compare_grads, head_keys, ref_head, ref_loss
from test_gpu_training_loss import reference_loss
from test_train_topk_cpu import ARCH, PAD_LEN, T0, default_dtype, load_golden

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, os.cpu_count() or 1))

B = 2
CASES = {
    "tiny_pool2_topk": ARCH,
    "tiny_pool1_topk": TINY.replace(pad_len=PAD_LEN),
    "tiny_pool2_full_topk": ARCH.replace(attention_type="full"),
}


def make_inputs(arch):
    """As test_gpu_train_head.test_head_backward_matches_oracle_autograd: generator seed 5; feats, hooks,
    text in that order, then the targets over all T0 classes with rows 0-2 ignored."""
    L_ = arch.grid ** 2 + 1
    gen = torch.Generator().manual_seed(5)
    feats = torch.randn(B, L_, arch.embed_dim, generator=gen, dtype=torch.float64)
    hooks = [torch.randn(B, L_, arch.vision_width, generator=gen, dtype=torch.float64) for _ in range(2)]
    text = F.normalize(torch.randn(T0, arch.embed_dim, generator=gen, dtype=torch.float64), dim=-1)
    R = 4 * arch.grid
    targets = torch.randint(0, T0, (B, R, R), generator=gen, dtype=torch.int32)
    targets[:, :3] = 255
    return feats, hooks, text, targets


def class_maxima(feats, text):
    """The top-k key (model.py:695) in float64: per image and class, the max over the pixels of the cost."""
    return (F.normalize(feats[:, 1:, :], dim=-1) @ F.normalize(text, dim=-1).T).max(dim=1)[0]


def assert_selection_is_separated(cm, targets=None):
    """gap >= 1e-3 per image, the images' sets differ and overlap (and, with targets, ground truth in an
    unselected class occurs); returns the sets."""
    sets = []
    for b in range(cm.shape[0]):
        srt = cm[b].sort(descending=True)[0]
        gap = (srt[PAD_LEN - 1] - srt[PAD_LEN]).item()
        assert gap >= 1e-3, (b, gap)
        sets.append(set(cm[b].topk(PAD_LEN)[1].tolist()))
    assert sets[0] != sets[1] and sets[0] & sets[1]
    if targets is not None:
        for b, s in enumerate(sets):
            assert (set(targets[b].unique().tolist()) - {255}) - s, b
    return sets


def device_head(arch, sd, keys, feats, hooks, text, targets):
    L_ = arch.grid ** 2 + 1
    P = {k: v.detach().cuda().requires_grad_(k in keys) for k, v in sd.items()}
    text_d = text.detach().float().cuda().requires_grad_(True)
    logits = head_train_forward(arch, P, feats.reshape(B * L_, -1).float().cuda(),
                                [h.reshape(B * L_, -1).float().cuda() for h in hooks], text_d)
    sel = training.last_topk
    loss = ops.BCEOneHotLoss.apply(logits, targets.cuda(), 255)
    loss.backward()
    grads = {k: P[k].grad for k in keys}
    grads["text"] = text_d.grad
    return logits, sel, loss, grads


@pytest.mark.parametrize("case", list(CASES))
def test_topk_head_backward_matches_oracle_autograd(case):
    arch = CASES[case]
    sd = synthesize_state_dict(arch, seed=0)
    keys = head_keys(sd)
    feats, hooks, text, targets = make_inputs(arch)
    sets = assert_selection_is_separated(class_maxima(feats, text), targets)

    # reference: fp64 autograd through the oracle (and the same graph in torch fp32, the noise floor)
    ref_grads = {}
    for dt, store in ((torch.float64, ref_grads), (torch.float32, {})):
        sdr = {k: v.detach().clone().to(dt).requires_grad_(k in keys) for k, v in sd.items()}
        tr = text.detach().clone().to(dt).requires_grad_(True)
        with default_dtype(dt):
            lg = ref_head(arch, sdr, feats.to(dt), [h.permute(1, 0, 2).to(dt) for h in hooks], tr)
            l_ = ref_loss(lg, targets)
        l_.backward()
        store.update({k: sdr[k].grad for k in keys})
        store["text"] = tr.grad
        if dt == torch.float64:
            ref_logits, rl = lg.detach(), l_
        else:
            ref32 = store
    R = 4 * arch.grid
    off_ref = (ref_logits.flatten(2) == -100.0).all(dim=2)                     # (B, T0)
    assert [set(torch.nonzero(~off_ref[b]).flatten().tolist()) for b in range(B)] == sets

    logits, sel, loss, grads = device_head(arch, sd, keys, feats, hooks, text, targets)
    assert logits.shape == (B, T0, R, R) and logits.requires_grad
    assert sel.shape == (B, PAD_LEN) and sel.dtype == torch.int32 and sel.is_cuda
    assert [set(s.tolist()) for s in sel.cpu()] == sets                       # the oracle's own top-k, as sets
    got = logits.detach().cpu().double()
    off = off_ref[..., None, None].expand_as(got)
    assert bool((got[off] == -100.0).all())                                   # unselected planes: exactly -100
    err = (got - ref_logits)[~off].abs().max().item()
    print(f"{case}: logits max abs err {err:.3e}; loss hip {loss.item()!r} ref {rl.item()!r}")
    assert err < 1e-4
    assert abs(loss.item() - rl.item()) <= 1e-5 * abs(rl.item())
    # the padding tokens are off the graph (T == pad_len downstream): no gradient, here as in the reference
    pads = [k for k in keys if k.endswith(("padding_tokens", "padding_guidance"))]
    assert pads and all(ref_grads[k] is None for k in pads)
    assert all(grads[k] is None or not grads[k].abs().max().item() for k in pads)
    rows = []
    try:
        compare_grads(grads, ref_grads, keys + ["text"], ref32=ref32, report=rows)
    finally:
        _write_report(case, rows)
        print(f"{case}: worst gradients (rel err hip, torch fp32, key): {rows[:3]}; text: "
              f"{[r for r in rows if r[2] == 'text']}")


def test_topk_head_backward_is_deterministic():
    """Two forward + backward runs give bit-identical gradients (no atomics, fixed-order sums)."""
    arch = CASES["tiny_pool2_topk"]
    sd = synthesize_state_dict(arch, seed=0)
    keys = head_keys(sd)
    feats, hooks, text, targets = make_inputs(arch)
    assert_selection_is_separated(class_maxima(feats, text))
    runs = [device_head(arch, sd, keys, feats, hooks, text, targets) for _ in range(2)]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][0], runs[1][0])
    for k, g0 in runs[0][3].items():
        g1 = runs[1][3][k]
        assert (g0 is None and g1 is None) or torch.equal(g0, g1), k


@pytest.fixture(scope="module")
def golden_step():
    """One training step of the whole model on the golden's batch: (golden, model, loss, batch, targets)."""
    g = load_golden()
    for b in range(B):           # the fixture's own preconditions (tests/test_train_topk_cpu.py checks the rest)
        assert g["gap"][b] >= 1e-3
    cfg = tiny_cfg(**{"MODEL.SEM_SEG_HEAD.POOLING_SIZES": "[2,2]"})
    model = build_model(cfg).cuda()
    model.sem_seg_head.predictor.set_class_tokens(torch.from_numpy(g["tokens"]))
    model.arch = model.arch.replace(pad_len=int(g["pad_len"]))
    model._engine = None
    ims = [torch.from_numpy(g["image0"]).float(), torch.from_numpy(g["image1"]).float()]
    tg = torch.from_numpy(g["targets"]).long()
    batch = [{"image": ims[i], "sem_seg": tg[i]} for i in range(B)]
    model.train()
    loss = model(batch)["loss_sem_seg"]
    sel = training.last_topk.cpu()
    loss.backward()
    return g, model, loss, sel, batch, tg


def test_topk_train_step_matches_reference_gradients(golden_step):
    """As test_gpu_train_head.test_catseg_train_step_matches_reference_gradients, on 31 classes with
    pad_len 24: loss 1e-5, sampled gradients max(1e-4, 8 x the reference graph's own float32 error), and
    the device's selection equal to the reference's as sets."""
    g, model, loss, sel, _, _ = golden_step
    assert [set(s.tolist()) for s in sel] == [set(c.tolist()) for c in g["classes"]]
    l64 = float(g["loss64"])
    print(f"train step: loss hip {loss.item()!r} reference {l64!r}")
    assert abs(loss.item() - l64) <= 1e-5 * abs(l64), (loss.item(), l64)
    named = dict(model.named_parameters())
    names = [str(k) for k in g["names"]]
    assert {k for k, p in named.items() if p.requires_grad} == set(names) | {str(k) for k in g["none"]}
    rows = []
    try:
        for k in names:
            mx, e32 = (float(v) for v in g["m_" + k])
            got = named[k].grad.detach().double().cpu().reshape(-1)
            if ".swin_block." in k and k.endswith("attn.k.bias"):
                scale = float(g["m_" + k[:-len("bias")] + "weight"][0])
                assert got.abs().max().item() <= 1e-5 * scale, k
                continue
            if mx == 0.0:                 # the dense block's dead q / k projections
                assert got.abs().max().item() == 0.0, k
                continue
            idx = torch.from_numpy(g["i_" + k])
            err = max((got[idx] - torch.from_numpy(g["g_" + k])).abs().max().item() / mx,
                      abs(got.abs().max().item() - mx) / mx)
            rows.append((err, e32, k))
            assert err <= max(TOL, 8 * e32), f"{k}: {err:.3e} (reference fp32 {e32:.3e})"
    finally:
        _write_report("reference_modules_train_step_topk", sorted(rows, reverse=True))
        print("train step: worst gradients", sorted(rows, reverse=True)[:3])
    for k in (str(k) for k in g["none"]):           # off the graph in the reference: none or zero here
        gr = named[k].grad
        assert gr is None or not gr.abs().max().item(), k


def test_topk_training_loss_equals_the_eval_path_loss(golden_step):
    """The training loss equals the reference loss of train_engine.head_logits (the fp32 eval top-k path,
    pinned by the e2e_tiny_topk goldens) on the same batch: same pattern as
    test_gpu_training_loss.test_catseg_training_forward_loss."""
    g, model, loss, sel, batch, tg = golden_step
    eng = model.train_engine
    with torch.no_grad():
        eng.set_text(eng.encode_text(torch.from_numpy(g["tokens"])))
        raw, sizes_dev, _ = model._batch(eng, [b["image"] for b in batch])
        logits = eng.head_logits(raw, sizes_dev).cpu()
    assert logits.shape[1] == T0
    assert [set(s.tolist()) for s in eng.last_topk.cpu()] == [set(s.tolist()) for s in sel]
    ref = reference_loss(logits, tg.int(), 255)
    got = loss.item()
    print(f"training loss {got!r} vs the eval path's logits' loss {ref!r}")
    assert abs(got - ref) <= 1e-5 * abs(ref) + 1e-6, (got, ref)
