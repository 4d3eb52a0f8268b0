"""Training the visual prompt tokens (CLIP_FINETUNE "prompt"), the parts that need no GPU.

tests/golden/train_tiny_vpt.npz holds the loss and the gradients of every trainable parameter of the
reference's own model_vpt.CLIP (prompt_depth 4, prompt_length 3) + Aggregator training step in float64
under the reference's "prompt" requires_grad rule (tests/golden/make_golden_train_vpt.py; inputs those
of train_tiny_pool2.npz, where the two images are kept).  Here: the build's requires_grad set and
optimizer groups, the oracle's float64 autograd pinned to that fixture (the GPU tests of
tests/test_gpu_train_vpt.py use the oracle as their reference), and the host side of the two
catseg_vpt_rows_* entry points (every call below returns from a failed check: no launch).
"""
import os

import numpy as np
import torch

from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg.arch import TINY
from cat_seg.optim import build_optimizer
from cat_seg.weights import CLIP, synthesize_state_dict
from oracle import catseg_oracle as O

from conftest import ROOT
from test_boundary_cpu import tiny_cfg
from test_gpu_train_head import ref_head, ref_loss

PROMPTS = CLIP + "visual.transformer.prompt_tokens"
VPT_ARCH = TINY.replace(prompt_depth=4, prompt_length=3, pooling_size=(2, 2))


def vpt_cfg(finetune="prompt", depth=4, length=3, **over):
    return tiny_cfg(**{"MODEL.SEM_SEG_HEAD.POOLING_SIZES": "[2,2]", "MODEL.SEM_SEG_HEAD.PROMPT_DEPTH": str(depth),
                       "MODEL.SEM_SEG_HEAD.PROMPT_LENGTH": str(length),
                       "MODEL.SEM_SEG_HEAD.CLIP_FINETUNE": finetune, **over})


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "train_tiny_vpt.npz"))


def test_prompt_mode_trains_what_the_reference_trains():
    g = golden()
    model = build_model(vpt_cfg())
    assert (model.arch.prompt_depth, model.arch.vpt, model.arch.vision_layers) == (4, 3, 4)
    trainable = {k for k, p in model.named_parameters() if p.requires_grad}
    assert trainable == {str(k) for k in g["names"]} | {str(k) for k in g["none"]}
    assert [k for k in trainable if k.startswith(CLIP)] == [PROMPTS]
    assert tuple(dict(model.named_parameters())[PROMPTS].shape) == (4, 3, VPT_ARCH.vision_width)


def test_prompt_tokens_optimizer_group():
    cfg = vpt_cfg(**{"SOLVER.BASE_LR": "0.002", "SOLVER.CLIP_MULTIPLIER": "0.25", "SOLVER.WEIGHT_DECAY": "0.03",
                     "SOLVER.WEIGHT_DECAY_NORM": "0.0"})
    model = build_model(cfg)
    p = dict(model.named_parameters())[PROMPTS]
    groups = [g for g in build_optimizer(cfg, model).param_groups if any(q is p for q in g["params"])]
    assert len(groups) == 1
    assert groups[0]["lr"] == 0.002 * 0.25 and groups[0]["weight_decay"] == 0.03


def test_last_layer_prompt_gradient_is_zero_in_the_reference():
    """The dense block is row-wise plus the CLS row and drops its prompt rows (model_vpt.py:219-240)."""
    pg = golden()["prompt_grad"]
    assert pg.shape == (4, 3, VPT_ARCH.vision_width)
    assert np.all(pg[3] == 0.0)
    assert all(np.abs(pg[i]).max() > 0.0 for i in range(3))


def test_oracle_prompt_training_gradients_match_reference_modules():
    """tests/test_oracle_train_golden.py's check with the prompt rows in the oracle's graph
    (oracle/catseg_oracle.py:116-127) and the "prompt" requires_grad rule: loss to 1e-10, every sampled
    gradient to 1e-9 of the parameter's largest, the whole prompt gradient too."""
    g = golden()
    base = np.load(os.path.join(ROOT, "tests", "golden", "train_tiny_pool2.npz"))
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    arch = VPT_ARCH
    names = [str(k) for k in g["names"]]
    sd = {k: v.double() for k, v in synthesize_state_dict(arch, seed=0).items()}
    for k in names:
        sd[k].requires_grad_(True)
    ims = [torch.from_numpy(base["image0"]).float(), torch.from_numpy(base["image1"]).float()]
    clip_ims, _ = O.preprocess(arch, ims)
    feats, hooks = O.encode_image_dense(arch, sd, clip_ims.double())
    with torch.no_grad():
        text = O.text_embeds(arch, sd, torch.from_numpy(g["tokens"]))[:, 0]
    loss = ref_loss(ref_head(arch, sd, feats, hooks, text), torch.from_numpy(g["targets"]).long())
    loss.backward()
    l64 = float(g["loss64"])
    assert abs(loss.item() - l64) <= 1e-10 * abs(l64), (loss.item(), l64)
    worst = (0.0, "")
    for k in names:
        mx = float(g["m_" + k][0])
        got = sd[k].grad.detach().reshape(-1)
        idx = torch.from_numpy(g["i_" + k])
        err = (got[idx] - torch.from_numpy(g["g_" + k])).abs().max().item()
        if ".swin_block." in k and k.endswith("attn.k.bias"):
            # zero in exact arithmetic: compare against the k weight's gradient scale
            err /= float(g["m_" + k[:-len("bias")] + "weight"][0])
        else:
            err /= mx
        worst = max(worst, (err, k))
    assert worst[0] <= 1e-9, worst
    pg = torch.from_numpy(g["prompt_grad"])
    got = sd[PROMPTS].grad
    assert (got - pg).abs().max().item() <= 1e-9 * pg.abs().max().item()
    assert got[3].abs().max().item() == 0.0


# ------------------------------------------------------------------ the entry points' host side
def test_vpt_entries_are_exported_and_bound():
    lib = L.load()
    for name in ("catseg_vpt_rows_forward", "catseg_vpt_rows_backward"):
        assert name in L.EXPORTED and hasattr(lib, name)
    assert lib.catseg_abi_version() == 1


def test_vpt_rows_forward_rejects_bad_arguments():
    fwd = L.load().catseg_vpt_rows_forward
    err = lambda: L.load().catseg_last_error().decode()  # noqa: E731
    S, D, PR = 1 << 20, 1 << 22, 1 << 24          # far-apart fake device addresses, never dereferenced
    ok = dict(src=S, ld_src=64, prompt=PR, ld_prompt=64, dst=D, ld_dst=64, B=2, L0=17, P=3, W=64, strip=0)

    def run(**kw):
        a = {**ok, **kw}
        return fwd(a["src"], a["ld_src"], a["prompt"], a["ld_prompt"], a["dst"], a["ld_dst"], a["B"], a["L0"], a["P"],
                   a["W"], a["strip"], None)

    for kw in (dict(dst=None), dict(B=0), dict(L0=0), dict(P=0), dict(W=0), dict(W=62), dict(ld_dst=60), dict(ld_dst=66),
               dict(dst=D + 4), dict(ld_src=32), dict(src=S + 8), dict(ld_prompt=65), dict(prompt=PR + 4)):
        assert run(**kw) == -1, kw
        assert "vpt_rows_forward" in err()
    assert run(src=None, prompt=None) == -1 and "nothing to write" in err()
    assert run(strip=1) == -1 and "strip" in err()                    # the strip takes no prompt
    assert run(strip=1, prompt=None, src=None) == -1
    # arguments must not overlap except in the in-place form (src == NULL)
    assert run(src=D) == -1 and "overlaps" in err()
    assert run(src=D + 2 * 19 * 64 * 4) == -1 and "overlaps" in err()   # src starts inside dst's last row
    assert run(prompt=D + 64 * 4) == -1 and "overlaps" in err()
    assert run(strip=1, prompt=None, src=D) == -1 and "overlaps" in err()


def test_vpt_rows_backward_rejects_bad_arguments():
    bwd = L.load().catseg_vpt_rows_backward
    err = lambda: L.load().catseg_last_error().decode()  # noqa: E731
    X, DP = 1 << 20, 1 << 24
    ok = dict(dx=X, ld_dx=64, dp=DP, ld_dp=64, B=2, L0=17, P=3, W=64, beta=0)

    def run(**kw):
        a = {**ok, **kw}
        return bwd(a["dx"], a["ld_dx"], a["dp"], a["ld_dp"], a["B"], a["L0"], a["P"], a["W"], a["beta"], None)

    for kw in (dict(dx=None), dict(B=0), dict(L0=0), dict(P=0), dict(W=30), dict(ld_dx=32), dict(ld_dx=70),
               dict(dx=X + 4), dict(ld_dp=60), dict(dp=DP + 8)):
        assert run(**kw) == -1, kw
        assert "vpt_rows_backward" in err()
    assert run(dp=X + 64 * 4) == -1 and "overlaps" in err()
