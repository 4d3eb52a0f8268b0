"""Generate tests/golden/train_tiny_vpt.npz: the training step of make_golden.train_case with visual
prompt tuning and CLIP_FINETUNE "prompt" (the reference's own model_vpt.CLIP with prompt_depth 4 /
prompt_length 3 and Aggregator in float64 and float32).  Build container only, as make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_vpt.py

make_golden.train_case hard-codes the requires_grad rule of CLIP_FINETUNE "attention", so its loop is
repeated here with the "prompt" rule (cat_seg_model.py:57-75: inside `transformer` only the parameters
whose name contains "prompt" train; the text transformer has none).  Tokens, images and targets are
drawn as for train_tiny_pool2.npz (same seed, same T): the two images (incompressible, 0.9 MB) are
checked against that fixture and left out of this one, which keeps it under the 1 MiB limit for a
committed file; the tests read them from train_tiny_pool2.npz.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import make_golden as M

torch.set_num_threads(8)
NAME = "train_tiny_vpt"
ARCH = M.TINY.replace(prompt_depth=4, prompt_length=3, pooling_size=(2, 2))
T, SEED, N_SUB = 9, 3, 256


def prompt_rule(name):
    """cat_seg_model.py:57-75, CLIP_FINETUNE "prompt"."""
    return "transformer" in name and "prompt" in name


def train_case_prompt(name, arch):
    sd = M.synthesize_state_dict(arch, seed=0)
    gen = torch.Generator().manual_seed(SEED)
    toks = torch.zeros(T, arch.context_length, dtype=torch.long)
    toks[:, 0] = 1
    toks[:, 1:4] = torch.randint(2, 400, (T, 3), generator=gen)
    toks[:, 4] = 511                                   # EOT = the argmax id
    ims = [torch.randint(0, 256, (3, 384, 384), generator=gen).float() for _ in range(2)]
    sems = [torch.randint(0, T, (384, 384), generator=gen) for _ in range(2)]
    sems[0][:20] = 255
    targets = torch.stack(sems)
    grads, losses = {}, {}
    ln_forward = M.model_vpt.LayerNorm.forward         # see make_golden.train_case: float64 end to end
    for dt in (torch.float64, torch.float32):
        M.model_vpt.LayerNorm.forward = nn.LayerNorm.forward if dt == torch.float64 else ln_forward
        clip, agg, up1, up2 = M.build_reference(arch, sd, pad_len=arch.pad_len)
        clip, agg, up1, up2 = clip.to(dt), agg.to(dt), up1.to(dt), up2.to(dt)
        for n, p in clip.named_parameters():
            p.requires_grad_(prompt_rule(n))
        for m in (clip, agg, up1, up2):
            m.train()
        text = clip.encode_text(toks)
        text = (text / text.norm(dim=-1, keepdim=True)).unsqueeze(1)
        layers = []
        hs = [clip.visual.transformer.resblocks[l].register_forward_hook(lambda m, i, o: layers.append(o))
              for l in arch.hook_layers]
        clip_images = M.glue_preprocess(arch, ims).to(dt)
        feats = clip.encode_image(clip_images, dense=True)
        for h in hs:
            h.remove()
        g = arch.grid
        B = feats.shape[0]
        res3 = feats[:, 1:, :].reshape(B, g, g, -1).permute(0, 3, 1, 2)
        res4 = up1(layers[0][1:].permute(1, 2, 0).reshape(B, -1, g, g))
        res5 = up2(layers[1][1:].permute(1, 2, 0).reshape(B, -1, g, g))
        out = agg(res3, text.repeat(B, 1, 1, 1), [res3, res4, res5])
        out = F.interpolate(out, size=targets.shape[-2:], mode="bilinear", align_corners=False)
        mask = targets != 255
        out = out.permute(0, 2, 3, 1)
        tg = torch.zeros(out.shape, dtype=dt)
        tg[mask] = F.one_hot(targets[mask], num_classes=out.shape[-1]).to(dt)
        loss = F.binary_cross_entropy_with_logits(out, tg)
        loss.backward()
        losses[dt] = loss.item()
        named = {M.CLIP_P + n: p for n, p in clip.named_parameters()}
        named.update({M.AGG_P + n: p for n, p in agg.named_parameters()})
        named.update({"upsample1." + n: p for n, p in up1.named_parameters()})
        named.update({"upsample2." + n: p for n, p in up2.named_parameters()})
        grads[dt] = {k: (None if p.grad is None else p.grad.detach().double().reshape(-1))
                     for k, p in named.items() if p.requires_grad}
    M.model_vpt.LayerNorm.forward = ln_forward
    kw = dict(tokens=toks, targets=targets.to(torch.int16), loss64=losses[torch.float64],
              loss32=losses[torch.float32], image0=ims[0].to(torch.uint8), image1=ims[1].to(torch.uint8))
    names, none = [], []
    for k, g64 in grads[torch.float64].items():
        if g64 is None:
            none.append(k)
            continue
        n = g64.numel()
        step = max(1, n // N_SUB)
        idx = torch.arange(0, n, step)[:N_SUB]
        g32 = grads[torch.float32][k]
        mx = g64.abs().max().item()
        names.append(k)
        kw["g_" + k] = g64[idx].numpy()
        kw["i_" + k] = idx.numpy().astype(np.int64)
        kw["m_" + k] = np.array([mx, (g32 - g64).abs().max().item() / (mx + 1e-300)])
    # the prompt tokens are small ((depth, length, W)) and the point of this fixture: kept whole too
    pk = M.CLIP_P + "visual.transformer.prompt_tokens"
    kw["prompt_grad"] = grads[torch.float64][pk].reshape(arch.prompt_depth, arch.prompt_length, -1).numpy()
    kw["names"] = np.array(names)
    kw["none"] = np.array(none)
    M.save(name, **kw)


train_case_prompt(NAME, ARCH)
path = os.path.join(M.HERE, NAME + ".npz")
new, base = dict(np.load(path)), np.load(os.path.join(M.HERE, "train_tiny_pool2.npz"))
for k in ("image0", "image1"):
    assert np.array_equal(new.pop(k), base[k]), k
assert np.array_equal(new["tokens"], base["tokens"]) and np.array_equal(new["targets"], base["targets"])
np.savez_compressed(path, **new)
print("rewrote", path, os.path.getsize(path), "bytes")
