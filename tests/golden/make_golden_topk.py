"""Generate tests/golden/train_tiny_topk.npz (+ train_tiny_topk_images.npz): the training step of
make_golden.train_case with MORE classes than pad_len (T0 = 31 > pad_len = 24), i.e. the per-image
top-k class selection of Aggregator.forward (model.py:691-725) in training mode, through the
reference's own model_vpt.CLIP and Aggregator in float64 and float32.  Build container only, as
make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_topk.py

Beside train_case's fields the fixture states its own preconditions:
  pad_len           24
  corr_max (2, 31)  make_golden.ref_corr_max: the float32 top-k key (per-image class maxima of the cost
                    volume); corr_max64 the same from the float64 modules
  classes (2, 24)   the selected class ids per image (ascending), equal as sets in float32 and float64
  gap (2,)          the 24th minus the 25th largest class maximum per image (the smaller of the two runs)
The generator fails unless every gap is >= 1e-3 (about 6000 x the float32-vs-float64 deviation of the
class maxima, 1.5e-7: below it a different fp32 summation order could select another set and the
gradient comparison would test nothing), the float32 and float64 runs select the same sets, the two
images' sets differ but overlap, and each image has ground-truth pixels of an unselected class.

The seed (5) is not the one of train_tiny_pool2.npz, so the two images cannot be shared with it; they
are incompressible (0.9 MB) and go to train_tiny_topk_images.npz, which keeps both files under the
1 MiB limit for a committed file.
"""
import os

import numpy as np
import torch
import torch.nn as nn

import make_golden as M

torch.set_num_threads(8)
NAME = "train_tiny_topk"
PAD_LEN, T0, SEED, MIN_GAP = 24, 31, 5, 1e-3
ARCH = M.TINY.replace(pooling_size=(2, 2), pad_len=PAD_LEN)


# model.py:722 builds the -100 volume with torch.full in the DEFAULT dtype and scatter_ refuses a source
# of another one: the float64 run needs the default dtype to be its own while the Aggregator runs (the
# float32 run is untouched: the default stays float32 there)
_agg_forward = M.agg_mod.Aggregator.forward


def _forward_in_input_dtype(self, img_feats, *args, **kw):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(img_feats.dtype)
    try:
        return _agg_forward(self, img_feats, *args, **kw)
    finally:
        torch.set_default_dtype(prev)


M.agg_mod.Aggregator.forward = _forward_in_input_dtype
M.train_case(NAME, ARCH, T0, seed=SEED)
path = os.path.join(M.HERE, NAME + ".npz")
new = dict(np.load(path))

# the top-k key of the same inputs from the reference modules, float32 and float64
sd = M.synthesize_state_dict(ARCH, seed=0)
toks = new["tokens"].astype(np.int64)
ims = [torch.from_numpy(new["image0"]).float(), torch.from_numpy(new["image1"]).float()]
clip_images = M.glue_preprocess(ARCH, ims)
cmax = {}
ln_forward = M.model_vpt.LayerNorm.forward         # see make_golden.train_case: float64 end to end
for dt in (torch.float32, torch.float64):
    M.model_vpt.LayerNorm.forward = nn.LayerNorm.forward if dt == torch.float64 else ln_forward
    clip, agg, _, _ = M.build_reference(ARCH, sd, pad_len=PAD_LEN)
    clip, agg = clip.to(dt), agg.to(dt)
    cmax[dt] = M.ref_corr_max(ARCH, clip, agg, clip_images.to(dt), M.ref_text(clip, toks)).double()
M.model_vpt.LayerNorm.forward = ln_forward
assert cmax[torch.float32].shape == (2, T0)

sel = {dt: [set(c.topk(PAD_LEN)[1].tolist()) for c in cm] for dt, cm in cmax.items()}
assert sel[torch.float32] == sel[torch.float64], "float32 and float64 select different class sets"
gap = np.array([min((cm[b].sort(descending=True)[0][PAD_LEN - 1] - cm[b].sort(descending=True)[0][PAD_LEN]).item()
                    for cm in cmax.values()) for b in range(2)])
assert (gap >= MIN_GAP).all(), f"top-k gap below {MIN_GAP}: {gap} (another seed is needed)"
s0, s1 = sel[torch.float64]
assert s0 != s1 and s0 & s1, "the two images' selections must differ and overlap"
targets = new["targets"]
for b, s in enumerate((s0, s1)):
    gt = set(np.unique(targets[b]).tolist()) - {255}
    assert gt - s, f"image {b}: every ground-truth class was selected"

new["pad_len"] = np.array(PAD_LEN)
new["classes"] = np.array([sorted(s0), sorted(s1)], dtype=np.int32)
new["corr_max"] = cmax[torch.float32].float().numpy()
new["corr_max64"] = cmax[torch.float64].numpy()
new["gap"] = gap
images = {k: new.pop(k) for k in ("image0", "image1")}
np.savez_compressed(path, **new)
ipath = os.path.join(M.HERE, NAME + "_images.npz")
np.savez_compressed(ipath, **images)
for p in (path, ipath):
    size = os.path.getsize(p)
    print("rewrote", p, size, "bytes")
    assert size <= (1 << 20), f"{p}: over the 1 MiB limit for a committed file"
print("gap", gap, "sets differ in", len(s0 - s1), "classes")
