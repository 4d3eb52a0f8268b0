"""Generate tests/golden/train_tiny_full_pool2.npz: the training step of make_golden.train_case with
ATTENTION_TYPE "full" (the reference's own model_vpt.CLIP and Aggregator(attention_type="full") in
float64 and float32).  Build container only, as make_golden.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_full.py

train_case draws the same tokens, images and targets as for train_tiny_pool2.npz (same seed, same T):
the two images (incompressible, 0.9 MB) are checked against that fixture and left out of this one,
which keeps it under the 1 MiB limit for a committed file; the test reads them from train_tiny_pool2.npz.
"""
import os

import numpy as np
import torch

import make_golden as M

torch.set_num_threads(8)
NAME = "train_tiny_full_pool2"
M.train_case(NAME, M.TINY.replace(attention_type="full", pooling_size=(2, 2)), 9)
path = os.path.join(M.HERE, NAME + ".npz")
new, base = dict(np.load(path)), np.load(os.path.join(M.HERE, "train_tiny_pool2.npz"))
for k in ("image0", "image1"):
    assert np.array_equal(new.pop(k), base[k]), k
assert np.array_equal(new["tokens"], base["tokens"]) and np.array_equal(new["targets"], base["targets"])
np.savez_compressed(path, **new)
print("rewrote", path, os.path.getsize(path), "bytes")
