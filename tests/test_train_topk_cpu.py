"""Training with more classes than pad_len (the per-image top-k selection of model.py:691-725), the
parts that need no GPU: the four catseg_class_* entries are declared, mirrored and refuse bad arguments
on the host before any launch; the reference golden tests/golden/train_tiny_topk.npz
(tests/golden/make_golden_topk.py: the reference's own CLIP + Aggregator with pad_len 24 on 31 classes)
states the preconditions that make its selection reproducible in fp32; and the oracle's differentiable
top-k branch (oracle/catseg_oracle.py aggregator) reproduces that golden's loss and gradients in float64,
which pins the reference graph of tests/test_gpu_train_topk.py."""
import contextlib
import os
import re

import numpy as np
import torch

from cat_seg import _lib as L
from cat_seg.arch import TINY
from cat_seg.weights import synthesize_state_dict
from oracle import catseg_oracle as O

from conftest import ROOT
from test_gpu_train_head import ref_head, ref_loss

NEW = ("catseg_class_inverse", "catseg_class_rows_reduce", "catseg_class_planes_gather",
       "catseg_class_planes_scatter")
PAD_LEN, T0 = 24, 31
ARCH = TINY.replace(pooling_size=(2, 2), pad_len=PAD_LEN)


@contextlib.contextmanager
def default_dtype(dt):
    """The oracle's -100 volume (as the reference's, model.py:722) is torch.full in the default dtype and
    scatter_ refuses a source of another one: a float64 run of the top-k branch needs the default dtype
    to be float64 while the graph is built."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(prev)


def load_golden():
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "train_tiny_topk.npz")))
    g.update(np.load(os.path.join(ROOT, "tests", "golden", "train_tiny_topk_images.npz")))
    return g


def test_header_and_lib_carry_the_class_selection_symbols():
    hdr = open(os.path.join(ROOT, "include", "catseg_hip_train.h")).read()
    declared = set(re.findall(r"\b(catseg_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for s in NEW:
        assert s in declared and s in L.EXPORTED and hasattr(lib, s), s
    assert "model.py:722-723" in hdr and "model.py:691-725" in hdr


def _calls(lib):
    """name -> call(B, k, T0, n, ptrs) with n the row / plane length and ptrs the entry's pointers in order."""
    return {
        "catseg_class_inverse": (2, lambda B, k, T, n, p: lib.catseg_class_inverse(p[0], B, k, T, p[1], None)),
        "catseg_class_rows_reduce": (3, lambda B, k, T, n, p: lib.catseg_class_rows_reduce(
            p[0], n, p[1], B, k, T, n, p[2], n, 0, None)),
        "catseg_class_planes_gather": (3, lambda B, k, T, n, p: lib.catseg_class_planes_gather(
            p[0], n, T * n, p[1], B, k, T, n, p[2], n, k * n, None)),
        "catseg_class_planes_scatter": (3, lambda B, k, T, n, p: lib.catseg_class_planes_scatter(
            p[0], n, k * n, p[1], B, k, T, n, -100.0, p[2], n, T * n, None)),
    }


def test_argument_checks_without_gpu():
    """The host-side checks refuse bad arguments before any launch (no device needed): the pointers are
    never dereferenced."""
    lib = L.load()
    for name, (nptr, fn) in _calls(lib).items():
        ptrs = [4096 * (i + 1) * 1024 for i in range(nptr)]        # aligned, disjoint, never dereferenced
        for i in range(nptr):                                       # every pointer null in turn
            bad = list(ptrs)
            bad[i] = None
            assert fn(2, 5, 13, 16, bad) == -1, (name, i)
            assert b"null" in lib.catseg_last_error(), (name, lib.catseg_last_error())
        for B, k, T, n, word in ((2, 14, 13, 16, b"k <= T0"), (1, 256, 2049, 16, b"2048"), (1, 2049, 2049, 16, b"2048"),
                                 (0, 5, 13, 16, b"non-positive"), (-1, 5, 13, 16, b"non-positive"),
                                 (2, 0, 13, 16, b"non-positive"), (2, -3, 13, 16, b"non-positive"),
                                 (2, 5, 0, 16, b"non-positive"), (2, 5, -13, 16, b"non-positive")):
            assert fn(B, k, T, n, ptrs) == -1, (name, B, k, T, n)
            assert word in lib.catseg_last_error(), (name, B, k, T, lib.catseg_last_error())
        if nptr == 3:                                               # the row / plane length
            for n in (0, -4):
                assert fn(2, 5, 13, n, ptrs) == -1, (name, n)


def test_stride_and_overlap_checks_without_gpu():
    lib = L.load()
    p = 1 << 20
    q = 1 << 24
    # a plane stride below the plane length, an image stride below the image's planes
    assert lib.catseg_class_planes_gather(p, 15, 13 * 16, q, 2, 5, 13, 16, 2 * q, 16, 5 * 16, None) == -1
    assert b"stride" in lib.catseg_last_error()
    assert lib.catseg_class_planes_scatter(p, 16, 4 * 16, q, 2, 5, 13, 16, -100.0, 2 * q, 16, 13 * 16, None) == -1
    assert b"stride" in lib.catseg_last_error()
    assert lib.catseg_class_rows_reduce(p, 15, q, 2, 5, 13, 16, 2 * q, 16, 0, None) == -1
    assert b"stride" in lib.catseg_last_error()
    # input and output ranges that overlap
    assert lib.catseg_class_planes_gather(p, 16, 13 * 16, q, 2, 5, 13, 16, p + 64, 16, 5 * 16, None) == -1
    assert b"overlap" in lib.catseg_last_error()
    assert lib.catseg_class_rows_reduce(p, 16, q, 2, 5, 13, 16, p + 64, 16, 0, None) == -1
    assert b"overlap" in lib.catseg_last_error()


def test_golden_states_its_preconditions():
    g = load_golden()
    assert int(g["pad_len"]) == PAD_LEN and g["tokens"].shape[0] == T0
    assert g["classes"].shape == (2, PAD_LEN) and g["corr_max"].shape == (2, T0) and g["gap"].shape == (2,)
    assert g["image0"].shape == g["image1"].shape == (3, 384, 384)
    assert (g["gap"] >= 1e-3).all(), g["gap"]
    sets = [set(c.tolist()) for c in g["classes"]]
    assert all(len(s) == PAD_LEN for s in sets)
    for key in ("corr_max", "corr_max64"):          # the float32 and the float64 run select the stored sets
        for b in range(2):
            cm = torch.from_numpy(g[key][b]).double()
            assert set(cm.topk(PAD_LEN)[1].tolist()) == sets[b], (key, b)
            srt = cm.sort(descending=True)[0]
            assert (srt[PAD_LEN - 1] - srt[PAD_LEN]).item() >= g["gap"][b] - 1e-12
    assert np.abs(g["corr_max"] - g["corr_max64"]).max() < 1e-5
    assert sets[0] != sets[1] and sets[0] & sets[1]
    for b in range(2):                               # ground truth in a class the image did not select
        gt = set(np.unique(g["targets"][b]).tolist()) - {255}
        assert gt - sets[b], b


def test_oracle_topk_training_gradients_match_reference_modules():
    g = load_golden()
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    names = [str(k) for k in g["names"]]
    sd = {k: v.double() for k, v in synthesize_state_dict(ARCH, seed=0).items()}
    for k in names:
        sd[k].requires_grad_(True)
    ims = [torch.from_numpy(g["image0"]).float(), torch.from_numpy(g["image1"]).float()]
    clip_ims, _ = O.preprocess(ARCH, ims)
    with default_dtype(torch.float64):
        feats, hooks = O.encode_image_dense(ARCH, sd, clip_ims.double())
        text = O.text_embeds(ARCH, sd, torch.from_numpy(g["tokens"]))[:, 0]
        logits = ref_head(ARCH, sd, feats, hooks, text)
        loss = ref_loss(logits, torch.from_numpy(g["targets"]).long())
    loss.backward()
    assert logits.shape[1] == T0
    for b in range(2):                               # the oracle selected the reference's sets
        off = (logits[b].detach().flatten(1) == -100.0).all(dim=1)
        assert set(torch.nonzero(~off).flatten().tolist()) == set(g["classes"][b].tolist()), b
    l64 = float(g["loss64"])
    assert abs(loss.item() - l64) <= 1e-10 * abs(l64), (loss.item(), l64)
    # the padding tokens are off the graph at T == pad_len, in the reference as in the oracle
    assert {k for k in g["none"]} >= {k for k in sd if k.endswith(("padding_tokens", "padding_guidance"))}
    worst = (0.0, "")
    for k in names:
        mx = float(g["m_" + k][0])
        if sd[k].grad is None:        # off the oracle's graph (the dense block's dead q / k): zero there
            assert mx == 0.0, k
            continue
        got = sd[k].grad.detach().reshape(-1)
        if mx == 0.0:
            assert got.abs().max().item() == 0.0, k
            continue
        idx = torch.from_numpy(g["i_" + k])
        scale = mx
        if ".swin_block." in k and k.endswith("attn.k.bias"):
            # zero in exact arithmetic: compare against the k weight's gradient scale
            scale = float(g["m_" + k[:-len("bias")] + "weight"][0])
        err = (got[idx] - torch.from_numpy(g["g_" + k])).abs().max().item() / scale
        worst = max(worst, (err, k))
    assert worst[0] <= 1e-9, worst
