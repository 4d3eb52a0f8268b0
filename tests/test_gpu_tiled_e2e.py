"""MODEL.CATSEG_HIP.TILED at the drop-in boundary: CATSeg.forward cuts every image into tiles, runs them
through the network as images of their own and merges them on the device (catseg_tile_crops ->
head_logits -> catseg_tiled_merge), at input resolution.

The reference result is composed from a non-tiled model with the same (synthetic) weights: forward_logits on
the same groups of tile crops in the same order, then per tile catseg_postprocess and a torch accumulation.
Tile width 64 runs catseg_postprocess banded, so the two must be EQUAL."""
import os

import numpy as np
import pytest
import torch

from cat_seg import build_model, ops, tiling
from cat_seg.evaluation import SemSegEvaluator

from conftest import GOLDEN
from test_boundary_cpu import tiny_cfg

pytestmark = pytest.mark.gpu

_CACHE = {}
H, W, TILE, STRIDE, BATCH = 150, 200, 64, 32, 5


def _tokens():
    if "tokens" not in _CACHE:
        _CACHE["tokens"] = dict(np.load(os.path.join(GOLDEN, "e2e_tiny_eval.npz")))["tokens"]
    return _CACHE["tokens"]


def _image(h=H, w=W, seed=5):
    return (torch.rand((3, h, w), generator=torch.Generator().manual_seed(seed)) * 255).to(torch.uint8)


def _model(**over):
    key = tuple(sorted(over.items()))
    if key not in _CACHE:
        m = build_model(tiny_cfg(**over)).cuda().eval()
        m.sem_seg_head.predictor.set_class_tokens(_tokens())
        _CACHE[key] = m
    return _CACHE[key]


def _tiled(output="probs", batch=BATCH, tile=TILE, stride=STRIDE, **over):
    return _model(**{"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": str(tile),
                     "MODEL.CATSEG_HIP.TILED.STRIDE": str(stride), "MODEL.CATSEG_HIP.TILED.BATCH": str(batch),
                     "MODEL.CATSEG_HIP.OUTPUT": output, **over})


def _banded(ch, cw, th, tw):
    """launch_post's rule (misc.hip), as tests/test_gpu_postprocess_tta.py restates it"""
    rows = 48 * ch // th + 3
    return tw % 4 == 0 and rows * cw * 4 <= 64 * 1024


def _composition():
    """The tiled result composed from the plain model: the tiles in row-major groups of BATCH through
    forward_logits, per tile ops.postprocess to (th, tw), fp32 adds in tile order, times fp32 1 / count."""
    if "composition" not in _CACHE:
        plain = _model(**{"MODEL.CATSEG_HIP.GRAPH": "False"})
        img = _image()
        g = tiling.tile_grid(H, W, TILE, STRIDE)
        org = [(oy, ox) for oy in g.oys for ox in g.oxs]
        assert len(org) == 24 and len(org) % BATCH != 0
        acc = cnt = None
        for i in range(0, len(org), BATCH):
            grp = org[i:i + BATCH]
            logits, crops = plain.forward_logits([{"image": img[:, oy:oy + g.th, ox:ox + g.tw]} for oy, ox in grp])
            assert all(_banded(ch, cw, g.th, g.tw) for ch, cw in crops)      # exact equality is owed
            if acc is None:
                acc = torch.zeros(logits.shape[1], H, W, device="cuda")
                cnt = torch.zeros(H, W, device="cuda")
            for j, (oy, ox) in enumerate(grp):
                out = torch.empty(1, logits.shape[1], g.th, g.tw, device="cuda")
                ops.postprocess(logits[j:j + 1].contiguous(), out, crop=crops[j])
                acc[:, oy:oy + g.th, ox:ox + g.tw] += out[0]
                cnt[oy:oy + g.th, ox:ox + g.tw] += 1
        rk = torch.tensor(1.0, dtype=torch.float32) / cnt.cpu()
        _CACHE["composition"] = acc.cpu() * rk
    return _CACHE["composition"]


def _tiled_probs():
    if "tiled_probs" not in _CACHE:
        out = _tiled()([{"image": _image()}])[0]
        assert set(out) == {"sem_seg"} and out["sem_seg"].is_cuda
        _CACHE["tiled_probs"] = out["sem_seg"].cpu()
    return _CACHE["tiled_probs"]


def test_probs_equal_the_composition():
    ref = _composition()
    got = _tiled_probs()
    assert got.shape == ref.shape == (int(_tokens().shape[0]), H, W)
    assert torch.equal(got, ref)
    assert 0 < (got.argmax(0) > 0).float().mean() < 1


def test_labels_equal_the_composition_and_the_argmax_of_probs():
    ref = _composition()
    out = _tiled("labels")([{"image": _image()}])[0]
    assert set(out) == {"sem_seg_labels", "sem_seg_score"}
    lab, sc = out["sem_seg_labels"], out["sem_seg_score"]
    assert lab.dtype == torch.int32 and sc.dtype == torch.float32 and lab.is_cuda and lab.shape == sc.shape == (H, W)
    assert torch.equal(lab.cpu(), ref.argmax(0).int()) and torch.equal(sc.cpu(), ref.max(0).values)
    probs = _tiled_probs()
    assert torch.equal(lab.cpu(), probs.argmax(0).int()) and torch.equal(sc.cpu(), probs.max(0).values)


def test_batch_1_equals_batch_5():
    one = _tiled(batch=1)([{"image": _image()}])[0]["sem_seg"].cpu()
    assert torch.equal(one, _tiled_probs())


def test_image_within_one_tile_matches_the_plain_model():
    """60 x 80 under the default 384 tile: one tile, the plain path's geometry.  Labels equal the plain
    model's except where its top two probabilities are within 1e-5, on at most 0.5 % of the pixels."""
    img = _image(60, 80, seed=9)
    assert tiling.tile_grid(60, 80, 384, 256)[2:4] == (60, 80)
    lab = _tiled("labels", batch=8, tile=384, stride=256)([{"image": img}])[0]["sem_seg_labels"].cpu()
    plain = _model(**{"MODEL.CATSEG_HIP.OUTPUT": "labels"})([{"image": img}])[0]["sem_seg_labels"].cpu()
    probs = _model()([{"image": img}])[0]["sem_seg"].cpu()
    top2 = probs.topk(2, dim=0).values
    close = (top2[0] - top2[1]) <= 1e-5
    assert lab.shape == plain.shape == (60, 80)
    assert close.float().mean().item() <= 0.005
    assert torch.equal(lab[~close], plain[~close])


def test_every_image_gets_its_own_map():
    a, b = _image(), _image(70, 100, seed=6)
    outs = _tiled()([{"image": a}, {"image": b, "height": 70, "width": 100}])
    assert [tuple(o["sem_seg"].shape[1:]) for o in outs] == [(H, W), (70, 100)]
    assert torch.equal(outs[0]["sem_seg"].cpu(), _tiled_probs())
    alone = _tiled()([{"image": b}])[0]["sem_seg"]
    assert torch.equal(outs[1]["sem_seg"], alone)
    ref_mode = _tiled(**{"MODEL.CATSEG_HIP.RETURN_ALL_IMAGES": "False"})([{"image": b}, {"image": a}])
    assert len(ref_mode) == 1 and torch.equal(ref_mode[0]["sem_seg"], alone)


def test_errors():
    m = _tiled()
    with pytest.raises(ValueError, match="MIN_SIZE_TEST 0"):
        m([{"image": _image(), "height": H * 2, "width": W * 2}])
    with pytest.raises(RuntimeError, match="TILED"):
        m.forward_logits([{"image": _image()}])


def test_evaluator_bins_the_tiled_label_map():
    T = int(_tokens().shape[0])
    gen = torch.Generator().manual_seed(1)
    gt = torch.randint(0, T, (H, W), generator=gen).int()
    gt[torch.rand(H, W, generator=gen) < 0.1] = 255
    inputs = [{"image": _image(), "sem_seg_gt": gt.numpy(), "file_name": "im0.png"}]
    outputs = _tiled("labels")(inputs)
    ev = SemSegEvaluator(None, distributed=False, output_dir=None, class_names=[f"c{i}" for i in range(T)],
                         ignore_label=255)
    ev.process(inputs, outputs)
    lab = outputs[0]["sem_seg_labels"].cpu().long()
    g = torch.where(gt == 255, torch.full_like(gt, T), gt).long()
    want = torch.bincount(((T + 1) * lab + g).reshape(-1), minlength=(T + 1) ** 2).reshape(T + 1, T + 1)
    assert int(want.sum()) == H * W
    assert np.array_equal(ev.confusion_matrix(), want.numpy())
