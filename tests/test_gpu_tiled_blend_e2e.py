"""MODEL.CATSEG_HIP.TILED.WINDOW / GLOBAL at the drop-in boundary: CATSeg.forward tapers every tile with the
pyramid window and averages the tiles' merge with the global view (the scene resized to the tile's extent
and run like a tile), in catseg_tiled_blend.

The reference result is composed from a non-tiled model's engine with the same (synthetic) weights: the same
tile groups through head_logits, the global canvas from ops.resize_bilinear, then the composition of
tests/test_gpu_tiled_blend.py (per tile catseg_postprocess, torch elementwise ops).  Tile width 64 and image
width 200 run catseg_postprocess banded, so the two must be EQUAL.  Model, image and geometry are those of
tests/test_gpu_tiled_e2e.py."""
import numpy as np
import pytest
import torch

from cat_seg import ops, tiling
from cat_seg.evaluation import SemSegEvaluator

from test_gpu_tiled_blend import _compose, _post
from test_gpu_tiled_e2e import BATCH, H, STRIDE, TILE, W, _banded, _image, _model, _tiled, _tokens

pytestmark = pytest.mark.gpu

_CACHE = {}
BLEND = {"MODEL.CATSEG_HIP.TILED.WINDOW": "pyramid", "MODEL.CATSEG_HIP.TILED.GLOBAL": "True"}


def _composition():
    """The blended result composed from the plain model's engine: the tiles in row-major groups of BATCH
    through catseg_tile_crops -> head_logits, the global view from ops.resize_bilinear on a tile's canvas
    through head_logits, per view ops.postprocess, then tests/test_gpu_tiled_blend.py::_compose."""
    if "composition" not in _CACHE:
        plain = _model(**{"MODEL.CATSEG_HIP.GRAPH": "False"})
        with torch.no_grad():
            eng = plain.engine
            plain.sem_seg_head.predictor.get_text_embeds()
            img = _image().cuda().float().contiguous()
            g = tiling.tile_grid(H, W, TILE, STRIDE)
            org = [(oy, ox) for oy in g.oys for ox in g.oxs]
            assert len(org) == 24 and len(org) % BATCH != 0
            d = max(plain.size_divisibility, 1)
            ch, cw = -(-g.th // d) * d, -(-g.tw // d) * d
            sizes = torch.tensor([[g.th, g.tw]] * BATCH, dtype=torch.int32, device="cuda")
            tiles, crop = [], None
            for i in range(0, len(org), BATCH):
                grp = org[i:i + BATCH]
                canvas = torch.empty(len(grp), 3, ch, cw, device="cuda")
                ops.tile_crops(img, grp, g.th, g.tw, canvas)
                lg = eng.head_logits(canvas, sizes[:len(grp)])
                crop = (min(lg.shape[2], g.th), min(lg.shape[3], g.tw))
                tiles += [_post(lg[j], (g.th, g.tw), crop) for j in range(len(grp))]
            assert _banded(crop[0], crop[1], g.th, g.tw) and _banded(crop[0], crop[1], H, W)   # equality is owed
            canvas = torch.zeros(1, 3, ch, cw, device="cuda")
            small = torch.empty(1, 3, g.th, g.tw, device="cuda")
            ops.resize_bilinear(img[None], small)
            canvas[:, :, :g.th, :g.tw].copy_(small)
            gout = _post(eng.head_logits(canvas, sizes[:1])[0], (H, W), crop)
            _CACHE["composition"] = _compose(tiles, gout, g, "pyramid", True)
            _CACHE["uniform_composition"] = _compose(tiles, gout, g, "uniform", False)
    return _CACHE["composition"]


def _blended_probs():
    if "probs" not in _CACHE:
        out = _tiled(**BLEND)([{"image": _image()}])[0]
        assert set(out) == {"sem_seg"}
        _CACHE["probs"] = out["sem_seg"].cpu()
    return _CACHE["probs"]


def test_probs_equal_the_composition():
    ref = _composition()
    got = _blended_probs()
    assert got.shape == ref.shape == (int(_tokens().shape[0]), H, W)
    assert torch.equal(got, ref)
    assert 0 < (got.argmax(0) > 0).float().mean() < 1
    # the feature is not a no-op on this image
    assert not torch.equal(got, _CACHE["uniform_composition"])


def test_labels_equal_the_composition_and_the_argmax_of_probs():
    ref = _composition()
    out = _tiled("labels", **BLEND)([{"image": _image()}])[0]
    assert set(out) == {"sem_seg_labels", "sem_seg_score"}
    lab, sc = out["sem_seg_labels"].cpu(), out["sem_seg_score"].cpu()
    assert torch.equal(lab, ref.argmax(0).int()) and torch.equal(sc, ref.max(0).values)
    probs = _blended_probs()
    assert torch.equal(lab, probs.argmax(0).int()) and torch.equal(sc, probs.max(0).values)


def test_explicit_defaults_equal_a_model_without_the_keys():
    off = _tiled(**{"MODEL.CATSEG_HIP.TILED.WINDOW": "uniform", "MODEL.CATSEG_HIP.TILED.GLOBAL": "False"})
    a = off([{"image": _image()}])[0]["sem_seg"].cpu()
    b = _tiled()([{"image": _image()}])[0]["sem_seg"].cpu()
    assert torch.equal(a, b)
    _composition()
    assert torch.equal(a, _CACHE["uniform_composition"])


def test_batch_1_equals_batch_5():
    one = _tiled(batch=1, **BLEND)([{"image": _image()}])[0]["sem_seg"].cpu()
    assert torch.equal(one, _blended_probs())


def test_a_single_tile_has_no_global_view():
    """60 x 80 under the default 384 tile is one tile: the global view would be the same image and is skipped."""
    img = _image(60, 80, seed=9)
    g = tiling.tile_grid(60, 80, 384, 256)
    assert (g.ny, g.nx) == (1, 1)
    kw = dict(batch=8, tile=384, stride=256)
    a = _tiled(**kw, **{"MODEL.CATSEG_HIP.TILED.GLOBAL": "True"})([{"image": img}])[0]["sem_seg"].cpu()
    b = _tiled(**kw, **{"MODEL.CATSEG_HIP.TILED.GLOBAL": "False"})([{"image": img}])[0]["sem_seg"].cpu()
    assert torch.equal(a, b)


def test_evaluator_bins_the_blended_label_map():
    T = int(_tokens().shape[0])
    gen = torch.Generator().manual_seed(1)
    gt = torch.randint(0, T, (H, W), generator=gen).int()
    gt[torch.rand(H, W, generator=gen) < 0.1] = 255
    inputs = [{"image": _image(), "sem_seg_gt": gt.numpy(), "file_name": "im0.png"}]
    outputs = _tiled("labels", **BLEND)(inputs)
    ev = SemSegEvaluator(None, distributed=False, output_dir=None, class_names=[f"c{i}" for i in range(T)],
                         ignore_label=255)
    ev.process(inputs, outputs)
    lab = outputs[0]["sem_seg_labels"].cpu().long()
    assert torch.equal(lab, _composition().argmax(0))
    gq = torch.where(gt == 255, torch.full_like(gt, T), gt).long()
    want = torch.bincount(((T + 1) * lab + gq).reshape(-1), minlength=(T + 1) ** 2).reshape(T + 1, T + 1)
    assert int(want.sum()) == H * W
    assert np.array_equal(ev.confusion_matrix(), want.numpy())
