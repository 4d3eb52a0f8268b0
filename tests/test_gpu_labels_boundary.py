"""MODEL.CATSEG_HIP.OUTPUT "labels" at the drop-in boundary: every eval branch of CATSeg.forward returns
{"sem_seg_labels", "sem_seg_score"} equal to the argmax / max of what the same model built with "probs"
returns, and the evaluators give the same matrices, metrics and prediction files from either.

Exact equality is asserted where the probs model's resize runs a banded kernel (output width a multiple of
4 and the band's source rows within LDS, misc.hip launch_post), since the fused kernel restates that
arithmetic; for other output sizes the two may differ where two classes are within rounding of each other."""
import json
import os

import numpy as np
import pytest
import torch

from cat_seg import build_model
from cat_seg.evaluation import SemSegEvaluator, VOCbEvaluator

from conftest import GOLDEN
from test_boundary_cpu import tiny_cfg

pytestmark = pytest.mark.gpu

_TOKENS = {}


def _tokens(name="e2e_tiny_eval"):
    if name not in _TOKENS:
        _TOKENS[name] = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    return _TOKENS[name]


def _model(output, **over):
    m = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": output, **over})).cuda().eval()
    m.sem_seg_head.predictor.set_class_tokens(_tokens()["tokens"])
    return m


def _pair(**over):
    """The tiny model twice with the same (seed 0) weights: OUTPUT "probs" and "labels"."""
    models = [_model(output, **over) for output in ("probs", "labels")]
    assert models[0].output == "probs" and models[1].output == "labels"
    return models


def _images(shapes, seed=3):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in shapes]


def _assert_exact(p, l):
    assert set(l) == {"sem_seg_labels", "sem_seg_score"}
    lab, sc = l["sem_seg_labels"], l["sem_seg_score"]
    assert lab.dtype == torch.int32 and sc.dtype == torch.float32 and lab.is_cuda and sc.is_cuda
    assert lab.shape == sc.shape == p["sem_seg"].shape[1:]
    probs = p["sem_seg"].cpu()
    assert torch.equal(lab.cpu(), probs.argmax(0).int())
    assert torch.equal(sc.cpu(), probs.max(0).values)


def _assert_within_rounding(p, l):
    """The probs model's probability of the returned label is within 1e-5 of the pixel's maximum, and the
    labels agree wherever its top two classes are at least 1e-5 apart."""
    probs = p["sem_seg"].cpu()
    lab = l["sem_seg_labels"].cpu().long()
    assert lab.shape == probs.shape[1:]
    top2 = probs.topk(2, dim=0).values
    assert ((top2[0] - probs.gather(0, lab[None])[0]) <= 1e-5).all()
    clear = (top2[0] - top2[1]) >= 1e-5
    assert clear.float().mean() > 0.9
    assert torch.equal(lab[clear], probs.argmax(0)[clear])
    assert (l["sem_seg_score"].cpu() - top2[0]).abs().max().item() <= 1e-5


@pytest.mark.parametrize("graph", ["True", "False"])
def test_labels_equal_argmax_of_probs(graph):
    pm, lm = _pair(**{"MODEL.CATSEG_HIP.GRAPH": graph})
    a, b = _images([(3, 384, 384), (3, 300, 352)])
    # two sizes, height / width given for one; output widths 300 and 352
    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    pr, lr = pm(inputs), lm(inputs)
    assert len(pr) == len(lr) == 2
    assert lr[0]["sem_seg_labels"].shape == (200, 300) and lr[1]["sem_seg_labels"].shape == (300, 352)
    for p, l in zip(pr, lr):
        _assert_exact(p, l)
    # equal sizes: the whole batch is resized with one launch
    c, d = _images([(3, 300, 352)] * 2, seed=4)
    inputs = [{"image": c}, {"image": d}]
    pr, lr = pm(inputs), lm(inputs)
    for p, l in zip(pr, lr):
        _assert_exact(p, l)
    assert not torch.equal(lr[0]["sem_seg_labels"], lr[1]["sem_seg_labels"])


def _assert_same_result(got, want):
    assert got.keys() == want.keys()
    for k in got:
        if k == "regions_info":
            assert got[k].keys() == want[k].keys()
            for col in got[k]:
                assert torch.equal(got[k][col], want[k][col]), (k, col)
        else:
            assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("output", ["probs", "labels"])
def test_eager_batch_equals_single_image_calls(output):
    """MODEL.CATSEG_HIP.GRAPH False: a uniform batch (equal image sizes, equal output sizes) is resized with one
    launch, its results views of one tensor, and a batch with one output size changed with one launch per
    image; either way every returned tensor equals what a call with that image alone returns (the labels
    model with its regions: the region numbers and every column of the table)."""
    over = {"MODEL.CATSEG_HIP.GRAPH": "False"}
    if output == "labels":
        over["MODEL.CATSEG_HIP.REGIONS.ENABLED"] = "True"
    m = _model(output, **over)
    assert not m.use_graph
    key = "sem_seg" if output == "probs" else "sem_seg_score"
    ims =_images([(3, 40, 48)] * 3)
    asked = {"height": 50, "width": 60}
    for sizes, uniform in (([{}] * 3, True), ([asked] * 3, True), ([asked, {**asked, "height": 44}, asked], False)):
        inputs = [{"image": im, **s} for im, s in zip(ims, sizes)]
        batch = m(inputs)
        assert len(batch) == 3
        for x, got in zip(inputs, batch):
            assert got[key].shape[-2:] == (x.get("height", 40), x.get("width", 48))
            assert got[key]._base.shape[0] == (3 if uniform else 1)      # the launch this result is a view of
            _assert_same_result(got, m([x])[0])
        assert not torch.equal(batch[0][key], batch[2][key])


def test_odd_output_width_is_within_rounding():
    pm, lm = _pair()
    inputs = [{"image": _images([(3, 320, 352)])[0], "height": 211, "width": 301}]
    _assert_within_rounding(pm(inputs)[0], lm(inputs)[0])


def test_reference_mode_returns_one_dict():
    pm, lm = _pair(**{"MODEL.CATSEG_HIP.RETURN_ALL_IMAGES": "False"})
    a, b = _images([(3, 384, 384), (3, 300, 352)])
    inputs = [{"image": a, "height": 200, "width": 300}, {"image": b}]
    out = lm(inputs)
    assert len(out) == 1
    _assert_exact(pm(inputs)[0], out[0])


def test_sliding_window_labels():
    """TEST.SLIDING_WINDOW: the argmax of the merged 640 x 640 probabilities without a sigmoid.  640 x 640
    (the probs model returns the merge itself) and 1400 x 128 (the one kind of size at which its resize from
    640 x 640 fits a banded kernel: <= 25 source rows per 48-row band) are exact; 480 x 400, the existing
    sliding test's size, goes through the probs model's unbanded fallback and is held to the rounding rule."""
    g = _tokens("e2e_tiny_sliding")
    pm, lm = _pair(**{"TEST.SLIDING_WINDOW": "True"})
    for m in (pm, lm):
        m.sem_seg_head.predictor.set_class_tokens(g["tokens"])
    im = torch.from_numpy(g["image0"])
    inputs = [{"image": im}, {"image": im, "height": 1400, "width": 128},
              {"image": im, "height": int(g["height"]), "width": int(g["width"])}]
    pr, lr = pm(inputs), lm(inputs)
    assert lr[0]["sem_seg_labels"].shape == (640, 640) and lr[1]["sem_seg_labels"].shape == (1400, 128)
    _assert_exact(pr[0], lr[0])
    _assert_exact(pr[1], lr[1])
    _assert_within_rounding(pr[2], lr[2])


def test_compile_fullgraph_labels_model():
    """torch.compile(fullgraph=True) of the labels model (the pattern of
    tests/test_gpu_custom_ops.py::test_compile_catseg_forward_fullgraph): the resize traces as
    catseg::postprocess_argmax and returns the eager labels."""
    lm = _pair()[1]
    im = torch.from_numpy(_tokens()["image0"])
    inputs = [{"image": im, "height": 200, "width": 300}, {"image": im[:, :40, :48]}]
    eager = lm(inputs)
    torch._dynamo.reset()
    got = torch.compile(lm, fullgraph=True, backend="aot_eager")(inputs)
    assert len(got) == len(eager) == 2
    for a, b in zip(eager, got):
        assert set(b) == {"sem_seg_labels", "sem_seg_score"}
        assert torch.equal(a["sem_seg_labels"], b["sem_seg_labels"])
        assert torch.equal(a["sem_seg_score"], b["sem_seg_score"])


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = float(a[k]), float(b[k])
        assert (np.isnan(x) and np.isnan(y)) or x == y, (k, x, y)


@pytest.mark.parametrize("cls", [SemSegEvaluator, VOCbEvaluator])
def test_evaluators_agree_on_labels_and_probs(cls, tmp_path):
    pm, lm = _pair()
    T = int(_tokens()["tokens"].shape[0])
    names = [f"c{i}" for i in range(T + 1 if cls is VOCbEvaluator else T)]
    ims = _images([(3, 320, 352), (3, 384, 384), (3, 320, 352)], seed=9)
    hw = [(200, 300), (384, 384), (320, 352)]
    gen = torch.Generator().manual_seed(1)
    inputs = []
    for i, (im, (h, w)) in enumerate(zip(ims, hw)):
        gt = torch.randint(0, T, (h, w), generator=gen).int()
        gt[torch.rand(h, w, generator=gen) < 0.1] = 255
        inputs.append({"image": im, "height": h, "width": w, "sem_seg_gt": gt.numpy(), "file_name": f"im{i}.png"})
    evs = []
    for m, sub in ((pm, "probs"), (lm, "labels")):
        ev = cls(None, distributed=False, output_dir=str(tmp_path / sub), class_names=names, ignore_label=255)
        ev.process(inputs[:2], m(inputs[:2]))
        ev.process(inputs[2:], m(inputs[2:]))
        evs.append((ev, ev.confusion_matrix(), ev.evaluate()["sem_seg"]))
    assert int(evs[0][1].sum()) == sum(h * w for h, w in hw)
    assert np.array_equal(evs[0][1], evs[1][1])
    _same(evs[0][2], evs[1][2])
    files = [(tmp_path / sub / "sem_seg_predictions.json").read_text() for sub in ("probs", "labels")]
    assert files[0] == files[1] and len(json.loads(files[0])) > 3
