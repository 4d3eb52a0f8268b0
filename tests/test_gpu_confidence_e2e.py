"""MODEL.CATSEG_HIP.CONFIDENCE at the drop-in boundary: the plain branch (graph and eager) and the sliding branch
return the top-k maps, the mass and the label map after the reject rule; regions and render run on that map; and
SemSegEvaluator(confidence=...) gives the same counters from a "labels" model as from the "probs" model of the same
weights, and the metrics tests/confidence_ref.py computes from the maps."""
import numpy as np
import pytest
import torch

import confidence_ref as CR
from cat_seg import ops
from cat_seg.evaluation import SemSegEvaluator, VOCbEvaluator

from test_gpu_label_regions import _model
from test_gpu_labels_boundary import _model as _output_model, _tokens

pytestmark = pytest.mark.gpu

CONF = {"MODEL.CATSEG_HIP.CONFIDENCE.ENABLED": "True"}
NEW_KEYS = {"sem_seg_topk_labels", "sem_seg_topk_score", "sem_seg_mass"}


def _inputs():
    gen = torch.Generator().manual_seed(3)
    a, b = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 384, 384), (3, 300, 352))]
    return [{"image": a, "height": 200, "width": 300}, {"image": b}]


def _check_maps(got, plain, K):
    """The new keys beside the old ones; plane 0 is what a model without CONFIDENCE returns."""
    assert set(got) == {"sem_seg_labels", "sem_seg_score"} | NEW_KEYS and set(plain) == {"sem_seg_labels", "sem_seg_score"}
    H, W = plain["sem_seg_labels"].shape
    assert got["sem_seg_topk_labels"].shape == (K, H, W) and got["sem_seg_topk_labels"].dtype == torch.int32
    assert got["sem_seg_topk_score"].shape == (K, H, W) and got["sem_seg_topk_score"].dtype == torch.float32
    assert got["sem_seg_mass"].shape == (H, W) and got["sem_seg_mass"].dtype == torch.float32
    assert torch.equal(got["sem_seg_topk_labels"][0], plain["sem_seg_labels"])
    assert torch.equal(got["sem_seg_score"], plain["sem_seg_score"])
    assert torch.equal(got["sem_seg_topk_score"][0], plain["sem_seg_score"])
    sc = got["sem_seg_topk_score"]
    assert bool((sc[:-1] >= sc[1:]).all()) and bool((got["sem_seg_mass"] >= sc.sum(0) * (1 - 1e-6)).all())


def test_plain_branch_graph_and_eager():
    inputs = _inputs()
    plain = _model()(inputs)
    outs = {}
    for graph in ("True", "False"):
        outs[graph] = _model(**{"MODEL.CATSEG_HIP.GRAPH": graph, **CONF})(inputs)
        for p, g in zip(plain, outs[graph]):
            _check_maps(g, p, 2)
            assert torch.equal(g["sem_seg_labels"], p["sem_seg_labels"])        # nothing is rejected
    for g, e in zip(outs["True"], outs["False"]):
        for k in g:
            assert torch.equal(g[k], e[k]), k
    # ENABLED False: the dict's keys are what they are today
    off = _model(**{"MODEL.CATSEG_HIP.CONFIDENCE.ENABLED": "False", "MODEL.CATSEG_HIP.CONFIDENCE.TOPK": "4"})(inputs)
    assert all(set(o) == {"sem_seg_labels", "sem_seg_score"} for o in off)


def test_topk4_uniform_batch():
    """A batch of equal images and sizes takes one launch; K = 4."""
    im = _inputs()[1]["image"]
    inputs = [{"image": im}, {"image": im.flip(-1)}]
    plain = _model()(inputs)
    for p, g in zip(plain, _model(**CONF, **{"MODEL.CATSEG_HIP.CONFIDENCE.TOPK": "4"})(inputs)):
        _check_maps(g, p, 4)


def test_sliding_branch():
    slide = {"TEST.SLIDING_WINDOW": "True"}
    a = _inputs()[1]["image"]
    inputs = [{"image": a}, {"image": a, "height": 480, "width": 400}]
    plain = _model(**slide)(inputs)
    got = _model(**slide, **CONF)(inputs)
    assert got[0]["sem_seg_labels"].shape == (640, 640) and got[1]["sem_seg_labels"].shape == (480, 400)
    for p, g in zip(plain, got):
        _check_maps(g, p, 2)
        assert torch.equal(g["sem_seg_labels"], p["sem_seg_labels"])


def test_min_score_rejects_into_the_label_beyond_the_classes_and_the_map_goes_on():
    inputs = _inputs()[1:]
    plain = _model()(inputs)[0]
    T = int(_tokens()["tokens"].shape[0])
    score = plain["sem_seg_score"]
    # above the median score: an fp32 value, which survives the config's text and the float argument
    min_score = float(score.flatten().kthvalue(int(0.6 * score.numel())).values)
    over = {**CONF, "MODEL.CATSEG_HIP.CONFIDENCE.MIN_SCORE": repr(min_score)}
    got = _model(**over)(inputs)[0]
    rejected = score < min_score
    assert 0.5 < rejected.float().mean().item() < 0.7
    assert torch.equal(got["sem_seg_labels"], torch.where(rejected, torch.full_like(plain["sem_seg_labels"], T),
                                                          plain["sem_seg_labels"]))
    assert torch.equal(got["sem_seg_topk_labels"][0], plain["sem_seg_labels"])  # plane 0 itself is not rejected
    # regions and render run on that map: the palette has one more row, black, for the reject label
    more = {"MODEL.CATSEG_HIP.REGIONS.ENABLED": "True", "MODEL.CATSEG_HIP.RENDER.ENABLED": "True",
            "MODEL.CATSEG_HIP.RENDER.ALPHA": "1.0", "MODEL.CATSEG_HIP.RENDER.EDGE_PX": "0"}
    m = _model(**over, **more)
    full = m(inputs)[0]
    assert NEW_KEYS | {"sem_seg_regions", "regions_info", "sem_seg_render"} <= set(full)
    assert torch.equal(full["sem_seg_labels"], got["sem_seg_labels"])
    pal = m._palette(full["sem_seg_labels"].device)
    assert pal.shape == (T + 1, 3) and pal[T].tolist() == [0, 0, 0]
    assert bool((full["sem_seg_render"][rejected] == 0).all())                  # ALPHA 1, no edges: black where rejected
    assert int(full["regions_info"]["label"].max()) == T


@pytest.mark.parametrize("cls,kind", [(SemSegEvaluator, "score"), (SemSegEvaluator, "normalized"), (VOCbEvaluator, "score")])
def test_evaluator_counters_from_labels_and_probs(cls, kind):
    pm, lm = _output_model("probs"), _model(**CONF)
    T = int(_tokens()["tokens"].shape[0])
    names = [f"c{i}" for i in range(T + 1 if cls is VOCbEvaluator else T)]
    gen = torch.Generator().manual_seed(9)
    ims = [(torch.rand(s, generator=gen) * 255).to(torch.uint8) for s in ((3, 320, 352), (3, 384, 384))]
    hw = [(200, 300), (384, 384)]            # widths at which the probs model's resize runs banded
    inputs = []
    for i, (im, (h, w)) in enumerate(zip(ims, hw)):
        gt = torch.randint(0, T, (h, w), generator=gen).int()
        gt[torch.rand(h, w, generator=gen) < 0.1] = 255
        inputs.append({"image": im, "height": h, "width": w, "sem_seg_gt": gt.numpy()})
    spec = dict(bins=15, kind=kind, topk=2)
    evs = []
    for m in (pm, lm):
        ev = cls(None, distributed=False, class_names=names, ignore_label=255, confidence=spec)
        outs = m(inputs)
        ev.process(inputs, outs)
        evs.append((ev._ccounters.cpu().numpy(), ev.evaluate()["sem_seg"], outs))
    assert np.array_equal(evs[0][0], evs[1][0]) and int(evs[0][0][-2]) > 0
    # the metrics, as the restatement computes them from the labels model's maps
    ref = np.zeros_like(evs[1][0])
    for x, o in zip(inputs, evs[1][2]):
        conf = o["sem_seg_topk_score"][0]
        if kind == "normalized":
            conf = conf / o["sem_seg_mass"]
        ref += CR.counters(o["sem_seg_topk_labels"].cpu().numpy(), conf.cpu().numpy(), x["sem_seg_gt"],
                           num_classes=len(names), clamp_pred=cls.clamp_pred, n_bins=15)
    assert np.array_equal(evs[1][0], ref)
    res = evs[1][1]
    for k, v in CR.metrics(ref, 15, 2).items():
        assert res[k] == pytest.approx(v, abs=1e-9), k
    assert res["pACC@1"] == res["pACC"] and res["pACC@1"] <= res["pACC@2"] <= 100.0
    assert 0.0 <= res["ECE"] <= res["MCE"] <= 100.0 and len(res["reliability"]["count"]) == 15
    # without confidence= nothing changes; a labels output without the maps is refused
    base = cls(None, distributed=False, class_names=names, ignore_label=255)
    base.process(inputs, evs[1][2])
    plain = base.evaluate()["sem_seg"]
    assert set(res) - set(plain) == {"ECE", "MCE", "pACC@1", "pACC@2", "reliability", "coverage", "selective-pACC",
                                     "nan-confidence"}
    assert all(plain[k] == res[k] or (np.isnan(plain[k]) and np.isnan(res[k])) for k in plain)
    ev = cls(None, distributed=False, class_names=names, ignore_label=255, confidence=spec)
    with pytest.raises(ValueError, match="CONFIDENCE.ENABLED"):
        ev.process(inputs, _model()(inputs))


def test_identity_topk_of_a_probability_volume_is_its_sort():
    """What the evaluator's probability path relies on: an identity-size call without the sigmoid returns the
    volume's own values."""
    g = torch.Generator().manual_seed(2)
    probs = torch.rand(1, 6, 37, 52, generator=g).cuda()
    got = ops.postprocess_topk(probs, 2, sigmoid=False, out_hw=(37, 52))
    vals, idx = torch.sort(probs, dim=1, descending=True, stable=True)
    assert torch.equal(got["topk_score"], vals[:, :2]) and torch.equal(got["topk_labels"], idx[:, :2].int())
