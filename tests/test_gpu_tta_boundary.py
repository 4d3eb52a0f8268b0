"""MODEL.CATSEG_HIP.TTA_MERGE "device" at the drop-in boundary: SemanticSegmentorWithTTA merges the views'
logits with one catseg_postprocess_tta launch and returns what the "host" merge (the reference's flip, add
and divide over the views' full-size volumes) returns, and a label map for a model built with OUTPUT "labels".

One seeded 60 x 80 image: the tiny model's logits are 96 x 96 and the views below 96 px are smaller than
that, so they carry real, differing crops.  Output width 80 runs catseg_postprocess banded, so the views'
values are the same bit for bit on both paths; with K = 4 the division by K and the multiplication by its
fp32 reciprocal are both exact."""
import os

import numpy as np
import pytest
import torch

from cat_seg import SemanticSegmentorWithTTA, build_model
from cat_seg.evaluation import SemSegEvaluator
from cat_seg.test_time_augmentation import DatasetMapperTTA

from conftest import GOLDEN
from test_boundary_cpu import tiny_cfg

pytestmark = pytest.mark.gpu

_CACHE = {}


def _tokens():
    if "tokens" not in _CACHE:
        _CACHE["tokens"] = dict(np.load(os.path.join(GOLDEN, "e2e_tiny_eval.npz")))["tokens"]
    return _CACHE["tokens"]


def _image():
    return (torch.rand((3, 60, 80), generator=torch.Generator().manual_seed(5)) * 255).to(torch.uint8)


def _wrapper(merge, output="probs", min_sizes=(48, 64), batch_size=1, **over):
    cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.TTA_MERGE": merge, "MODEL.CATSEG_HIP.OUTPUT": output, **over})
    m = build_model(cfg).cuda().eval()
    m.sem_seg_head.predictor.set_class_tokens(_tokens())
    return SemanticSegmentorWithTTA(cfg, m, tta_mapper=DatasetMapperTTA(min_sizes=min_sizes, max_size=4000, flip=True),
                                    batch_size=batch_size)


def _host(min_sizes, **inp):
    key = ("host", min_sizes, tuple(sorted(inp.items())))
    if key not in _CACHE:
        _CACHE[key] = _wrapper("host", min_sizes=min_sizes)([{"image": _image(), **inp}])[0]["sem_seg"].cpu()
    return _CACHE[key]


def _device_probs(min_sizes=(48, 64), **inp):
    key = ("device", min_sizes, tuple(sorted(inp.items())))
    if key not in _CACHE:
        _CACHE[key] = _wrapper("device", min_sizes=min_sizes)([{"image": _image(), **inp}])[0]["sem_seg"].cpu()
    return _CACHE[key]


def test_mapper_views_have_differing_crops():
    views = DatasetMapperTTA(min_sizes=(48, 64, 120), flip=True)({"image": _image()})
    assert [tuple(v["image"].shape[1:]) for v in views] == [(48, 64)] * 2 + [(64, 85)] * 2 + [(120, 160)] * 2


@pytest.mark.parametrize("graph", ["True", "False"])
@pytest.mark.parametrize("batch_size", [1, 2])
def test_device_merge_equals_host_merge_k4(graph, batch_size):
    ref = _host((48, 64))
    assert ref.shape[1:] == (60, 80)
    w = _wrapper("device", batch_size=batch_size, **{"MODEL.CATSEG_HIP.GRAPH": graph})
    out = w([{"image": _image()}])[0]
    assert set(out) == {"sem_seg"} and out["sem_seg"].is_cuda
    assert torch.equal(out["sem_seg"].cpu(), ref)


def test_device_merge_k6_within_one_ulp_of_the_scale():
    """K = 6: the host divides by 6, the device multiplies by fp32(1 / 6): at most one ulp of a value below
    1 apart (6e-8); nothing else differs.  2e-7 absolute."""
    ref = _host((48, 64, 120))
    got = _device_probs((48, 64, 120))
    err = (got - ref).abs().max().item()
    print(f"K=6 device vs host merge: max abs diff {err:.2e}")
    assert err <= 2e-7


@pytest.mark.parametrize("hw", [None, (50, 68)])
def test_labels_model_returns_the_argmax_of_the_device_merge(hw):
    inp = {} if hw is None else {"height": hw[0], "width": hw[1]}
    probs = _device_probs(**inp)
    out = _wrapper("device", output="labels")([{"image": _image(), **inp}])[0]
    assert set(out) == {"sem_seg_labels", "sem_seg_score"}
    lab, sc = out["sem_seg_labels"], out["sem_seg_score"]
    assert lab.dtype == torch.int32 and sc.dtype == torch.float32 and lab.is_cuda and sc.is_cuda
    assert lab.shape == sc.shape == (hw or (60, 80)) == probs.shape[1:]
    assert torch.equal(lab.cpu(), probs.argmax(0).int())
    assert torch.equal(sc.cpu(), probs.max(0).values)


def test_evaluator_gives_the_same_confusion_matrix():
    T = int(_tokens().shape[0])
    gen = torch.Generator().manual_seed(1)
    gt = torch.randint(0, T, (60, 80), generator=gen).int()
    gt[torch.rand(60, 80, generator=gen) < 0.1] = 255
    inputs = [{"image": _image(), "sem_seg_gt": gt.numpy(), "file_name": "im0.png"}]
    mats = []
    for output in ("probs", "labels"):
        ev = SemSegEvaluator(None, distributed=False, output_dir=None, class_names=[f"c{i}" for i in range(T)],
                             ignore_label=255)
        ev.process(inputs, _wrapper("device", output=output)(inputs))
        mats.append(ev.confusion_matrix())
    assert int(mats[0].sum()) == 60 * 80
    assert np.array_equal(mats[0], mats[1])


def test_forward_logits():
    m = build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.RETURN_ALL_IMAGES": "False"})).cuda().eval()
    m.sem_seg_head.predictor.set_class_tokens(_tokens())
    a = _image()
    logits, crops = m.forward_logits([{"image": a}, {"image": a[:, :48, :64]}])
    assert logits.shape == (2, int(_tokens().shape[0]), 96, 96) and logits.dtype == torch.float32
    assert crops == [(60, 80), (48, 64)]
    assert len(m([{"image": a}, {"image": a[:, :48, :64]}])) == 1        # forward keeps the reference mode
    s = build_model(tiny_cfg(**{"TEST.SLIDING_WINDOW": "True"})).cuda().eval()
    with pytest.raises(RuntimeError, match="SLIDING_WINDOW"):
        s.forward_logits([{"image": a}])
    with pytest.raises(RuntimeError, match="eval"):
        m.train().forward_logits([{"image": a}])


def test_more_than_32_views_raise_at_call_time():
    w = _wrapper("device", min_sizes=tuple(range(40, 40 + 17)))          # 34 views
    with pytest.raises(ValueError, match="32"):
        w([{"image": _image()}])
