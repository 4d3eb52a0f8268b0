"""The evaluators' `boundary=` argument on the device: the metrics of SemSegEvaluator / VOCbEvaluator over images of
different sizes, fed as probabilities and as label maps, against the numpy restatement (tests/boundary_ref.py).  The
counters are equal integers, so the floats agree to 1e-12 relative."""
import math

import numpy as np
import pytest
import torch

import boundary_ref as B
from cat_seg import _lib as L
from cat_seg import ops
from cat_seg.evaluation import SemSegEvaluator, VOCbEvaluator

pytestmark = pytest.mark.gpu

NAMES = ["road", "roof", "tree", "water", "car"]
SPECS = [("ratio", 0.02), ("px", 3)]
TAGS = ["0.02d", "3px"]


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def image(H, W, seed, n, pred_max):
    """(pred, gt): ground truth of 14-pixel blocks with an ignore patch, the prediction shifted by (2, 1) + speckle."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W]
    G = (yy // 14 + 2 * (xx // 14)) % n
    P = np.roll(G, (2, 1), (0, 1))
    P = np.where(rng.random((H, W)) < 0.04, rng.integers(0, pred_max + 1, (H, W)), P)
    G[4:13, W - 25:W - 6] = 255
    return P.astype(np.int64), G.astype(np.int64)


def as_probs(P, T):
    """(T, H, W) fp32 scores whose argmax is P."""
    g = torch.Generator().manual_seed(int(P.sum()) % 1000)
    probs = torch.rand((T,) + P.shape, generator=g) * 0.5
    probs.scatter_(0, torch.from_numpy(P)[None], 1.0)
    return probs.cuda()


def feed(ev, images, T, as_labels):
    for (P, G), lab in zip(images, as_labels):
        out = {"sem_seg_labels": torch.from_numpy(P).int().cuda()} if lab else {"sem_seg": as_probs(P, T)}
        ev.process([{"sem_seg_gt": torch.from_numpy(G)}], [out])


def reference(images, n, clamp_pred, names):
    conf, c = np.zeros((n + 1, n + 1), np.int64), None
    for P, G in images:
        H, W = P.shape
        conf += B.confusion(P, G, n, 255, clamp_pred)[0]
        c = B.counters(P, G, [B.ratio_width(0.02, H, W), 3], n, 255, clamp_pred, out=c)
    return conf, c, B.metrics(conf, c, names, TAGS)


def same(a, b, rel=0.0):
    return (math.isnan(a) and math.isnan(b)) or a == b or abs(a - b) <= rel * abs(b)


SIZES = [(96, 130), (150, 101), (64, 200)]          # 0.02 d = 3, 4, 4 pixels


def test_semseg_evaluator_metrics():
    images = [image(H, W, i, 5, 4) for i, (H, W) in enumerate(SIZES)]
    assert [B.ratio_width(0.02, H, W) for H, W in SIZES] == [3, 4, 4]
    ev = SemSegEvaluator(class_names=NAMES, distributed=False, boundary=SPECS)
    feed(ev, images, 5, (False, True, False))
    res = ev.evaluate()["sem_seg"]
    conf, c, ref = reference(images, 5, -1, NAMES)
    assert np.array_equal(ev.confusion_matrix(), conf)
    assert np.array_equal(ev._bcounters.cpu().numpy(), c)
    assert c.reshape(2, -1).sum(1).min() > 0
    for k, v in ref.items():
        assert k in res and same(res[k], v, 1e-12), (k, res[k], v)
    # the prediction is the ground truth shifted: its errors lie at the class boundaries
    assert 0 < res["mBIoU@3px"] < 100 and res["trimap-mIoU@3px"] < res["eroded-mIoU@3px"]
    # the plain metrics are what an evaluator without the argument gives, key for key, in the same order
    plain = SemSegEvaluator(class_names=NAMES, distributed=False)
    feed(plain, images, 5, (False, True, False))
    base = plain.evaluate()["sem_seg"]
    assert list(res)[:len(base)] == list(base) and set(res) - set(base) == set(ref)
    assert all(same(res[k], base[k]) for k in base)
    # reset() clears the counters
    ev.reset()
    assert int(ev._bcounters.abs().sum()) == 0 and int(ev._conf.sum()) == 0
    feed(ev, images[:1], 5, (True,))
    one = reference(images[:1], 5, -1, NAMES)
    assert np.array_equal(ev._bcounters.cpu().numpy(), one[1])


def test_vocb_evaluator_folds_before_the_distance():
    names = [f"c{i}" for i in range(21)]
    images = [image(H, W, 10 + i, 21, 24) for i, (H, W) in enumerate(SIZES[:2])]
    ev = VOCbEvaluator(class_names=names, distributed=False, boundary=SPECS)
    feed(ev, images, 25, (False, True))
    res = ev.evaluate()["sem_seg"]
    conf, c, ref = reference(images, 21, 20, names)
    assert np.array_equal(ev._bcounters.cpu().numpy(), c)
    assert not np.array_equal(c, reference(images, 21, -1, names)[1])
    for k, v in ref.items():
        assert same(res[k], v, 1e-12), (k, res[k], v)


def test_boundary_none_changes_nothing(tmp_path):
    images = [image(H, W, 20 + i, 5, 4) for i, (H, W) in enumerate(SIZES[:2])]
    old, ops.PROFILE = ops.PROFILE, []
    try:
        a = SemSegEvaluator(class_names=NAMES, distributed=False, boundary=None)
        feed(a, images, 5, (False, True))
        ra = a.evaluate()["sem_seg"]
        kernels = [r["kernel"] for r in ops.PROFILE]
    finally:
        ops.PROFILE = old
    assert kernels and not [k for k in kernels if k.startswith("boundary_")]
    assert not hasattr(a, "_bcounters")
    b = SemSegEvaluator(class_names=NAMES, distributed=False)
    feed(b, images, 5, (False, True))
    rb = b.evaluate()["sem_seg"]
    assert list(ra) == list(rb) and all(same(ra[k], rb[k]) for k in ra)
    assert not [k for k in ra if "BIoU" in k or "trimap" in k or "eroded" in k]
    # and with the argument the recorder sees the new launches
    old, ops.PROFILE = ops.PROFILE, []
    try:
        c = SemSegEvaluator(class_names=NAMES, distributed=False, boundary=SPECS, output_dir=str(tmp_path))
        feed(c, images, 5, (False, True))
        rc = c.evaluate()["sem_seg"]
        kernels = [r["kernel"] for r in ops.PROFILE]
    finally:
        ops.PROFILE = old
    assert kernels.count("boundary_confusion") == 2 and kernels.count("boundary_distance") == 4
    saved = torch.load(str(tmp_path / "sem_seg_evaluation.pth"), weights_only=False)
    assert list(saved) == list(rc) and "mBIoU@0.02d" in saved
