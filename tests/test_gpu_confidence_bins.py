"""catseg_confidence_bins on the device: the counters equal the numpy restatement (tests/confidence_ref.py)
exactly, whatever order the pixels land in."""
import numpy as np
import pytest
import torch

import confidence_ref as CR
from cat_seg import _lib as L
from cat_seg import ops

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def _case(K, H, W, n_classes, n_bins, seed):
    """Top-k maps with ties to the ground truth at every rank, ignored pixels, labels beyond the classes (the fold),
    NaN / inf / negative confidences and confidences of exactly 0, 1 and b / n_bins."""
    g = torch.Generator().manual_seed(seed)
    gt = torch.randint(0, n_classes, (H, W), generator=g).int()
    labels = torch.randint(0, n_classes + 2, (K, H, W), generator=g).int()
    for k in range(K):          # a share of the pixels is hit at rank k
        hit = torch.rand(H, W, generator=g) < 0.3
        labels[k][hit] = gt[hit]
    gt[torch.rand(H, W, generator=g) < 0.1] = 255
    conf = torch.rand(H, W, generator=g)
    edges = (torch.randint(0, n_bins + 1, (H, W), generator=g).float() / n_bins)      # 0, b / n_bins, 1: the bin edges
    pick = torch.rand(H, W, generator=g)
    conf = torch.where(pick < 0.3, edges, conf)
    conf[(pick >= 0.3) & (pick < 0.35)] = float("nan")
    conf[(pick >= 0.35) & (pick < 0.38)] = 1.5
    conf[(pick >= 0.38) & (pick < 0.41)] = -0.25
    conf[(pick >= 0.41) & (pick < 0.42)] = float("inf")
    flat = conf.view(-1)
    flat[:3] = torch.tensor([0.0, 1.0, float("nan")])[: flat.numel()]
    return labels, conf, gt


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("n_bins", [1, 15, 256])
@pytest.mark.parametrize("H,W,n_classes,clamp", [(5, 7, 1, -1), (97, 131, 150, -1), (48, 64, 21, 20)])
def test_counters_equal_the_restatement(H, W, n_classes, clamp, n_bins, K):
    labels, conf, gt = _case(K, H, W, n_classes, n_bins, seed=H + n_bins + K)
    kw = dict(num_classes=n_classes, ignore_label=255, clamp_pred=clamp, n_bins=n_bins)
    counters = torch.zeros(3 * n_bins + K + 2, dtype=torch.int64, device="cuda")
    ref = np.zeros(3 * n_bins + K + 2, np.int64)
    for _ in range(2):          # accumulates across calls
        ops.confidence_bins(labels.cuda(), conf.cuda(), gt.cuda(), counters, **kw)
        ref += CR.counters(labels.numpy(), conf.numpy(), gt.numpy(), **kw)
    got = counters.cpu().numpy()
    assert np.array_equal(got, ref)
    live = int((gt != 255).sum())
    assert got[-2] + got[-1] == 2 * live and got[:n_bins].sum() == got[-2]
    if H * W > 100:
        assert got[-1] > 0 and 0 < got[n_bins:2 * n_bins].sum() < got[-2]
        assert all(got[3 * n_bins + k] <= got[3 * n_bins + k + 1] for k in range(K - 1))


def test_ground_truth_outside_the_classes_enters_nothing():
    labels, conf, gt = _case(2, 16, 16, 5, 15, seed=3)
    gt[0, :4] = torch.tensor([7, -2, 5, 255], dtype=torch.int32)
    kw = dict(num_classes=5, n_bins=15)
    counters = torch.zeros(3 * 15 + 4, dtype=torch.int64, device="cuda")
    ops.confidence_bins(labels.cuda(), conf.cuda(), gt.cuda(), counters, **kw)
    assert np.array_equal(counters.cpu().numpy(), CR.counters(labels.numpy(), conf.numpy(), gt.numpy(), **kw))
    assert int(counters[-2] + counters[-1]) == int(((gt >= 0) & (gt < 5)).sum())
