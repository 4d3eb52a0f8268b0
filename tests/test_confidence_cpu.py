"""The confidence outputs without a GPU: the ABI (header, library exports, binding), the host-side argument checks
of catseg_postprocess_topk / catseg_confidence_bins (they run before any launch), MODEL.CATSEG_HIP.CONFIDENCE, the
custom op's fake kernel, confidence_metrics against hand-made counters, the numpy restatement against a direct
histogram, and the refusals of the branches that keep one class per pixel."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import confidence_ref as CR
from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg import custom_ops  # noqa: F401  (registers torch.ops.catseg.*)
from cat_seg.evaluation import confidence_metrics, confidence_spec

from conftest import ROOT
from test_boundary_cpu import tiny_cfg

NEW = ("catseg_postprocess_topk", "catseg_confidence_bins")
LABELS = {"MODEL.CATSEG_HIP.OUTPUT": "labels", "MODEL.CATSEG_HIP.CONFIDENCE.ENABLED": "True"}


def test_header_library_and_binding_declare_the_new_entries():
    text = open(os.path.join(ROOT, "include", "catseg_hip_confidence.h")).read()
    assert '#include "catseg_hip_confidence.h"' in open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert f"int {name}(" in text and hasattr(lib, name)
    assert L.CONFIDENCE_HEADERS == ("catseg_hip_confidence.h",) and set(L.EXPORTED_CONFIDENCE) == set(NEW)
    bound = L.load()
    assert len(bound.catseg_postprocess_topk.argtypes) == 19 and len(bound.catseg_confidence_bins.argtypes) == 12
    assert bound.catseg_postprocess_topk.argtypes[13] is ctypes.c_float       # min_score
    assert bound.catseg_abi_version() == 1
    assert "A NaN class value makes the" in text                              # the mass and NaN, said in the header


def _topk(lib, *, logits=16, B=1, T=5, h=8, w=8, ch=8, cw=8, sigmoid=1, K=2, tl=16, ts=16, mass=0, labels=0,
          min_score=0.0, min_margin=0.0, reject=0, H=16, W=16):
    return lib.catseg_postprocess_topk(logits, B, T, h, w, ch, cw, sigmoid, K, tl, ts, mass, labels, min_score,
                                       min_margin, reject, H, W, None)


@pytest.mark.parametrize("bad,text", [
    ({"K": 0}, b"K out of range"), ({"K": 5}, b"K out of range"), ({"K": 4, "T": 3}, b"K out of range"),
    ({"tl": 0}, b"null"), ({"ts": 0}, b"null"), ({"logits": 0}, b"null"),
    ({"tl": 18}, b"misaligned"), ({"mass": 6}, b"misaligned"), ({"labels": 17}, b"misaligned"),
    ({"cw": 9}, b"bad crop"), ({"ch": 0}, b"bad crop"),
    ({"h": 640, "w": 640, "ch": 640, "cw": 640, "H": 64, "W": 64}, b"LDS"),
    ({"labels": 16, "reject": -1}, b"reject_label"),
    ({"T": 0}, b"positive"), ({"B": 1 << 20}, b"grid"),
])
def test_postprocess_topk_rejects_bad_arguments_before_any_launch(bad, text):
    lib = L.load()
    assert _topk(lib, **bad) == -1
    err = lib.catseg_last_error()
    assert err.startswith(b"postprocess_topk:") and text in err


def _bins(lib, *, tl=16, K=2, conf=16, gt=16, H=4, W=4, N=5, ignore=255, clamp=-1, n_bins=15, counters=16):
    return lib.catseg_confidence_bins(tl, K, conf, gt, H, W, N, ignore, clamp, n_bins, counters, None)


@pytest.mark.parametrize("bad,text", [
    ({"n_bins": 0}, b"n_bins"), ({"n_bins": 257}, b"n_bins"), ({"K": 0}, b"K must"), ({"K": 5}, b"K must"),
    ({"tl": 0}, b"null"), ({"conf": 0}, b"null"), ({"gt": 0}, b"null"), ({"counters": 0}, b"null"),
    ({"counters": 20}, b"misaligned"), ({"conf": 18}, b"misaligned"), ({"H": 0}, b"H and W"), ({"N": 0}, b"num_classes"),
])
def test_confidence_bins_rejects_bad_arguments_before_any_launch(bad, text):
    lib = L.load()
    assert _bins(lib, **bad) == -1
    err = lib.catseg_last_error()
    assert err.startswith(b"confidence_bins:") and text in err


def test_config_keys_and_defaults():
    c = tiny_cfg().MODEL.CATSEG_HIP.CONFIDENCE
    assert (c.ENABLED, c.TOPK, c.MIN_SCORE, c.MIN_MARGIN, c.REJECT_LABEL) == (False, 2, 0.0, 0.0, -1)
    m = build_model(tiny_cfg())
    assert m.confidence is False and m.confidence_reject(5) is None
    m = build_model(tiny_cfg(**LABELS))
    assert m.confidence and m.confidence_topk == 2 and m.confidence_reject(5) is None      # nothing is rejected
    m = build_model(tiny_cfg(**LABELS, **{"MODEL.CATSEG_HIP.CONFIDENCE.MIN_SCORE": "0.5",
                                          "MODEL.CATSEG_HIP.CONFIDENCE.TOPK": "4"}))
    assert m.confidence_topk == 4 and m.confidence_reject(5) == (0.5, 0.0, 5)             # -1: the number of classes
    m = build_model(tiny_cfg(**LABELS, **{"MODEL.CATSEG_HIP.CONFIDENCE.MIN_MARGIN": "0.1",
                                          "MODEL.CATSEG_HIP.CONFIDENCE.REJECT_LABEL": "3"}))
    assert m.confidence_reject(5) == (0.0, 0.1, 3)
    with pytest.raises(ValueError, match="TOPK"):
        build_model(tiny_cfg(**LABELS, **{"MODEL.CATSEG_HIP.CONFIDENCE.TOPK": "5"}))
    with pytest.raises(ValueError, match="OUTPUT 'labels'"):
        build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.CONFIDENCE.ENABLED": "True"}))


def test_tiled_tta_and_traced_branches_refuse():
    with pytest.raises(ValueError, match="CONFIDENCE does not serve MODEL.CATSEG_HIP.TILED"):
        build_model(tiny_cfg(**LABELS, **{"MODEL.CATSEG_HIP.TILED.ENABLED": "True"}))
    with pytest.raises(ValueError, match="CONFIDENCE does not serve MODEL.CATSEG_HIP.TTA_MERGE"):
        build_model(tiny_cfg(**LABELS, **{"MODEL.CATSEG_HIP.TTA_MERGE": "device"}))
    from cat_seg import SemanticSegmentorWithTTA
    with pytest.raises(ValueError, match="does not serve MODEL.CATSEG_HIP.CONFIDENCE"):
        SemanticSegmentorWithTTA(tiny_cfg(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device", "MODEL.CATSEG_HIP.OUTPUT": "labels"}),
                                 build_model(tiny_cfg(**LABELS)))
    with pytest.raises(RuntimeError, match="CONFIDENCE cannot be traced"):
        build_model(tiny_cfg(**LABELS))._forward_traced([{"image": torch.zeros(3, 32, 32)}])


def test_custom_op_fake_kernel_shapes():
    tl, ts, mass = torch.ops.catseg.postprocess_topk(torch.empty(2, 5, 96, 96, device="meta"), 3, 336, 300, 96, 80, True)
    assert tl.shape == (2, 3, 336, 300) and tl.dtype == torch.int32 and tl.device.type == "meta"
    assert ts.shape == (2, 3, 336, 300) and ts.dtype == torch.float32 and ts.device.type == "meta"
    assert mass.shape == (2, 336, 300) and mass.dtype == torch.float32 and mass.device.type == "meta"


def test_torch_sort_is_the_ranking_the_kernel_is_held_to():
    """stable descending sort: NaNs first in index order, equal values in index order."""
    v = torch.tensor([1.0, float("nan"), 3.0, 3.0, float("inf"), float("nan"), -float("inf")])
    vals, idx = torch.sort(v, descending=True, stable=True)
    assert idx.tolist() == [1, 5, 4, 2, 3, 0, 6]


# ---------------------------------------------------------------- confidence_metrics
def _block(count, correct, conf_mean, hit, nan=0):
    q = [int(round(n * c * 16777216)) for n, c in zip(count, conf_mean)]
    return np.array(list(count) + list(correct) + q + list(hit) + [sum(count), nan], np.int64)


def test_metrics_of_a_perfectly_calibrated_table():
    # 4 bins, the mean confidence of each equals its accuracy (all exact in Q24)
    res = confidence_metrics(_block([8, 16, 4, 0], [1, 8, 3, 0], [0.125, 0.5, 0.75, 0.0], [12, 20]), 4, 2)
    assert res["ECE"] == 0.0 and res["MCE"] == 0.0
    assert res["pACC@1"] == pytest.approx(100 * 12 / 28) and res["pACC@2"] == pytest.approx(100 * 20 / 28)
    assert res["reliability"]["count"] == [8, 16, 4, 0] and math.isnan(res["reliability"]["accuracy"][3])
    assert res["reliability"]["accuracy"][:3] == [12.5, 50.0, 75.0] == res["reliability"]["confidence"][:3]
    assert res["coverage"] == [100.0, pytest.approx(100 * 20 / 28), pytest.approx(100 * 4 / 28), 0.0]
    assert res["selective-pACC"][:3] == [pytest.approx(100 * 12 / 28), pytest.approx(100 * 11 / 20), 75.0]
    assert math.isnan(res["selective-pACC"][3]) and res["nan-confidence"] == 0


def test_metrics_of_a_two_bin_table_by_hand():
    # bin 0: 30 pixels, 6 right (acc 0.2), mean confidence 0.25 -> gap 0.05; bin 1: 10 pixels, 9 right (acc 0.9),
    # mean confidence 0.75 -> gap 0.15.  ECE = 30/40 * 0.05 + 10/40 * 0.15 = 0.075, MCE = 0.15
    res = confidence_metrics(_block([30, 10], [6, 9], [0.25, 0.75], [15], nan=3), 2, 1)
    assert res["ECE"] == pytest.approx(7.5, abs=1e-9) and res["MCE"] == pytest.approx(15.0, abs=1e-9)
    assert res["pACC@1"] == pytest.approx(37.5) and res["nan-confidence"] == 3
    assert res["coverage"] == [100.0, 25.0] and res["selective-pACC"] == [pytest.approx(37.5), pytest.approx(90.0)]
    ref = CR.metrics(_block([30, 10], [6, 9], [0.25, 0.75], [15], nan=3), 2, 1)
    assert all(res[k] == pytest.approx(v, abs=1e-9) for k, v in ref.items())
    with pytest.raises(ValueError, match="counters"):
        confidence_metrics(np.zeros(9, np.int64), 2, 2)


def test_confidence_spec():
    assert confidence_spec({}) == {"bins": 15, "kind": "score", "topk": 2}
    assert confidence_spec({"bins": 10, "kind": "normalized", "topk": 4})["kind"] == "normalized"
    for bad in ({"bins": 0}, {"bins": 257}, {"kind": "softmax"}, {"topk": 5}, {"width": 3}, 15):
        with pytest.raises(ValueError, match="confidence"):
            confidence_spec(bad)


# ---------------------------------------------------------------- the restatement itself
def test_restatement_against_a_direct_histogram():
    """A 2 x 4 map worked by hand and with np.histogram: 4 bins, K = 2, 3 classes, clamp at 2."""
    gt = np.array([[0, 1, 2, 255], [1, 1, 0, 2]])
    top = np.array([[[0, 2, 5, 1], [1, 0, 0, 2]],            # rank 0 (5 folds to 2)
                    [[1, 1, 0, 0], [0, 1, 1, 1]]])           # rank 1
    conf = np.array([[0.0, 0.25, 0.6, 0.9], [1.0, np.nan, 1.5, -3.0]], np.float32)
    got = CR.counters(top, conf, gt, num_classes=3, clamp_pred=2, n_bins=4)
    live = np.array([1, 1, 1, 0, 1, 0, 1, 1], bool)          # the ignored pixel and the NaN one are out
    c = np.clip(np.nan_to_num(conf.reshape(-1)), 0, 1)[live]
    count, _ = np.histogram(c, bins=[0, 0.25, 0.5, 0.75, 1.0])          # the last bin is closed: 1.0 lands in bin 3
    assert got[:4].tolist() == count.tolist() == [2, 1, 1, 2]
    assert got[4:8].tolist() == [2, 0, 1, 2]                 # right at rank 0: pixels 0, 7 | - | 2 (folded) | 4, 6
    assert got[8:12].tolist() == [0, 1 << 22, int(np.rint(np.float32(0.6) * np.float32(16777216))), 2 << 24]
    assert got[12:14].tolist() == [5, 6]                     # pixel 1 is hit at rank 1 only
    assert got[14:].tolist() == [6, 1]
