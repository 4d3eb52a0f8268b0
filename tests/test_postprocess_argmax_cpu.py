"""The label-map output mode without a GPU: the ABI (header, library exports, ctypes mirror), the host-side
argument checks of catseg_postprocess_argmax / catseg_semseg_confusion_labels (they run before any
launch), the MODEL.CATSEG_HIP.OUTPUT key, the custom op's fake kernel, and the TTA wrapper's refusal."""
import ctypes
import os

import pytest
import torch

from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg import custom_ops  # noqa: F401  (registers torch.ops.catseg.*)

from conftest import ROOT
from test_boundary_cpu import tiny_cfg

NEW = ("catseg_postprocess_argmax", "catseg_semseg_confusion_labels")


def test_header_library_and_mirror_declare_the_new_entries():
    header = open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert f"int {name}(" in header
        assert name in L.EXPORTED
        assert hasattr(lib, name)
    assert L.load().catseg_abi_version() == 1
    # each cites what it replaces
    for name in NEW:
        doc = header[: header.index(f"int {name}(")].rsplit("/*", 1)[1]
        assert "cat_seg_model.py:222-227" in doc and "plain_train_net.py:107-116" in doc


def _argmax(lib, *, logits=16, B=1, T=5, h=8, w=8, ch=8, cw=8, sigmoid=1, labels=16, score=0, H=16, W=16):
    return lib.catseg_postprocess_argmax(logits, B, T, h, w, ch, cw, sigmoid, labels, score, H, W, None)


@pytest.mark.parametrize("bad", [{"labels": 0}, {"logits": 0}, {"T": 0}, {"B": 0}, {"cw": 9}, {"ch": 0}, {"H": 0},
                                 {"W": -3}, {"B": 1 << 20}])
def test_postprocess_argmax_rejects_bad_arguments_before_any_launch(bad):
    lib = L.load()
    assert _argmax(lib, **bad) == -1
    assert lib.catseg_last_error().startswith(b"postprocess_argmax:")


def test_postprocess_argmax_rejects_a_patch_that_does_not_fit_lds():
    """Downsampling 640 -> 64: the source patch of one output tile is far beyond the LDS stage; the entry
    says so instead of taking another path."""
    lib = L.load()
    assert _argmax(lib, h=640, w=640, ch=640, cw=640, H=64, W=64) == -1
    err = lib.catseg_last_error()
    assert err.startswith(b"postprocess_argmax:") and b"LDS" in err


def test_confusion_labels_rejects_bad_arguments_before_any_launch():
    lib = L.load()
    f = lib.catseg_semseg_confusion_labels
    assert f(0, 4, 4, 16, 3, 255, -1, 16, 16, None) == -1
    assert lib.catseg_last_error().startswith(b"semseg_confusion_labels:")
    assert f(16, 4, 0, 16, 3, 255, -1, 16, 16, None) == -1
    assert f(16, 4, 4, 16, 3, 255, -1, 20, 16, None) == -1          # conf not 8-byte aligned
    assert b"misaligned" in lib.catseg_last_error()


def test_output_config_key():
    assert tiny_cfg().MODEL.CATSEG_HIP.OUTPUT == "probs"
    assert build_model(tiny_cfg()).output == "probs"
    assert build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "labels"})).output == "labels"
    with pytest.raises(ValueError, match="OUTPUT"):
        build_model(tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "bogus"}))


def test_custom_op_fake_kernel_shapes():
    lab, sc = torch.ops.catseg.postprocess_argmax(torch.empty(2, 5, 96, 96, device="meta"), 336, 300, 96, 80, True)
    assert lab.shape == (2, 336, 300) and lab.dtype == torch.int32 and lab.device.type == "meta"
    assert sc.shape == (2, 336, 300) and sc.dtype == torch.float32 and sc.device.type == "meta"


def test_tta_refuses_a_labels_model():
    from cat_seg import SemanticSegmentorWithTTA       # the exported wrapper, as train_net.py imports it
    from cat_seg import test_time_augmentation as TTA
    assert issubclass(SemanticSegmentorWithTTA, TTA.SemanticSegmentorWithTTA)
    cfg = tiny_cfg(**{"MODEL.CATSEG_HIP.OUTPUT": "labels"})
    with pytest.raises(ValueError, match="probabilities"):
        SemanticSegmentorWithTTA(cfg, build_model(cfg))
    SemanticSegmentorWithTTA(tiny_cfg(), build_model(tiny_cfg()))     # a probs model wraps as before
