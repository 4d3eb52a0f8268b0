"""The device-side test-time-augmentation merge without a GPU: the ABI (header, library export, ctypes
mirror), the host-side argument checks of catseg_postprocess_tta (all run before any launch), the
MODEL.CATSEG_HIP.TTA_MERGE key, the wrapper's construction matrix and the operators' fake kernels."""
import ctypes
import os

import pytest
import torch

from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg import custom_ops  # noqa: F401  (registers torch.ops.catseg.*)

from conftest import ROOT
from test_boundary_cpu import tiny_cfg

NAME = "catseg_postprocess_tta"


def test_header_library_and_mirror_declare_the_entry():
    header = open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    assert f"int {NAME}(" in header
    assert NAME in L.EXPORTED
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    assert L.load().catseg_abi_version() == 1
    doc = header[: header.index(f"int {NAME}(")].rsplit("/*", 1)[1]
    assert "test_time_augmentation.py:81-108" in doc
    assert "cat_seg_model.py:222-227" in doc and "plain_train_net.py:107-116" in doc


def _tta(lib, *, logits=16, K=2, T=5, h=8, w=8, views=((8, 8, 0), (8, 8, 1)), probs=16, labels=0, score=0, H=16, W=16):
    flat = [e for v in views for e in v] if views is not None else []
    table = (ctypes.c_int32 * max(len(flat), 1))(*flat)
    vptr = ctypes.cast(table, ctypes.c_void_p) if views is not None else None
    return lib.catseg_postprocess_tta(logits, K, T, h, w, vptr, probs, labels, score, H, W, None)


BAD = [
    pytest.param({"K": 0, "views": ()}, id="K0"),
    pytest.param({"K": 33, "views": ((8, 8, 0),) * 33}, id="K33"),
    pytest.param({"logits": 0}, id="null-logits"),
    pytest.param({"views": None}, id="null-views"),
    pytest.param({"probs": 0, "labels": 0}, id="no-output"),
    pytest.param({"probs": 16, "labels": 0, "score": 16}, id="score-without-labels"),
    pytest.param({"views": ((8, 8, 0), (8, 9, 1))}, id="crop_w-too-wide"),
    pytest.param({"views": ((8, 8, 0), (0, 8, 1))}, id="crop_h-zero"),
    pytest.param({"views": ((8, 8, 2), (8, 8, 1))}, id="flip-2"),
    pytest.param({"H": 0}, id="H0"),
    pytest.param({"W": -3}, id="W-negative"),
    pytest.param({"T": 0}, id="T0"),
    pytest.param({"probs": 18}, id="misaligned-probs"),
    pytest.param({"probs": 0, "labels": 16, "score": 6}, id="misaligned-score"),
    pytest.param({"H": 16 * 65536}, id="grid"),
]


@pytest.mark.parametrize("bad", BAD)
def test_rejects_bad_arguments_before_any_launch(bad):
    lib = L.load()
    assert _tta(lib, **bad) == -1
    assert lib.catseg_last_error().startswith(b"postprocess_tta:")


def test_messages_name_the_view():
    lib = L.load()
    assert _tta(lib, views=((8, 8, 0), (8, 9, 1))) == -1
    assert b"view 1" in lib.catseg_last_error()
    assert _tta(lib, views=((8, 8, 2), (8, 8, 1))) == -1
    assert b"view 0" in lib.catseg_last_error()


def test_rejects_a_patch_that_does_not_fit_lds():
    """Downsampling 640 -> 64 in the second view: the same rule and wording as catseg_postprocess_argmax."""
    lib = L.load()
    assert _tta(lib, h=640, w=640, views=((64, 64, 0), (640, 640, 1)), H=64, W=64) == -1
    err = lib.catseg_last_error()
    assert err.startswith(b"postprocess_tta:") and b"LDS" in err and b"view 1" in err


def test_tta_merge_config_key():
    assert tiny_cfg().MODEL.CATSEG_HIP.TTA_MERGE == "host"


def _sliding_cfg(**over):
    return tiny_cfg(**{"TEST.SLIDING_WINDOW": "True"}, **over)


def test_wrapper_construction_matrix():
    from cat_seg import SemanticSegmentorWithTTA       # the exported wrapper, as train_net.py imports it
    dev, lab = {"MODEL.CATSEG_HIP.TTA_MERGE": "device"}, {"MODEL.CATSEG_HIP.OUTPUT": "labels"}

    def wrap(cfg):
        return SemanticSegmentorWithTTA(cfg, build_model(cfg))

    assert wrap(tiny_cfg()).tta_merge == "host"
    with pytest.raises(ValueError, match="probabilities"):
        wrap(tiny_cfg(**lab))
    assert wrap(tiny_cfg(**dev)).tta_merge == "device"
    assert wrap(tiny_cfg(**dev, **lab)).tta_merge == "device"
    with pytest.raises(ValueError, match="SLIDING_WINDOW"):
        wrap(_sliding_cfg(**dev))
    wrap(_sliding_cfg())                               # host + sliding window wraps as before
    with pytest.raises(ValueError, match="TTA_MERGE"):
        wrap(tiny_cfg(**{"MODEL.CATSEG_HIP.TTA_MERGE": "bogus"}))


def test_custom_op_fake_kernel_shapes():
    lg = torch.empty(3, 5, 96, 96, device="meta")
    args = (336, 300, [96, 80, 96], [96, 96, 72], [0, 1, 0])
    p = torch.ops.catseg.postprocess_tta(lg, *args)
    assert p.shape == (5, 336, 300) and p.dtype == torch.float32 and p.device.type == "meta"
    lab, sc = torch.ops.catseg.postprocess_tta_argmax(lg, *args)
    assert lab.shape == (336, 300) and lab.dtype == torch.int32 and lab.device.type == "meta"
    assert sc.shape == (336, 300) and sc.dtype == torch.float32 and sc.device.type == "meta"
