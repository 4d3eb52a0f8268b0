"""Host half of the boundary-aware evaluation: the numpy restatement (tests/boundary_ref.py), which the GPU tests
hold the kernels to, against scipy's binary erosion (the published per-class method), the definition by brute force
and hand answers; `boundary_metrics` on hand-made counters with its NaN cases and identities; the C ABI entries and
their host-side argument checks; the evaluator's `boundary=` argument; and the kernels' logic
(csrc/boundary_eval_logic.h) run sequentially on the host against the brute-force definition
(tools/boundary_eval_host.cpp, built with the address and undefined-behaviour sanitizers)."""
import math
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import boundary_ref as B
from cat_seg import _lib as L
from cat_seg.evaluation import (SemSegEvaluator, VOCbEvaluator, boundary_metrics, boundary_specs, boundary_widths,
                                semseg_metrics)

from conftest import ROOT
from test_region_outlines_cpu import random_map

SHAPES = [(1, 1), (1, 9), (9, 1), (7, 7), (34, 25)]
CAPS = (1, 2, 5, 30)


def speckled(seed, H, W, nlab=3):
    rng = np.random.default_rng(seed)
    m = random_map(rng, H, W, nlab)
    return np.where(rng.random((H, W)) < 0.02, rng.integers(0, nlab, (H, W)), m)


# ------------------------------------------------------------------ the restatement against scipy and brute force
@pytest.mark.parametrize("H,W", SHAPES)
def test_restatement_is_the_per_label_erosion(H, W):
    """D(p) <= k exactly when p is in its class mask but not in the mask eroded k times (3 x 3 ones, zero border):
    mask_to_boundary of the published Boundary IoU code."""
    ndi = pytest.importorskip("scipy.ndimage")
    for seed in range(3):
        m = speckled(100 * H + W + seed, H, W)
        for cap in CAPS:
            D = B.distance(m, cap)
            assert D.dtype == np.int16 and D.shape == (H, W) and D.min() >= 1 and D.max() <= cap
            for lab in np.unique(m):
                mask = m == lab
                for k in range(1, cap):
                    er = ndi.binary_erosion(mask, np.ones((3, 3)), iterations=k, border_value=0)
                    assert np.array_equal(mask & ~er, mask & (D <= k)), (lab, k, cap)


@pytest.mark.parametrize("H,W", SHAPES + [(12, 40)])
def test_restatement_is_the_definition(H, W):
    m = speckled(7 * H + W, H, W, 4)
    for cap in CAPS:
        assert np.array_equal(B.distance(m, cap), B.distance_bruteforce(m, cap))
        assert np.array_equal(B.distance(m, cap, clamp_pred=2), B.distance_bruteforce(np.minimum(m, 2), cap))


def test_hand_answers():
    assert B.distance([[7]], 5).tolist() == [[1]]
    u = B.distance(np.full((9, 13), 3), 30)
    assert u.max() == 5 == (min(9, 13) + 1) // 2
    assert (u[0] == 1).all() and (u[-1] == 1).all() and (u[:, 0] == 1).all() and (u[:, -1] == 1).all()
    assert u[4].tolist() == [1, 2, 3, 4, 5, 5, 5, 5, 5, 4, 3, 2, 1]
    assert (B.distance(np.full((9, 13), 3), 3) == np.minimum(u, 3)).all()                 # the cap
    yy, xx = np.mgrid[:6, :7]
    assert (B.distance((yy + xx) % 2, 30) == 1).all()                                      # a checkerboard
    split = np.array([[0, 0, 0, 0, 1, 1, 1]] * 5)       # two labels split by a vertical line between x = 3 and 4
    assert B.distance(split, 30).tolist() == [[1, 1, 1, 1, 1, 1, 1],
                                              [1, 2, 2, 1, 1, 2, 1],
                                              [1, 2, 2, 1, 1, 2, 1],
                                              [1, 2, 2, 1, 1, 2, 1],
                                              [1, 1, 1, 1, 1, 1, 1]]
    wild = np.array([[-1, -1, 255], [-1, -1, 255], [-2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1]])
    assert (B.distance(wild, 30) == 1).all()
    assert B.distance(np.array([[0, 1, 2, 3, 4]] * 3), 9, clamp_pred=2).tolist() == [[1] * 5, [1, 1, 1, 2, 1], [1] * 5]


# ------------------------------------------------------------------ the metrics
NAMES = ["a", "b", "c"]


def hand_case():
    rng = np.random.default_rng(3)
    G = random_map(rng, 30, 41, 3)
    G[3:8, 5:15] = 255
    P = np.roll(G, (2, 1), (0, 1))
    P[P == 255] = 1
    return P, G


def test_metrics_on_hand_made_counters():
    n, n1 = 3, 4
    per = B.counters_per_width(n)
    conf = np.zeros((n1, n1), np.int64)
    conf[:3, :3] = [[50, 4, 0], [6, 30, 0], [0, 0, 0]]                # class c has no ground truth
    conf[0, 3] = 9                                                    # ignored pixels predicted a
    band = np.zeros((n1, n1), np.int64)
    band[:3, :3] = [[10, 4, 0], [5, 8, 0], [0, 0, 0]]
    c = np.zeros(2 * per, np.int64)                                   # width 0 as above, width 1 an empty band
    c[:16] = band.ravel()
    c[16:19], c[19:22], c[22:25] = [6, 5, 0], [15, 12, 0], [12, 10, 0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = boundary_metrics(conf, c, NAMES, ["3px", "1px"])
    assert m["BIoU@3px-a"] == 100 * 6 / (15 + 12 - 6) and m["BIoU@3px-b"] == 100 * 5 / (12 + 10 - 5)
    assert math.isnan(m["BIoU@3px-c"])
    assert m["mBIoU@3px"] == pytest.approx((m["BIoU@3px-a"] + m["BIoU@3px-b"]) / 2, rel=1e-15)
    assert m["trimap-pACC@3px"] == 100 * 18 / 27
    assert m["trimap-mIoU@3px"] == pytest.approx(100 * (10 / 19 + 8 / 17) / 2, rel=1e-15)
    er = conf - band                                                  # [[40, 0], [1, 22]]
    assert m["eroded-pACC@3px"] == 100 * 62 / 63
    assert m["eroded-mIoU@3px"] == pytest.approx(100 * (40 / 41 + 22 / 23) / 2, rel=1e-15)
    assert m["eroded-mF1@3px"] == pytest.approx(100 * (80 / 81 + 44 / 45) / 2, rel=1e-15)
    assert m["eroded-mIoU@3px"] == semseg_metrics(er, NAMES)["mIoU"]
    # the empty band: NaN for its own metrics, the eroded map is the whole map
    for k in ("mBIoU@1px", "BIoU@1px-a", "trimap-mIoU@1px", "trimap-pACC@1px"):
        assert math.isnan(m[k]), k
    assert m["eroded-mIoU@1px"] == semseg_metrics(conf, NAMES)["mIoU"]
    assert m["eroded-pACC@1px"] == semseg_metrics(conf, NAMES)["pACC"]
    # the band that is the whole map: the eroded map is empty
    full = np.zeros(per, np.int64)
    full[:16] = conf.ravel()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m = boundary_metrics(conf, full, NAMES, ["9px"])
    assert all(math.isnan(m[k]) for k in ("eroded-mIoU@9px", "eroded-pACC@9px", "eroded-mF1@9px", "mBIoU@9px"))
    assert m["trimap-mIoU@9px"] == semseg_metrics(conf, NAMES)["mIoU"]
    ref = B.metrics(conf, c, NAMES, ["3px", "1px"])
    got = boundary_metrics(conf, c, NAMES, ["3px", "1px"])
    assert list(ref) == list(got)
    for k in ref:
        assert (math.isnan(ref[k]) and math.isnan(got[k])) or got[k] == pytest.approx(ref[k], rel=1e-12), k
    with pytest.raises(ValueError):
        boundary_metrics(conf, c[:-1], NAMES, ["3px", "1px"])


def test_counter_identities_of_the_restatement():
    P, G = hand_case()
    widths = [1, 3, 40]
    conf, invalid = B.confusion(P, G, 3)
    assert invalid == 0
    c = B.counters(P, G, widths, 3)
    for w, (band, inter, gt_band, pred_band) in zip(widths, B.split(c, 3, 3)):
        assert (band >= 0).all() and (conf - band >= 0).all()                     # conf = band + eroded
        assert (inter <= np.minimum(gt_band, pred_band)).all()
        assert (gt_band == band[:, :3].sum(0)).all()
    assert (B.split(c, 3, 3)[2][0] == conf).all()                                 # width 40 covers the 30 x 41 map
    same = B.counters(G, G, widths, 3)
    m = B.metrics(B.confusion(G, G, 3)[0], same, NAMES, ["1px", "3px", "40px"])
    for t in ("1px", "3px", "40px"):
        assert all(m[f"BIoU@{t}-{n}"] == 100 for n in NAMES) and m[f"mBIoU@{t}"] == 100
    # a ground-truth label that is neither a class nor the ignore label is skipped, not binned
    G2 = G.copy()
    G2[0, 0] = 77
    band2 = B.split(B.counters(P, G2, [3], 3), 3, 1)[0][0]
    assert band2.sum() == ((B.distance(G2, 4) <= 3) & (G2 != 77)).sum() and B.confusion(P, G2, 3)[1] == 1


# ------------------------------------------------------------------ the C ABI
NEW = ("catseg_boundary_distance_workspace", "catseg_boundary_distance", "catseg_boundary_confusion")


def test_header_and_lib_carry_the_symbols():
    text = open(os.path.join(ROOT, "include", "catseg_hip_boundary.h")).read()
    declared = set(re.findall(r"\b(catseg_\w+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    assert declared == set(NEW) == set(L.EXPORTED_EXTENSIONS)
    assert L.EXTENSION_HEADERS == ("catseg_hip_boundary.h",)
    assert not set(NEW) & (set(L.EXPORTED) | set(L.EXPORTED_INCLUDED))
    assert '#include "catseg_hip_boundary.h"' in open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    lib = L.load()
    for s in NEW:
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s


def test_workspace_and_argument_checks_without_gpu():
    """The host-side checks return before anything is launched: bad arguments are refused without a device."""
    import ctypes as C
    lib = L.load()
    ws = lib.catseg_boundary_distance_workspace
    assert ws(0, 5, 4) == 0 and ws(5, 0, 4) == 0 and ws(16385, 5, 4) == 0 and ws(5, 16385, 4) == 0
    assert ws(5, 5, 0) == 0 and ws(5, 5, 16385) == 0
    assert ws(16384, 16384, 16384) == 2 * 16384 * 16384 and ws(3, 5, 2) == 32 and ws(70, 100, 7) == 14000
    p = 1 << 20                                     # an aligned non-null address, never dereferenced on these paths
    nb = ws(8, 8, 4)
    good = (p, 8, 8, 8, -1, 4, p, 8, p, nb, None)
    bad = lambda i, v: lib.catseg_boundary_distance(*(good[:i] + (v,) + good[i + 1:]))
    assert bad(0, None) == -1 and bad(6, None) == -1 and bad(8, None) == -1        # null pointers
    assert bad(3, 7) == -1 and bad(7, 7) == -1                                      # ld < W, ld_dist < W
    assert b"stride" in lib.catseg_last_error()
    assert bad(1, 0) == -1 and bad(2, 0) == -1 and bad(1, 16385) == -1 and bad(2, 16385) == -1
    assert b"16384" in lib.catseg_last_error()
    assert bad(5, 0) == -1 and bad(5, 16385) == -1                                  # cap
    assert b"cap" in lib.catseg_last_error()
    assert bad(9, nb - 2) == -1                                                     # workspace too small
    assert b"workspace" in lib.catseg_last_error()
    assert bad(0, p + 2) == -1 and bad(6, p + 1) == -1                              # misaligned map / result
    w = (C.c_int * 8)(1, 2, 3, 5, 8, 13, 21, 34)
    good = (p, p, p, p, 8, 8, 5, 255, -1, w, 8, p, None)
    bad = lambda i, v: lib.catseg_boundary_confusion(*(good[:i] + (v,) + good[i + 1:]))
    for i in (0, 1, 2, 3, 9, 11):
        assert bad(i, None) == -1, i                                                # null pointers
    assert bad(4, 0) == -1 and bad(5, 0) == -1 and bad(4, 16385) == -1 and bad(5, 16385) == -1
    assert bad(6, 0) == -1                                                          # no classes
    assert bad(10, 0) == -1 and bad(10, 9) == -1                                    # K
    assert b"K" in lib.catseg_last_error()
    assert bad(9, (C.c_int * 8)(1, 2, 0, 5, 8, 13, 21, 34)) == -1                   # a width of 0
    assert b"width" in lib.catseg_last_error()
    assert bad(9, (C.c_int * 8)(1, 2, 16384, 5, 8, 13, 21, 34)) == -1
    assert bad(11, p + 4) == -1                                                     # misaligned counters
    assert b"misaligned" in lib.catseg_last_error()


# ------------------------------------------------------------------ the evaluator argument
def test_evaluator_specs_and_tags():
    specs = boundary_specs([("ratio", 0.02), ("px", 3), ["px", 1]])
    assert [s[2] for s in specs] == ["0.02d", "3px", "1px"]
    assert boundary_widths(specs, 2048, 3072) == [74, 3, 1]                         # round(0.02 * 3692.07)
    assert boundary_widths(specs, 5, 5) == [1, 3, 1]                                # a ratio is at least one pixel
    assert boundary_widths(specs, 100, 75) == [B.ratio_width(0.02, 100, 75), 3, 1] == [2, 3, 1]   # 2.5 rounds to even
    assert boundary_specs([("ratio", 0.005)])[0][2] == "0.005d"
    ev = SemSegEvaluator(class_names=NAMES, device="cpu", distributed=False, boundary=[("ratio", 0.02), ("px", 3)])
    assert ev.boundary_tags == ["0.02d", "3px"]
    assert ev._bcounters.numel() == 2 * B.counters_per_width(3) and ev._bcounters.dtype.is_floating_point is False
    assert VOCbEvaluator(class_names=NAMES, device="cpu", boundary=(("px", 2),)).boundary_tags == ["2px"]
    plain = SemSegEvaluator(class_names=NAMES, device="cpu")
    assert plain.boundary_tags == [] and not hasattr(plain, "_bcounters")
    for bad in ([], "px", 3, [("px", 0)], [("px", 2.5)], [("px", 16384)], [("ratio", 0)], [("ratio", 1.0)],
                [("ratio", float("nan"))], [("disk", 3)], [("px",)], [3], [("px", "3")], [("px", True)],
                [("px", 3), ("px", 3)], [("px", i + 1) for i in range(9)]):
        with pytest.raises(ValueError):
            SemSegEvaluator(class_names=NAMES, device="cpu", boundary=bad)


# ------------------------------------------------------------------ the kernels' logic on the host
def test_kernel_logic_on_the_host_against_brute_force(tmp_path):
    """tools/boundary_eval_host.cpp: the functions the kernels call, pass by pass and sequentially, against the
    brute-force definition, under the address and undefined-behaviour sanitizers.  A stand-alone program: nothing
    is loaded into this process."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "boundary_eval_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "boundary_eval_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().startswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])
