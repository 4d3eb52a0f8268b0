"""Host half of the majority filter and the mode overviews: the numpy restatement (tests/mode_ref.py), which the GPU
tests hold the kernels to, against hand-worked maps, scipy's generic_filter and a np.unique loop; the kernels' logic
(csrc/mode_filter_logic.h) run sequentially on the host against the restatement (tools/mode_filter_host.cpp, built
with the address and undefined-behaviour sanitizers); the C ABI entries and their host-side argument checks; the
config keys, every ValueError of the two nodes and the traced refusal."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import mode_ref as M
from cat_seg import _lib as L
from cat_seg import build_model

from conftest import ROOT
from test_boundary_cpu import tiny_cfg

LABELS = {"MODEL.CATSEG_HIP.OUTPUT": "labels"}
SMOOTH = {**LABELS, "MODEL.CATSEG_HIP.SMOOTH.ENABLED": "True"}
# test_gpu_render.py's SCORES
SCORES = np.array([0.0, 0.5, 1.0, 1.5, -1.0, np.nan, 0.123, 0.999, np.inf, -np.inf, -0.0, 1e-30, 0.25], np.float32)


def blob_map(rng, H, W, labels=(0, 1, 2, 3, -1, 255, 8191), cell=5, speckle=0.03):
    """Coarse blobs of `labels` with speckle, label changes forced onto the tile borders of the filter kernel
    (x = 63 | 64, y = 15 | 16) and other labels in the four corners."""
    labels = np.asarray(labels, np.int32)
    coarse = rng.integers(0, len(labels), (H // cell + 1, W // cell + 1))
    m = labels[np.repeat(np.repeat(coarse, cell, 0), cell, 1)[:H, :W]]
    noise = rng.random((H, W)) < speckle
    m = np.where(noise, labels[rng.integers(0, len(labels), (H, W))], m).astype(np.int32)
    if W > 64:
        m[:, 64:] = np.where(m[:, 64:] == m[:, 63:64], labels[1], m[:, 64:])[:, :W - 64]
        m[::3, 63] = labels[2]
    if H > 16:
        m[16, ::2] = labels[3]
        m[15, 1::2] = labels[0]
    for (y, x), l in zip(((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)), (255, -1, 8191, 2)):
        m[y, x] = l
    return m


# ------------------------------------------------------------------ the restatement against hand answers
def test_weights_by_hand():
    s = np.array([[0.0, 0.5, 1.0, 1.5, -1.0, np.nan, np.inf, -np.inf, -0.0, 1e-30, 0.5 / 65536, 1.5 / 65536]], np.float32)
    lab = np.zeros(s.shape, np.int32)
    assert M.weights(lab, s).tolist() == [[0, 32768, 65536, 65536, 0, 0, 65536, 0, 0, 0, 0, 2]]   # halves to even
    assert M.weights(lab).tolist() == [[1] * 12]
    assert M.weights(np.array([[7, 3, 7]]), None, 7).tolist() == [[0, 1, 0]]


def test_a_tie_won_by_the_centre():
    # the window of the centre holds 3 x 1, 3 x 2, 3 x 5: all tied, the centre's own label 5 stays
    m = np.array([[1, 1, 1], [2, 5, 2], [5, 2, 5]], np.int32)
    assert M.mode_filter(m, 3)[1, 1] == 5
    m[1, 1] = 2                                      # now 2 has 4 votes
    assert M.mode_filter(m, 3)[1, 1] == 2


def test_a_tie_won_by_the_smallest_label():
    # the centre's own label 9 has 1 vote; 4 and -3 have 4 each: the smaller value wins
    m = np.array([[4, 4, -3], [4, 9, -3], [4, -3, -3]], np.int32)
    assert M.mode_filter(m, 3)[1, 1] == -3
    # clipped window of the corner (0, 0): 4, 4, 4, 9 -> 4
    assert M.mode_filter(m, 3)[0, 0] == 4


def test_half_keeps_a_pixel_without_a_majority():
    m = np.array([[1, 1, 1], [1, 9, 2], [2, 2, 3]], np.int32)     # 1 has 4 of 9 votes: a plurality, not more than half
    assert M.mode_filter(m, 3)[1, 1] == 1
    assert M.mode_filter(m, 3, rule="half")[1, 1] == 9
    m[2, 2] = 1                                                    # 5 of 9
    assert M.mode_filter(m, 3, rule="half")[1, 1] == 1
    # exactly half is not more than half: the corner window of (0, 0) in [[1, 2], [2, 1]]
    assert M.mode_filter(np.array([[3, 2], [2, 1]], np.int32), 3, rule="half")[0, 0] == 3


def test_a_window_without_votes_and_fill():
    m = np.full((5, 5), 7, np.int32)
    m[2, 2] = 4
    # nothing votes in the window of (0, 0) with novote 7 (only 4 at (2, 2) votes, out of reach of size 3)
    out = M.mode_filter(m, 3, novote_label=7, fill=True)
    assert out[0, 0] == 7 and out[1, 1] == 4 and out[2, 2] == 4 and out[4, 4] == 7
    assert np.array_equal(M.mode_filter(m, 3, novote_label=7, fill=False), m)        # rejected pixels stay rejected
    # the novote label never wins, however many pixels carry it
    assert M.mode_filter(m, 3, novote_label=7, fill=False)[2, 2] == 4
    assert M.mode_filter(m, 3)[2, 2] == 7
    # zero scores: no votes anywhere, the map stays
    assert np.array_equal(M.mode_filter(m, 5, score=np.zeros((5, 5), np.float32)), m)
    # weights decide: one pixel of weight 1 beats eight of weight 0.1
    s = np.full((5, 5), 0.1, np.float32)
    s[2, 2] = 1.0
    assert M.mode_filter(m, 3, score=s)[1, 1] == 4 and M.mode_filter(m, 3, score=s)[0, 0] == 7


def test_iterations_are_repeated_single_passes():
    rng = np.random.default_rng(3)
    m = blob_map(rng, 17, 23)
    once = M.mode_filter(m, 3)
    assert np.array_equal(M.mode_filter(m, 3, iterations=3), M.mode_filter(M.mode_filter(once, 3), 3))


@pytest.mark.parametrize("size", [3, 5])
def test_restatement_is_scipy_generic_filter(size):
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(size)

    def mode(win):
        c = int(win[len(win) // 2])
        v = win[win >= 0].astype(np.int64)
        lab, cnt = np.unique(v, return_counts=True)
        tied = lab[cnt == cnt.max()]
        return c if c in tied else tied[0]

    for H, W in ((1, 1), (1, 9), (9, 1), (7, 7), (17, 23)):
        m = blob_map(rng, H, W, labels=(0, 1, 2, 3, 9), cell=3, speckle=0.1) if min(H, W) > 1 else \
            rng.integers(0, 3, (H, W)).astype(np.int32)
        want = ndi.generic_filter(m.astype(np.float64), mode, size=size, mode="constant", cval=-1).astype(np.int32)
        assert np.array_equal(M.mode_filter(m, size), want), (H, W)


def test_overview_cells_against_np_unique():
    rng = np.random.default_rng(5)
    for (H, W), f in (((4, 5), 3), ((17, 23), 2), ((17, 23), 7), ((5, 9), 16), ((16, 64), 32)):
        m = blob_map(rng, H, W, cell=2, speckle=0.2)
        got = M.mode_overview(m, f)
        Ho, Wo = -(-H // f), -(-W // f)
        assert got["labels"].shape == (Ho, Wo)
        for Y in range(Ho):
            for X in range(Wo):
                lab, cnt = np.unique(m[Y * f:Y * f + f, X * f:X * f + f], return_counts=True)
                assert got["labels"][Y, X] == lab[cnt == cnt.max()][0]
                assert got["votes"][Y, X] == cnt.max() and got["total"][Y, X] == cnt.sum()
                assert got["share"][Y, X] == np.float32(cnt.max() / cnt.sum())
    # a cell without votes gets the novote label, votes 0 of 0 and a NaN share
    m = np.array([[7, 7, 1], [7, 7, 7]], np.int32)
    got = M.mode_overview(m, 2, novote_label=7)
    assert got["labels"].tolist() == [[7, 1]] and got["votes"].tolist() == [[0, 1]] and got["total"].tolist() == [[0, 1]]
    assert np.isnan(got["share"][0, 0]) and got["share"][0, 1] == 1.0


# ------------------------------------------------------------------ the kernels' logic on the host
def _case(rng, k, H, W):
    noise = k % 6 == 5
    m = rng.integers(-100, 100, (H, W)).astype(np.int32) if noise else blob_map(rng, H, W)
    score = rng.choice(SCORES, (H, W)).astype(np.float32) if k % 3 == 1 else None
    if k % 3 == 2:
        score = rng.random((H, W)).astype(np.float32)
    novote = (None, 255, 1)[(k // 2) % 3]
    return m, score, novote, bool((k // 3) % 2), ("plurality", "half")[(k // 4) % 2]


def write_case(path, op, k, m, score=None, novote=None, fill=False, rule="plurality", iterations=1):
    H, W = m.shape
    hdr = np.array([H, W, op, k, int(rule == "half"), int(score is not None), int(novote is not None),
                    0 if novote is None else novote, int(fill), iterations], np.int32)
    with open(path, "wb") as fh:
        fh.write(hdr.tobytes())
        fh.write(np.ascontiguousarray(m, np.int32).tobytes())
        if score is not None:
            fh.write(np.ascontiguousarray(score, np.float32).tobytes())


def test_kernel_logic_on_the_host_against_the_restatement(tmp_path):
    """tools/mode_filter_host.cpp: the functions the kernels call, pass by pass and sequentially, under the address
    and undefined-behaviour sanitizers, against the restatement.  A stand-alone program: nothing is loaded into this
    process."""
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "mode_filter_host")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "cat-seg_amd", "csrc"),
                    os.path.join(ROOT, "tools", "mode_filter_host.cpp"), "-o", exe], check=True)
    rng = np.random.default_rng(17)
    shapes = [(1, 1), (1, 70), (70, 1), (17, 23), (16, 64), (17, 65), (33, 40)]
    case, res = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")

    def run():
        r = subprocess.run([exe, case, res], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.startswith("ok"), (r.stdout[-2000:], r.stderr[-2000:])
        return np.fromfile(res, np.int32)

    for k in range(42):
        H, W = shapes[k % len(shapes)]
        m, score, novote, fill, rule = _case(rng, k, H, W)
        size, its = (3, 5, 15)[k % 3], (1, 3)[k % 7 == 3]
        write_case(case, 0, size, m, score, novote, fill, rule, its)
        want = M.mode_filter(m, size, its, rule, score, novote, fill)
        assert np.array_equal(run().reshape(H, W), want), (k, H, W, size, rule, novote, fill)
        f = (2, 3, 7, 16, 32)[k % 5]
        write_case(case, 1, f, m, score, novote)
        want = M.mode_overview(m, f, score, novote)
        got = run().reshape(3, *want["labels"].shape)
        for i, name in enumerate(("labels", "votes", "total")):
            assert np.array_equal(got[i], want[name]), (k, H, W, f, name)


# ------------------------------------------------------------------ the C ABI
NEW = ("catseg_mode_filter", "catseg_mode_overview")


def test_header_library_and_binding_declare_the_new_entries():
    text = open(os.path.join(ROOT, "include", "catseg_hip_mode.h")).read()
    assert '#include "catseg_hip_mode.h"' in open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    assert "struct" not in text and "enum" not in text
    assert L.MODE_HEADERS == ("catseg_hip_mode.h",) and set(L.EXPORTED_MODE) == set(NEW)
    lib = L.load()
    for name in NEW:
        assert getattr(lib, name).restype is not None and name not in L.EXPORTED


def _filter(lib, **kw):
    a = dict(labels=0x1000, H=8, W=8, ld=8, size=3, rule=0, score=None, ld_score=0, has_novote=0, novote=0, fill=0,
             out=0x100000, ld_out=8)
    a.update(kw)
    return lib.catseg_mode_filter(a["labels"], a["H"], a["W"], a["ld"], a["size"], a["rule"], a["score"], a["ld_score"],
                                  a["has_novote"], a["novote"], a["fill"], a["out"], a["ld_out"], None)


def _overview(lib, **kw):
    a = dict(labels=0x1000, H=8, W=8, ld=8, factor=2, score=None, ld_score=0, out=0x100000, votes=0x200000,
             total=0x300000)
    a.update(kw)
    return lib.catseg_mode_overview(a["labels"], a["H"], a["W"], a["ld"], a["factor"], a["score"], a["ld_score"], 0, 0,
                                    a["out"], a["votes"], a["total"], None)


@pytest.mark.parametrize("bad, text", [
    (dict(labels=None), "null pointer"), (dict(out=None), "null pointer"),
    (dict(H=0), "1 .. 16384"), (dict(W=16385, ld=16385, ld_out=16385), "1 .. 16384"),
    (dict(size=1), "odd, 3 .. 15"), (dict(size=4), "odd, 3 .. 15"), (dict(size=17), "odd, 3 .. 15"),
    (dict(ld=7), "row stride"), (dict(ld_out=7), "row stride"), (dict(score=0x2000, ld_score=7), "row stride"),
    (dict(labels=0x1002), "misaligned"), (dict(score=0x2001, ld_score=8), "misaligned"),
    (dict(out=0x1000), "overlaps"), (dict(out=0x1004), "overlaps"),
    (dict(ld=16, ld_out=16, out=0x1000 + 4 * 4), "overlaps"),          # columns 4 .. 11 of the same rows
])
def test_mode_filter_rejects_bad_arguments_before_any_launch(bad, text):
    lib = L.load()
    assert _filter(lib, **bad) == -1
    assert text in lib.catseg_last_error().decode()


@pytest.mark.parametrize("bad, text", [
    (dict(labels=None), "null pointer"), (dict(votes=None), "null pointer"), (dict(total=None), "null pointer"),
    (dict(H=16385), "1 .. 16384"), (dict(W=0), "1 .. 16384"),
    (dict(factor=1), "2 .. 32"), (dict(factor=33), "2 .. 32"),
    (dict(ld=7), "row stride"), (dict(score=0x2000, ld_score=3), "row stride"),
    (dict(out=0x100001), "misaligned"),
])
def test_mode_overview_rejects_bad_arguments_before_any_launch(bad, text):
    lib = L.load()
    assert _overview(lib, **bad) == -1
    assert text in lib.catseg_last_error().decode()


# ------------------------------------------------------------------ the config nodes
def test_config_keys_and_defaults():
    s, o = tiny_cfg().MODEL.CATSEG_HIP.SMOOTH, tiny_cfg().MODEL.CATSEG_HIP.OVERVIEW
    assert (s.ENABLED, s.SIZE, s.ITERATIONS, s.RULE, s.WEIGHT, s.REJECT) == (False, 3, 1, "plurality", "count", "keep")
    assert (tuple(o.FACTORS), o.WEIGHT) == ((), "count")
    m = build_model(tiny_cfg())
    assert m.smooth is False and m.overview_factors == () and m._reject_label() is None
    m = build_model(tiny_cfg(**SMOOTH, **{"MODEL.CATSEG_HIP.SMOOTH.SIZE": "7", "MODEL.CATSEG_HIP.SMOOTH.ITERATIONS": "2",
                                          "MODEL.CATSEG_HIP.SMOOTH.RULE": "half", "MODEL.CATSEG_HIP.SMOOTH.WEIGHT": "score",
                                          "MODEL.CATSEG_HIP.SMOOTH.REJECT": "fill",
                                          "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(2, 8)",
                                          "MODEL.CATSEG_HIP.OVERVIEW.WEIGHT": "score"}))
    assert (m.smooth, m.smooth_size, m.smooth_iterations, m.smooth_rule, m.smooth_weight, m.smooth_reject) == \
        (True, 7, 2, "half", "score", "fill")
    assert m.overview_factors == (2, 8) and m.overview_weight == "score"
    # the reject label of CONFIDENCE is the label that casts no votes
    m = build_model(tiny_cfg(**SMOOTH, **{"MODEL.CATSEG_HIP.CONFIDENCE.ENABLED": "True",
                                          "MODEL.CATSEG_HIP.CONFIDENCE.MIN_SCORE": "0.5",
                                          "MODEL.CATSEG_HIP.CONFIDENCE.REJECT_LABEL": "3"}))
    assert m._reject_label() == 3


@pytest.mark.parametrize("keys, text", [
    ({"MODEL.CATSEG_HIP.SMOOTH.ENABLED": "True"}, "SMOOTH filters the label map of MODEL.CATSEG_HIP.OUTPUT 'labels'"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.SIZE": "4"}, "SMOOTH.SIZE"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.SIZE": "17"}, "SMOOTH.SIZE"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.SIZE": "1"}, "SMOOTH.SIZE"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.ITERATIONS": "0"}, "SMOOTH.ITERATIONS"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.ITERATIONS": "9"}, "SMOOTH.ITERATIONS"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.RULE": "majority"}, "SMOOTH.RULE"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.WEIGHT": "area"}, "SMOOTH.WEIGHT"),
    ({**SMOOTH, "MODEL.CATSEG_HIP.SMOOTH.REJECT": "drop"}, "SMOOTH.REJECT"),
    ({"MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(2,)"}, "OVERVIEW reduces the label map of MODEL.CATSEG_HIP.OUTPUT 'labels'"),
    ({**LABELS, "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(1,)"}, "OVERVIEW.FACTORS"),
    ({**LABELS, "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(2, 33)"}, "OVERVIEW.FACTORS"),
    ({**LABELS, "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(4, 4)"}, "OVERVIEW.FACTORS"),
    ({**LABELS, "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(2,)", "MODEL.CATSEG_HIP.OVERVIEW.WEIGHT": "area"},
     "OVERVIEW.WEIGHT"),
])
def test_every_value_error_of_the_two_nodes(keys, text):
    with pytest.raises(ValueError, match=text):
        build_model(tiny_cfg(**keys))


def test_traced_forward_refuses():
    for keys in (SMOOTH, {**LABELS, "MODEL.CATSEG_HIP.OVERVIEW.FACTORS": "(2,)"}):
        with pytest.raises(RuntimeError, match="cannot be traced"):
            build_model(tiny_cfg(**keys))._forward_traced([{"image": torch.zeros(3, 32, 32)}])
