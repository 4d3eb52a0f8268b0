"""Host half of the device RLE path (cat_seg.evaluation): the per-label COCO RLEs assembled from the
column-major label runs of a map equal `coco_rle_encode(map == label)` and the oracle's loop restatement
(oracle/semseg_eval.py) for every label, the split of `coco_rle_encode` leaves its results as they were,
and the C ABI carries the catseg_label_runs_* entries, whose host-side checks refuse bad arguments
without a device."""
import os
import re

import numpy as np
import pytest

from cat_seg import _lib as L
from cat_seg.evaluation import (SemSegEvaluator, coco_rle_encode, rle_counts_to_string, rle_mask_counts,
                                rle_records_from_runs)
from oracle import semseg_eval as OE

from conftest import ROOT


def numpy_runs(m, clamp_pred=-1):
    """(run_start, run_label) of fold(m).ravel(order="F"): the definition the kernel is held to."""
    m = np.asarray(m).astype(np.int64)
    if clamp_pred >= 0:
        m = np.where(m >= clamp_pred, clamp_pred, m)
    flat = m.ravel(order="F")
    start = np.concatenate(([0], np.flatnonzero(flat[1:] != flat[:-1]) + 1))
    return start.astype(np.int32), flat[start].astype(np.int32)


def _alternating(shape):
    return (np.arange(shape[0] * shape[1]) % 2).reshape(shape[1], shape[0]).T.copy()


def _maps():
    rng = np.random.default_rng(5)
    wrap = rng.integers(0, 4, (9, 7))
    wrap[0, 0] = wrap[-1, -1] = 3                          # the first pixel's label also ends the sequence
    wrap[1, 0] = 2
    yy, xx = np.mgrid[:64, :64]
    return {"1x1": np.array([[7]]), "6x1": _alternating((6, 1)), "1x6": _alternating((1, 6)),
            "constant": np.full((13, 17), 4), "checkerboard": (yy + xx) % 2,
            "random150": rng.integers(0, 150, (97, 131)), "first_label_ends": wrap}


@pytest.mark.parametrize("name", list(_maps()))
def test_records_from_runs_equal_mask_encoding(name):
    m = _maps()[name]
    H, W = m.shape
    recs = rle_records_from_runs(*numpy_runs(m), H, W)
    assert [l for l, _ in recs] == np.unique(m).tolist()
    for label, rle in recs:
        mask = m == label
        assert rle == coco_rle_encode(mask), (name, label)
        assert rle == OE.rle_encode(mask), (name, label)
        assert np.array_equal(OE.rle_decode(rle), mask.astype(np.uint8)), (name, label)


def test_records_from_runs_negative_and_extreme_labels():
    m = np.array([[-2 ** 31, -1, 0], [2 ** 31 - 1, -1, -2 ** 31]], np.int64)
    recs = rle_records_from_runs(*numpy_runs(m), 2, 3)
    assert [l for l, _ in recs] == [-2 ** 31, -1, 0, 2 ** 31 - 1]
    for label, rle in recs:
        assert rle == OE.rle_encode(m == label)


def test_records_from_runs_refuses_runs_that_do_not_start_the_map():
    with pytest.raises(ValueError):
        rle_records_from_runs(np.array([1]), np.array([0]), 2, 2)
    with pytest.raises(ValueError):
        rle_records_from_runs(np.array([0, 2]), np.array([0]), 2, 2)


# the hand vectors of tests/test_eval_cpu.py (derived there from maskApi.c rleToString)
@pytest.mark.parametrize("counts,expect", [([4], "4"), ([0, 1], "01"), ([100], "T3"), ([10, 20, 5], ":d05"),
                                           ([10, 20, 5, 3], ":d05_O"), ([0, 40, 2, 40], "0X120")])
def test_rle_counts_to_string_hand_vectors(counts, expect):
    assert rle_counts_to_string(counts) == expect
    assert rle_counts_to_string(np.asarray(counts)) == expect


@pytest.mark.parametrize("shape,density", [((37, 53), 0.5), ((64, 64), 0.02), ((1, 97), 0.7), ((120, 5), 0.98),
                                           ((16, 16), 0.0), ((16, 16), 1.0)])
def test_coco_rle_encode_split_is_unchanged(shape, density):
    rng = np.random.default_rng(shape[1] * 11 + int(density * 100))
    m = (rng.random(shape) < density).astype(np.uint8)
    if 0 < density < 1:
        m[: shape[0] // 2, : shape[1] // 3] = 1
    got = coco_rle_encode(m)
    assert got == OE.rle_encode(m)
    assert got == {"size": list(shape), "counts": rle_counts_to_string(rle_mask_counts(m))}
    assert sum(rle_mask_counts(m)) == m.size


def test_encode_json_label_runs_equals_encode_json_sem_seg():
    ev = SemSegEvaluator(None, distributed=False, class_names=list("abcde"), ignore_label=255, device="cpu")
    pred = np.random.default_rng(0).integers(0, 5, (23, 31))
    pred[pred == 3] = 4
    runs = numpy_runs(pred)
    assert ev.encode_json_label_runs(*runs, 23, 31, "img.jpg") == ev.encode_json_sem_seg(pred, "img.jpg")
    assert ev.encode_json_label_runs(*runs, 23, 31, "img.jpg") == OE.sem_seg_records(pred, "img.jpg")
    ev._contiguous_id_to_dataset_id = {0: 10, 1: 11, 2: 12, 3: 13, 4: 20}
    mapped = ev.encode_json_label_runs(*runs, 23, 31, "img.jpg")
    assert mapped == ev.encode_json_sem_seg(pred, "img.jpg")
    assert [r["category_id"] for r in mapped] == [10, 11, 12, 20]
    ev._contiguous_id_to_dataset_id = {0: 10}
    with pytest.raises(AssertionError):
        ev.encode_json_label_runs(*runs, 23, 31, "img.jpg")


def test_evaluator_rle_argument():
    kw = dict(distributed=False, class_names=["a"], ignore_label=255, device="cpu")
    assert SemSegEvaluator(None, **kw)._rle == "device"
    assert SemSegEvaluator(None, rle="host", **kw)._rle == "host"
    with pytest.raises(ValueError):
        SemSegEvaluator(None, rle="pycocotools", **kw)


NEW = ("catseg_label_runs_workspace", "catseg_label_runs_count", "catseg_label_runs_write")


def test_header_and_lib_carry_the_label_runs_symbols():
    hdr = open(os.path.join(ROOT, "include", "catseg_hip.h")).read()
    declared = set(re.findall(r"\b(catseg_[a-z0-9_]+)\s*\(", hdr))
    lib = L.load()
    for s in NEW:
        assert s in declared and s in L.EXPORTED and hasattr(lib, s), s
    assert "plain_train_net.py:207-228" in hdr and "rleEncode" in hdr
    assert lib.catseg_abi_version() == 1


def test_label_runs_workspace_and_argument_checks_without_gpu():
    """The host-side checks refuse bad arguments before any launch (no device needed): the pointers are
    never dereferenced."""
    lib = L.load()
    assert lib.catseg_label_runs_workspace(0, 5) == 0
    assert lib.catseg_label_runs_workspace(1 << 16, 1 << 15) == 0           # H * W == 2^31
    # header + one offset per (column, 64-row chunk), padded to 4 ints + one block sum per 2048 of them
    assert lib.catseg_label_runs_workspace(70, 5000) == 4 * (4 + 10000 + 5)
    nb = lib.catseg_label_runs_workspace(8, 8)
    assert nb == 4 * (4 + 8 + 1)
    p = 4096                                                                # aligned, never dereferenced
    cases = [((p, 8, 8, 7, -1, p, nb, None), b"ld"), ((p, 1 << 16, 1 << 15, 1 << 15, -1, p, 1 << 40, None), b"2^31"),
             ((None, 8, 8, 8, -1, p, nb, None), b"null"), ((p, 8, 8, 8, -1, None, nb, None), b"null"),
             ((p, 0, 8, 8, -1, p, nb, None), b"positive"), ((p, 8, 8, 8, -1, p, nb - 4, None), b"workspace"),
             ((p, 8, 8, 8, -1, p + 4, nb, None), b"misaligned")]
    for args, word in cases:
        assert lib.catseg_label_runs_count(*args) == -1, args
        assert word in lib.catseg_last_error(), (args, lib.catseg_last_error())
        wargs = args[:7] + (p, p, 4, None)
        assert lib.catseg_label_runs_write(*wargs) == -1, wargs
        assert word in lib.catseg_last_error(), (wargs, lib.catseg_last_error())
    assert lib.catseg_label_runs_write(p, 8, 8, 8, -1, p, nb, None, p, 4, None) == -1
    assert lib.catseg_label_runs_write(p, 8, 8, 8, -1, p, nb, p, p, -1, None) == -1
    assert b"capacity" in lib.catseg_last_error()
