"""ops.mode_overview (catseg_mode_overview) against the sequential restatement tests/mode_ref.py, bit for bit: the
shapes of the filter's tests with factors that leave partial cells and exceed H or W, weights, the novote label, a
cell with no votes, strided views of poisoned buffers, the refusals."""
import numpy as np
import pytest
import torch

import mode_ref as M
import poison
from cat_seg import ops

from test_gpu_label_regions import strided_input
from test_gpu_mode_filter import SHAPES, case, noise_case

pytestmark = pytest.mark.gpu

FACTORS = (2, 3, 7, 16, 32)


def check(got, want, what):
    assert set(got) == {"labels", "votes", "total", "share"}
    for k in ("labels", "votes", "total"):
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), want[k]), (what, k)
    assert got["share"].dtype == torch.float32
    poison.check_bit_identical(got["share"].cpu(), torch.as_tensor(want["share"]), f"{what}: share")
    v, t = got["votes"].cpu().numpy().astype(np.float64), got["total"].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(got["share"].cpu().numpy(), (v / t).astype(np.float32), equal_nan=True), what


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_and_factors(H, W):
    c = case(H, W)
    lab, score = torch.as_tensor(c["labels"]).cuda(), torch.as_tensor(c["score"]).cuda()
    for f in FACTORS:
        got = ops.mode_overview(lab, f)
        assert got["labels"].shape == (-(-H // f), -(-W // f))
        check(got, M.mode_overview(c["labels"], f), (f, "count"))
        check(ops.mode_overview(lab, f, score=score), M.mode_overview(c["labels"], f, c["score"]), (f, "score"))
        check(ops.mode_overview(lab, f, score=score, novote_label=255),
              M.mode_overview(c["labels"], f, c["score"], 255), (f, "score, novote"))
        check(ops.mode_overview(lab, f, novote_label=0), M.mode_overview(c["labels"], f, None, 0), (f, "novote"))


def test_cells_without_votes():
    lab = np.full((9, 14), 7, np.int32)
    lab[0, 0], lab[8, 13], lab[4, 4:8] = 3, -5, 9
    score = np.zeros((9, 14), np.float32)
    score[4, 5] = np.nan
    t = torch.as_tensor(lab).cuda()
    for f in (2, 3, 4, 5, 32):
        got = ops.mode_overview(t, f, novote_label=7)
        check(got, M.mode_overview(lab, f, None, 7), (f, "novote 7"))
        if f < 5:
            assert bool((got["total"] == 0).any()) and bool(got["share"].isnan().any())
            assert bool((got["labels"][got["total"] == 0] == 7).all())
        # no vote anywhere and no novote label: the cell's smallest label, 0 of 0 votes
        got = ops.mode_overview(t, f, score=torch.as_tensor(score).cuda())
        check(got, M.mode_overview(lab, f, score), (f, "zero scores"))
        assert int(got["total"].abs().sum()) == 0 and bool(got["share"].isnan().all())


def test_noise_map_with_200_labels():
    c = noise_case()
    lab, score = torch.as_tensor(c["labels"]).cuda(), torch.as_tensor(c["score"]).cuda()
    for f in FACTORS:
        check(ops.mode_overview(lab, f), M.mode_overview(c["labels"], f), (f, "count"))
        check(ops.mode_overview(lab, f, score=score), M.mode_overview(c["labels"], f, c["score"]), (f, "score"))
    ext = c["labels"].copy()
    ext[:4, :8] = np.resize(np.array([2 ** 31 - 1, -2 ** 31, 0], np.int32), (4, 8))
    for f in (2, 3, 32):
        check(ops.mode_overview(torch.as_tensor(ext).cuda(), f), M.mode_overview(ext, f), (f, "extreme labels"))


def test_strided_views_of_poisoned_buffers_and_determinism():
    H, W = 37, 75
    c = case(150, 203)
    lab_np, score_np = c["labels"][:H, :W], c["score"][:H, :W]
    lbuf, lab = strided_input(lab_np)
    sbuf, score = poison.padded(torch.as_tensor(np.ascontiguousarray(score_np)), 2, 5, device="cuda")
    for f in (2, 7, 32):
        got = ops.mode_overview(lab, f, score=score, novote_label=255)
        check(got, M.mode_overview(lab_np, f, score_np, 255), (f, "strided"))
        again = ops.mode_overview(lab.contiguous(), f, score=score.contiguous(), novote_label=255)
        for k in got:
            poison.check_bit_identical(got[k], again[k], f"two runs: {k}")
    assert torch.equal(lbuf, strided_input(lab_np)[0]), "the input buffer changed"


def test_argument_checks():
    lab = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    score = torch.zeros((8, 8), device="cuda")
    bad = [
        (dict(labels=lab.cpu()), "CUDA tensor"), (dict(labels=lab.long()), "int32"), (dict(labels=lab.t()), "contiguous"),
        (dict(factor=1), "factor"), (dict(factor=33), "factor"), (dict(factor=2.0), "factor"), (dict(factor=True), "factor"),
        (dict(score=score.half()), "score"), (dict(score=score[:, :4]), "score"), (dict(score=score.cpu()), "score"),
        (dict(novote_label=-2 ** 31 - 1), "novote_label"), (dict(novote_label="7"), "novote_label"),
    ]
    for kw, text in bad:
        a = dict(labels=lab, factor=2)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.mode_overview(a.pop("labels"), a.pop("factor"), **a)
    with pytest.raises(ValueError, match="16384"):
        ops.mode_overview(torch.zeros((16385, 1), dtype=torch.int32, device="cuda"), 2)
