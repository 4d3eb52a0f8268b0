"""ops.mode_filter (catseg_mode_filter) against the sequential restatement tests/mode_ref.py, bit for bit: shapes
smaller than the window, equal to the kernel's 64 x 16 tile, one pixel past a tile border and several tiles wide;
label changes on the tile borders and in the corners; a noise map with 200 distinct labels; both rules, the special
scores, the novote label with and without fill, iterations, strided views of poisoned buffers, the refusals."""
import numpy as np
import pytest
import torch

import mode_ref as M
import poison
from cat_seg import ops

from test_gpu_label_regions import strided_input
from test_gpu_render import SCORES
from test_mode_filter_cpu import blob_map

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (17, 23), (16, 64), (17, 65), (150, 203)]
SIZES = (3, 5, 15)
_CASES, _REF = {}, {}


def case(H, W):
    """One set of inputs per shape, made once: labels -1, 255 and 8191 among them."""
    if (H, W) not in _CASES:
        rng = np.random.default_rng(1000 * H + W)
        _CASES[(H, W)] = dict(labels=blob_map(rng, H, W), score=rng.choice(SCORES, (H, W)).astype(np.float32))
    return _CASES[(H, W)]


def noise_case():
    if "noise" not in _CASES:
        rng = np.random.default_rng(7)
        lab = (rng.integers(0, 200, (17, 65)) * 37 - 3000).astype(np.int32)          # 200 distinct labels, some negative
        _CASES["noise"] = dict(labels=lab, score=rng.random((17, 65)).astype(np.float32))
    return _CASES["noise"]


def ref(key, c, size, rule="plurality", scored=False, **kw):
    """The restatement of one pass, computed once per case and options (both rules from one count)."""
    k = (key, size, scored, tuple(sorted(kw.items())))
    if k not in _REF:
        _REF[k] = M.mode_filter_rules(c["labels"], size, score=c["score"] if scored else None, **kw)
    return _REF[k][rule]


def run(c, size, scored=False, **kw):
    dev = lambda a: torch.as_tensor(a).cuda()
    return ops.mode_filter(dev(c["labels"]), size, score=dev(c["score"]) if scored else None, **kw).cpu().numpy()


@pytest.mark.parametrize("H,W", SHAPES)
def test_shapes_sizes_and_rules(H, W):
    c = case(H, W)
    for size in SIZES:
        for rule in ("plurality", "half"):
            got = run(c, size, rule=rule)
            assert got.dtype == np.int32 and np.array_equal(got, ref((H, W), c, size, rule=rule)), (size, rule)


@pytest.mark.parametrize("H,W", SHAPES[:-1])
def test_scores_and_the_novote_label(H, W):
    c = case(H, W)
    for size in SIZES:
        assert np.array_equal(run(c, size, scored=True), ref((H, W), c, size, scored=True)), size
        for fill in (False, True):
            for scored in (False, True):
                kw = dict(novote_label=255, fill=fill, rule="half" if fill else "plurality")
                got = run(c, size, scored=scored, **kw)
                assert np.array_equal(got, ref((H, W), c, size, scored=scored, **kw)), (size, fill, scored)
                if not fill:
                    assert np.array_equal(got == 255, c["labels"] == 255)        # rejected pixels stay, none appear


def test_every_special_score_in_one_window():
    c = dict(labels=case(17, 23)["labels"], score=np.resize(SCORES, (17, 23)).astype(np.float32))
    for size in SIZES:
        assert np.array_equal(run(c, size, scored=True), M.mode_filter(c["labels"], size, score=c["score"])), size


def test_noise_map_with_200_labels():
    c = noise_case()
    assert len(np.unique(c["labels"])) > 190
    for size in SIZES:
        for scored in (False, True):
            assert np.array_equal(run(c, size, scored=scored), ref("noise", c, size, scored=scored)), (size, scored)
    kw = dict(novote_label=int(c["labels"][3, 3]), fill=True, rule="half")
    assert np.array_equal(run(c, 5, **kw), ref("noise", c, 5, **kw))


def test_extreme_label_values():
    c = dict(case(17, 65))
    c["labels"] = c["labels"].copy()
    c["labels"][2, :6] = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, -1]
    c["labels"][3, :6] = [2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0, -1]
    for kw in ({}, dict(novote_label=-2 ** 31), dict(novote_label=2 ** 31 - 1, fill=True)):
        assert np.array_equal(run(c, 3, **kw), M.mode_filter(c["labels"], 3, **kw)), kw


def test_iterations_equal_single_calls():
    c = case(17, 65)
    lab, score = torch.as_tensor(c["labels"]).cuda(), torch.as_tensor(c["score"]).cuda()
    for kw in (dict(), dict(score=score, rule="half"), dict(novote_label=255, fill=True)):
        for n in (2, 3):
            want = lab
            for _ in range(n):
                want = ops.mode_filter(want, 5, **kw)
            assert torch.equal(ops.mode_filter(lab, 5, iterations=n, **kw), want), (kw.keys(), n)
    assert np.array_equal(ops.mode_filter(lab, 3, iterations=3).cpu().numpy(), M.mode_filter(c["labels"], 3, iterations=3))
    out = torch.empty_like(lab)
    assert ops.mode_filter(lab, 3, iterations=2, out=out) is out               # the last pass lands in out
    assert np.array_equal(out.cpu().numpy(), M.mode_filter(c["labels"], 3, iterations=2))


def test_strided_views_of_poisoned_buffers_and_determinism():
    H, W = 37, 75
    rng = np.random.default_rng(11)
    c = dict(labels=blob_map(rng, H, W), score=rng.choice(SCORES, (H, W)).astype(np.float32))
    lbuf, lab = strided_input(c["labels"])
    sbuf, score = poison.padded(torch.as_tensor(c["score"]), 2, 5, device="cuda")
    for size, its in ((3, 1), (15, 1), (5, 2)):
        obuf, out = poison.out_buffer(H, W, 3, 7, torch.int32)
        dense = ops.mode_filter(lab.contiguous(), size, iterations=its, score=score.contiguous(), novote_label=255)
        got = ops.mode_filter(lab, size, iterations=its, score=score, novote_label=255, out=out)
        assert got is out
        poison.check_untouched(obuf, H, W, f"mode_filter size {size}")
        poison.check_bit_identical(out.contiguous(), dense, "strided vs dense")
        again = ops.mode_filter(lab, size, iterations=its, score=score, novote_label=255)
        poison.check_bit_identical(again, dense, "two runs")
        assert np.array_equal(dense.cpu().numpy(),
                              M.mode_filter(c["labels"], size, its, score=c["score"], novote_label=255))
    assert torch.equal(lbuf, strided_input(c["labels"])[0]), "the input buffer changed"
    # two views of one pitched buffer, side by side
    both = torch.full((H, 2 * W + 3), 5, dtype=torch.int32, device="cuda")
    both[:, :W] = lab
    ops.mode_filter(both[:, :W], 3, out=both[:, W + 3:])
    assert np.array_equal(both[:, W + 3:].cpu().numpy(), M.mode_filter(c["labels"], 3))
    assert bool((both[:, W:W + 3] == 5).all()) and torch.equal(both[:, :W], lab)


def test_argument_checks():
    lab = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    score = torch.zeros((8, 8), device="cuda")
    bad = [
        (dict(labels=lab.cpu()), "CUDA tensor"), (dict(labels=lab.long()), "int32"), (dict(labels=lab[0]), "2-D"),
        (dict(labels=lab.t()), "contiguous"),
        (dict(size=4), "size"), (dict(size=1), "size"), (dict(size=17), "size"), (dict(size=3.0), "size"),
        (dict(iterations=0), "iterations"), (dict(iterations=9), "iterations"), (dict(iterations=True), "iterations"),
        (dict(rule="majority"), "rule"),
        (dict(score=score.cpu()), "score"), (dict(score=score.double()), "score"), (dict(score=score[:4]), "score"),
        (dict(score=score.t()), "score"),
        (dict(novote_label=2 ** 31), "novote_label"), (dict(novote_label=1.0), "novote_label"),
        (dict(out=torch.zeros((8, 9), dtype=torch.int32, device="cuda")), "out"),
        (dict(out=torch.zeros((8, 8), device="cuda")), "out"), (dict(out=lab.cpu()), "out"),
    ]
    for kw, text in bad:
        a = dict(labels=lab, size=3)
        a.update(kw)
        with pytest.raises(ValueError, match=text):
            ops.mode_filter(a.pop("labels"), a.pop("size"), **a)
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.mode_filter(lab, 3, out=lab)
    big = torch.zeros((1, 16385), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="16384"):
        ops.mode_filter(big, 3)
