"""catseg_tiled_blend on the device: the merge of the tiles of one tiled scene with a window over every tile
("uniform" / "pyramid", cat_seg/tiling.py: window_weights) and, optionally, the global view (the scene's
logits at the tile's extent, resized to the canvas and averaged with the tiles' merge).

The arithmetic is pinned (a multiply and an add per covering tile, never an fma; one multiply by fp32
1 / sum(w); an add and a halving for the global view), so where catseg_postprocess runs banded the kernel
must EQUAL a composition of the existing kernels and torch elementwise ops, for all four (window, global)
combinations; at other widths it is checked against an fp64 reference.  Cases, the band rule and the helpers
are those of tests/test_gpu_tiled_merge.py."""
import functools

import pytest
import torch
import torch.nn.functional as F

import poison
from cat_seg import _lib as L
from cat_seg import ops, tiling
from test_gpu_tiled_merge import EXACT, FP64, _banded, _exact_case, _levels, _origins, _outputs

pytestmark = pytest.mark.gpu

KINDS = ("uniform", "pyramid")
COMBOS = [(k, gl) for k in KINDS for gl in (False, True)]
CASES = ["shifted-3x3", "T150-96", "npp16", "downsample", "rect-short"]


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def _wmap(g, kind, dtype=torch.float32):
    wy = torch.tensor(tiling.window_weights(g.th, kind), dtype=dtype)
    wx = torch.tensor(tiling.window_weights(g.tw, kind), dtype=dtype)
    return wy[:, None] * wx[None, :]


def _compose(tiles, gout, g, kind, glob):
    """Per tile `tmp = out * wmap`, `acc += tmp` in row-major tile order and `wsum += wmap` on the device; on
    the host m = acc * (fp32 1 / wsum); with the global view (m + gout) * 0.5.  tiles: the per-tile
    ops.postprocess outputs (T, th, tw); gout: ops.postprocess of the global logits to (H, W)."""
    T = tiles[0].shape[0]
    wmap = _wmap(g, kind).cuda()
    acc = torch.zeros(T, g.H, g.W, device="cuda")
    wsum = torch.zeros(g.H, g.W, device="cuda")
    for out, (oy, ox) in zip(tiles, _origins(g)):
        tmp = out * wmap
        acc[:, oy:oy + g.th, ox:ox + g.tw] += tmp
        wsum[oy:oy + g.th, ox:ox + g.tw] += wmap
    assert int(wsum.min()) >= 1 and float(wsum.max()) < 2 ** 24
    m = acc.cpu() * (torch.tensor(1.0, dtype=torch.float32) / wsum.cpu())
    return (m + gout.cpu()) * 0.5 if glob else m


def _post(lg, size, crop):
    out = torch.empty(1, lg.shape[0], size[0], size[1], device="cuda")
    ops.postprocess(lg[None].contiguous(), out, crop=crop)
    return out[0]


def _fused(lg, glg, g, crop, kind, glob, **which):
    p, lab, sc = _outputs(lg.shape[1], g, **which)
    ops.tiled_blend(lg.cuda().contiguous(), g, (0, g.ny), (0, g.H), weights=kind,
                    global_logits=glg.cuda().contiguous() if glob else None, crop=crop, probs=p, labels=lab, score=sc)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (p, lab, sc))


def _bound(tile, crop, out):
    """pt_patch_bound (post_tile.h): the source span of `tile` consecutive outputs of a crop -> out resize"""
    return min(crop, (tile - 1) * crop // out + 4)


@functools.lru_cache(maxsize=None)
def _case(name):
    """The inputs of EXACT[name] (the tiles' logits are those of tests/test_gpu_tiled_merge.py) plus global
    logits, and the two resizes every composition shares: computed once, not modified."""
    g, crop, lg, _, _, _ = _exact_case(name)
    T, h, w = lg.shape[1:]
    assert _banded(crop[0], crop[1], g.th, g.tw) and _banded(crop[0], crop[1], g.H, g.W)     # equality is owed
    glg = _levels((T, h, w), seed=7000 + T + g.H)
    dev = lg.cuda()
    tiles = [_post(dev[i], (g.th, g.tw), crop) for i in range(dev.shape[0])]
    gout = _post(glg.cuda(), (g.H, g.W), crop)
    return g, crop, lg, glg, tiles, gout


@functools.lru_cache(maxsize=None)
def _result(name, kind, glob):
    g, crop, lg, glg, tiles, gout = _case(name)
    return _compose(tiles, gout, g, kind, glob), _fused(lg, glg, g, crop, kind, glob)


# ---------------------------------------------------------------- (a) bit-exact against the composition
@pytest.mark.parametrize("kind,glob", COMBOS)
@pytest.mark.parametrize("name", CASES)
def test_equals_the_composition(name, kind, glob):
    ref, (p, lab, sc) = _result(name, kind, glob)
    assert torch.equal(p, ref)
    assert torch.equal(lab, ref.argmax(0).int()) and torch.equal(sc, ref.max(0).values)
    assert torch.equal(lab, p.argmax(0).int()) and torch.equal(sc, p.max(0).values)
    assert 0 < (lab > 0).float().mean() < 1


def test_patch_bounds_of_the_two_views():
    """The LDS stage follows from the larger of the tile's and the global view's patch bound.  The global
    view resizes the same crop to (H, W) >= (th, tw), so its bound never exceeds the tile's: the two are equal
    where the tile is the scene (npp16) and the tile's is larger elsewhere (downsample); a global patch larger
    than the tile's cannot be constructed, so that order of the max has no case."""
    for name in CASES:
        g, crop = _case(name)[:2]
        tile = _bound(16, crop[0], g.th) * _bound(64, crop[1], g.tw)
        glob = _bound(16, crop[0], g.H) * _bound(64, crop[1], g.W)
        assert glob <= tile, name
        if name == "npp16":
            assert (g.ny, g.nx) == (1, 1) and glob == tile and tile > 2048        # 16 passes over the patch
        if name == "downsample":
            assert tile > glob and (tile, glob) == (21 * 37, 13 * 37)


def test_pyramid_differs_from_uniform_only_where_tiles_overlap():
    """Not a restatement of the kernel: one covering tile -> w p / w, which is p up to two roundings."""
    ref_u, (pu, _, _) = _result("shifted-3x3", "uniform", False)
    _, (pp, _, _) = _result("shifted-3x3", "pyramid", False)
    g = _case("shifted-3x3")[0]
    cnt = torch.zeros(g.H, g.W)
    for oy, ox in _origins(g):
        cnt[oy:oy + g.th, ox:ox + g.tw] += 1
    one = cnt == 1
    assert one.any() and (~one).any()
    assert (pp[:, one] - pu[:, one]).abs().max().item() <= 2 ** -22
    assert not torch.equal(pp[:, ~one], pu[:, ~one])


# ---------------------------------------------------------------- (b) unchanged when off
@pytest.mark.parametrize("name", ["shifted-3x3", "T150-96", "npp16"])
def test_uniform_without_global_is_tiled_merge(name):
    _, (p, lab, sc) = _result(name, "uniform", False)
    p0, lab0, sc0 = _exact_case(name)[5]                           # ops.tiled_merge on the same logits
    poison.check_bit_identical(p, p0, "probs")
    poison.check_bit_identical(lab, lab0, "labels")
    poison.check_bit_identical(sc, sc0, "score")


# ---------------------------------------------------------------- (c) streaming over windows of tile rows
@pytest.mark.parametrize("name", ["shifted-3x3", "T150-96"])
def test_streaming_equals_one_shot(name):
    g, crop, lg, glg, _, _ = _case(name)
    _, (p1, lab1, sc1) = _result(name, "pyramid", True)
    lg, glg = lg.cuda(), glg.cuda()
    p, lab, sc = _outputs(lg.shape[1], g)
    steps = list(tiling.merge_schedule(g.H, g.th, g.sy))
    assert len(steps) > 1
    for row0, rows, y0, y1 in steps:
        window = lg[row0 * g.nx:(row0 + rows) * g.nx].clone()    # only the window's tile rows, in a fresh buffer
        ops.tiled_blend(window, g, (row0, rows), (y0, y1), weights="pyramid", global_logits=glg, crop=crop, probs=p,
                        labels=lab, score=sc)
        torch.cuda.synchronize()
        # rows at and beyond y1 still hold the sentinel
        assert bool((p[:, y1:] == -7).all()) and bool((lab[y1:] == -7).all()) and bool((sc[y1:] == -7).all())
    assert torch.equal(p.cpu(), p1) and torch.equal(lab.cpu(), lab1) and torch.equal(sc.cpu(), sc1)


# ---------------------------------------------------------------- (d) poisoned outputs
@pytest.mark.parametrize("shift", [0, 1])
def test_poisoned_outputs(shift):
    """Outputs as views of sentinel buffers (shift 1: not 16-byte aligned, the scalar store path): the slack
    behind them is untouched, the result is the dense run's; outputs not passed and rows outside [y0, y1) are
    not written."""
    name = "shifted-3x3"
    g, crop, lg, glg, _, _ = _case(name)
    _, (p1, lab1, sc1) = _result(name, "pyramid", True)
    lg, glg = lg.cuda(), glg.cuda()
    T, n = lg.shape[1], g.H * g.W
    kw = dict(weights="pyramid", global_logits=glg, crop=crop)

    def bufs():
        pb = poison.filled((shift + T * n + 64,), torch.float32, "cuda")
        lb = poison.filled((shift + n + 64,), torch.int32, "cuda")
        sb = poison.filled((shift + n + 64,), torch.float32, "cuda")
        return (pb, lb, sb), (pb[shift:shift + T * n].view(T, g.H, g.W), lb[shift:shift + n].view(g.H, g.W),
                              sb[shift:shift + n].view(g.H, g.W))

    (pb, lb, sb), (p, lab, sc) = bufs()
    ops.tiled_blend(lg, g, (0, g.ny), (0, g.H), probs=p, labels=lab, score=sc, **kw)
    torch.cuda.synchronize()
    for buf, m, what in ((pb, T * n, "probs"), (lb, n, "labels"), (sb, n, "score")):
        assert bool(poison.holds_fill(buf[:shift]).all()), what
        poison.check_untouched_flat(buf, shift + m, what)
    poison.check_no_nan(p, "probs")
    poison.check_bit_identical(p.cpu(), p1, "probs")
    poison.check_bit_identical(lab.cpu(), lab1, "labels")
    poison.check_bit_identical(sc.cpu(), sc1, "score")
    # outputs not passed are not written
    (pb, lb, sb), (p, lab, sc) = bufs()
    ops.tiled_blend(lg, g, (0, g.ny), (0, g.H), labels=lab, **kw)
    torch.cuda.synchronize()
    assert bool(poison.holds_fill(pb).all()) and bool(poison.holds_fill(sb).all())
    poison.check_bit_identical(lab.cpu(), lab1, "labels alone")
    (pb, lb, sb), (p, lab, sc) = bufs()
    ops.tiled_blend(lg, g, (0, g.ny), (0, g.H), probs=p, **kw)
    torch.cuda.synchronize()
    assert bool(poison.holds_fill(lb).all()) and bool(poison.holds_fill(sb).all())
    poison.check_bit_identical(p.cpu(), p1, "probs alone")
    # rows outside [y0, y1): a middle step of the schedule
    steps = list(tiling.merge_schedule(g.H, g.th, g.sy))
    row0, rows, y0, y1 = steps[1]
    assert 0 < y0 < y1 < g.H
    (pb, lb, sb), (p, lab, sc) = bufs()
    ops.tiled_blend(lg[row0 * g.nx:(row0 + rows) * g.nx].clone(), g, (row0, rows), (y0, y1), probs=p, labels=lab,
                    score=sc, **kw)
    torch.cuda.synchronize()
    for t, ref in ((p, p1), (lab, lab1), (sc, sc1)):
        assert bool(poison.holds_fill(t[..., :y0, :]).all()) and bool(poison.holds_fill(t[..., y1:, :]).all())
        poison.check_bit_identical(t[..., y0:y1, :].cpu(), ref[..., y0:y1, :], "rows of the step")
    for buf, m in ((pb, T * n), (lb, n), (sb, n)):
        poison.check_untouched_flat(buf, shift + m, "step")


# ---------------------------------------------------------------- (e) fp64 reference at widths that do not band
@pytest.mark.parametrize("name", list(FP64))
def test_against_fp64_reference(name):
    """fp64 on the host: per tile the sigmoid of the logits, F.interpolate(bilinear, align_corners=False) to
    the tile's extent, weighted by the window, accumulated and divided by the weight sum; the global view
    (the last slice of the logits) the same resize to (H, W), then (m + g) / 2.  The rule of
    tests/test_gpu_tiled_merge.py::test_against_fp64_reference, unchanged, for all four (window, global)
    combinations: a pixel is contested when its fp64 top-two gap is below 1e-5; uncontested pixels carry the
    fp64 argmax, contested ones a label within 1e-5 of the maximum; scores and probabilities are within 1e-5;
    at most 0.5 % of the pixels are contested.  The label form must also equal the argmax / max of the
    kernel's own probability form."""
    H, W, tile, stride, T, h, w = FP64[name]
    g = tiling.tile_grid(H, W, tile, stride)
    ch, cw = h, w
    n = g.ny * g.nx
    lg = 3 * torch.randn(n + 1, T, h, w, generator=torch.Generator().manual_seed(4000 + T + H))
    tiles, glg = lg[:n], lg[n]
    wmaps = {k: _wmap(g, k, torch.float64) for k in KINDS}
    num = {k: torch.zeros(T, H, W, dtype=torch.float64) for k in KINDS}
    den = {k: torch.zeros(H, W, dtype=torch.float64) for k in KINDS}
    for i, (oy, ox) in enumerate(_origins(g)):
        r = F.interpolate(tiles[i:i + 1].double()[..., :ch, :cw].sigmoid(), size=(g.th, g.tw), mode="bilinear",
                          align_corners=False)[0]
        for k in KINDS:
            num[k][:, oy:oy + g.th, ox:ox + g.tw] += r * wmaps[k]
            den[k][oy:oy + g.th, ox:ox + g.tw] += wmaps[k]
    gref = F.interpolate(glg[None].double()[..., :ch, :cw].sigmoid(), size=(H, W), mode="bilinear",
                         align_corners=False)[0]
    for kind, glob in COMBOS:
        ref = num[kind] / den[kind]
        if glob:
            ref = (ref + gref) / 2
        top2 = ref.topk(2, dim=0).values
        contested = (top2[0] - top2[1]) < 1e-5
        p, _, _ = _fused(tiles, glg, g, (ch, cw), kind, glob, labels=False, score=False)
        _, lab, sc = _fused(tiles, glg, g, (ch, cw), kind, glob, probs=False)
        assert torch.equal(lab, p.argmax(0).int()) and torch.equal(sc, p.max(0).values)
        lab, sc = lab.long(), sc.double()
        assert int(lab.min()) >= 0 and int(lab.max()) < T
        picked = ref.gather(0, lab[None])[0]
        share = contested.float().mean().item()
        print(f"{name} {kind} global={glob} T={T} {H}x{W}: contested {100 * share:.3f} %, max |probs - fp64| "
              f"{(p.double() - ref).abs().max().item():.2e}, max |score - fp64| "
              f"{(sc - top2[0]).abs().max().item():.2e}, max fp64 shortfall of the label "
              f"{(top2[0] - picked).max().item():.2e}")
        assert share <= 0.005
        assert torch.equal(lab[~contested], ref.argmax(0)[~contested])
        assert ((top2[0] - picked)[contested] <= 1e-5).all()
        assert (sc - top2[0]).abs().max().item() <= 1e-5
        assert (p.double() - ref).abs().max().item() <= 1e-5


# ---------------------------------------------------------------- (f) NaN
@pytest.mark.parametrize("where", ["tile", "global", "both"])
def test_nan_ranks_highest_first_nan_wins(where):
    """Two tiles of 24 x 24 at columns 0 and 12 of a 24 x 36 image (identity resize per tile) and a global
    view resized 24 -> 36 columns; pyramid + global.  A NaN in a tile's logit, in the global logits, or in
    both reaches the output (w * NaN, s + NaN, m + NaN are NaN) and the label is the first NaN class."""
    g = tiling.tile_grid(24, 36, 24, 12)
    assert (g.ny, g.nx, g.oxs) == (1, 2, (0, 12)) and _banded(24, 24, 24, 36)
    lg = _levels((2, 9, 24, 24), seed=7)
    glg = _levels((9, 24, 24), seed=8)
    if where in ("tile", "both"):
        lg[0, 3, 10, 12:17] = float("nan")     # image columns 12 .. 16: both tiles cover
        lg[0, 5, 1, :] = float("nan")
        lg[0, 2, 1, ::2] = float("nan")        # two NaNs at one pixel: the first (class 2) wins
        lg[1, 7, 3, 4] = float("inf")
    if where in ("global", "both"):
        glg[4, 10, 9] = float("nan")           # global column 9 -> image columns around 14
        glg[1, 20, :] = float("nan")           # a class below the tile's NaN classes: wins where both are NaN
        glg[6, 5, 6] = float("inf")
    dev = lg.cuda()
    tiles = [_post(dev[i], (g.th, g.tw), (24, 24)) for i in range(2)]
    gout = _post(glg.cuda(), (g.H, g.W), (24, 24))
    ref = _compose(tiles, gout, g, "pyramid", True)
    p, lab, sc = _fused(lg, glg, g, (24, 24), "pyramid", True)
    nan = ref.isnan()
    assert int(nan.sum()) >= (5 + 24 + 12 if where != "global" else 36)
    first = torch.where(nan.any(0), nan.int().argmax(0), ref.nan_to_num(nan=-1.0).argmax(0)).int()
    assert torch.equal(lab, first)             # the first NaN class where there is one
    assert torch.equal(lab, ref.argmax(0).int())
    if where != "global":
        assert int(lab[1, 0]) == 2 and int(lab[1, 23]) == 5 and int(lab[10, 14]) == 3
    if where != "tile":
        assert bool((lab[20] == 1).all())      # the global view's NaN row (rows are not resized: 24 -> 24)
    assert torch.equal(p.isnan(), nan) and torch.equal(sc.isnan(), ref.max(0).values.isnan())
    assert torch.allclose(p, ref, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(sc, ref.max(0).values, rtol=0, atol=0, equal_nan=True)


# ---------------------------------------------------------------- (g) errors
def test_errors():
    g, crop, lg, glg, _, _ = _case("shifted-3x3")
    lg, glg = lg.cuda(), glg.cuda()
    p = _outputs(lg.shape[1], g, labels=False, score=False)[0]
    row0, rows, y0, y1 = list(tiling.merge_schedule(g.H, g.th, g.sy))[-1]
    assert rows >= 2
    # a window that omits a covering tile row: catseg_tiled_merge's message
    with pytest.raises(RuntimeError, match="covered by tile rows"):
        ops.tiled_blend(lg[(row0 + 1) * g.nx:(row0 + rows) * g.nx].clone(), g, (row0 + 1, rows - 1), (y0, y1),
                        weights="pyramid", global_logits=glg, crop=crop, probs=p)
    with pytest.raises(ValueError):
        ops.tiled_blend(lg, g, (0, g.ny), (0, g.H), weights="pyramid")
    with pytest.raises(ValueError, match="window"):
        ops.tiled_blend(lg, g, (0, g.ny), (0, g.H), weights="hann", probs=p)
    # the LDS stage: 400 x 400 logits squeezed into 48 x 48 tiles.  The message names the views whose patch
    # does not fit; the global view's never exceeds a tile's (test_patch_bounds_of_the_two_views), so it is
    # named together with the tile and only when it is passed.
    big = torch.zeros(g.ny * g.nx, 1, 400, 400, device="cuda")
    p1 = _outputs(1, g, labels=False, score=False)[0]
    with pytest.raises(RuntimeError, match="LDS stage.*of a tile and of the global view"):
        ops.tiled_blend(big, g, (0, g.ny), (0, g.H), weights="pyramid", global_logits=big[0], probs=p1)
    with pytest.raises(RuntimeError, match="LDS stage.*of a tile:"):
        ops.tiled_blend(big, g, (0, g.ny), (0, g.H), weights="pyramid", probs=p1)
    assert bool((p == -7).all()) and bool((p1 == -7).all())
