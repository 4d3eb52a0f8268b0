"""catseg_tiled_merge / catseg_tile_crops on the device: the merge of the tiles of one tiled scene (per tile
the sigmoid + bilinear resize to the tile's extent, fp32 sum over the covering tiles in row-major tile
order, scale by the fp32 reciprocal of the per-pixel cover count) as probabilities and as the label map of
their argmax, in one shot and streamed over windows of tile rows; and the tile gather.

Where catseg_postprocess runs banded for a tile (tw % 4 == 0 and the band rule `_banded` restates) the
kernel forms every tile's value with the same taps and fmas, so its output must EQUAL the composition of the
existing kernels; at other widths it is checked against an fp64 reference."""
import functools

import pytest
import torch
import torch.nn.functional as F

from cat_seg import _lib as L
from cat_seg import ops, tiling

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _lib():
    L.require_gpu()


def _banded(ch, cw, H, W):
    """launch_post's rule (misc.hip): 48 output rows per band, the band's source rows in <= 64 KB of LDS."""
    rows = 48 * ch // H + 3
    return W % 4 == 0 and rows * cw * 4 <= 64 * 1024


def _levels(shape, seed):
    # a few levels: exact ties between classes are common, so the first-maximum rule is exercised
    return torch.randint(-2, 2, shape, generator=torch.Generator().manual_seed(seed)).float()


def _origins(g):
    return [(oy, ox) for oy in g.oys for ox in g.oxs]


def _composition(lg, g, crop):
    """What the existing kernel offers: per tile ops.postprocess to (th, tw), sequential fp32 adds in
    row-major tile order, then a MULTIPLY by fp32 1 / count."""
    lg = lg.cuda()
    T = lg.shape[1]
    acc = torch.zeros(T, g.H, g.W, device="cuda")
    cnt = torch.zeros(g.H, g.W, device="cuda")
    for i, (oy, ox) in enumerate(_origins(g)):
        out = torch.empty(1, T, g.th, g.tw, device="cuda")
        ops.postprocess(lg[i:i + 1].contiguous(), out, crop=crop)
        acc[:, oy:oy + g.th, ox:ox + g.tw] += out[0]
        cnt[oy:oy + g.th, ox:ox + g.tw] += 1
    assert int(cnt.min()) >= 1 and int(cnt.max()) <= 9
    rk = torch.tensor(1.0, dtype=torch.float32) / cnt.cpu()      # fp32 1 / count, formed on the host
    return acc.cpu() * rk, cnt.cpu()


def _outputs(T, g, *, probs=True, labels=True, score=True):
    p = torch.full((T, g.H, g.W), -7.0, device="cuda") if probs else None
    lab = torch.full((g.H, g.W), -7, dtype=torch.int32, device="cuda") if labels else None
    sc = torch.full((g.H, g.W), -7.0, device="cuda") if score else None
    return p, lab, sc


def _fused(lg, g, crop, **which):
    p, lab, sc = _outputs(lg.shape[1], g, **which)
    ops.tiled_merge(lg.cuda().contiguous(), g, (0, g.ny), (0, g.H), crop=crop, probs=p, labels=lab, score=sc)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu() for t in (p, lab, sc))


# ---------------------------------------------------------------- bit-exact against the existing kernels
EXACT = {  # id: H, W, tile, stride, T, h, w, crop
    "one-tile": (48, 68, 68, 34, 7, 24, 24, (20, 23)),
    "grid-2x3": (48, 64, 32, 16, 7, 8, 8, None),
    "shifted-3x3": (90, 92, 48, 24, 18, 12, 12, None),
    "T150-96": (300, 356, 128, 96, 150, 96, 96, None),
    "npp16": (20, 72, (20, 72), (10, 36), 3, 60, 72, None),
    "downsample": (50, 60, (28, 36), (14, 18), 19, 40, 40, (33, 37)),
    "rect-short": (33, 132, (64, 48), (32, 24), 5, 16, 12, None),
}


@functools.lru_cache(maxsize=None)
def _exact_case(name):
    """Inputs, the composition and the one-shot fused outputs of an EXACT case, computed once and shared."""
    H, W, tile, stride, T, h, w, crop = EXACT[name]
    g = tiling.tile_grid(H, W, tile, stride)
    crop = crop or (h, w)
    assert _banded(crop[0], crop[1], g.th, g.tw)                 # exact equality is owed
    lg = _levels((g.ny * g.nx, T, h, w), seed=T + H + W)
    ref, cnt = _composition(lg, g, crop)
    return g, crop, lg, ref, cnt, _fused(lg, g, crop)


@pytest.mark.parametrize("name", list(EXACT))
def test_equals_the_composition_of_existing_kernels(name):
    g, crop, lg, ref, cnt, (p, lab, sc) = _exact_case(name)
    assert torch.equal(p, ref)
    assert torch.equal(lab, ref.argmax(0).int())
    assert torch.equal(sc, ref.max(0).values)
    assert torch.equal(lab, p.argmax(0).int()) and torch.equal(sc, p.max(0).values)
    assert 0 < (lab > 0).float().mean() < 1
    if name == "one-tile":
        assert (g.ny, g.nx, g.th, g.tw) == (1, 1, 48, 68)
        # one tile is the existing single-view kernels, exactly
        out = torch.empty(1, lg.shape[1], g.H, g.W, device="cuda")
        ops.postprocess(lg.cuda(), out, crop=crop)
        assert torch.equal(p, out[0].cpu())
        l1 = torch.empty(1, g.H, g.W, dtype=torch.int32, device="cuda")
        s1 = torch.empty(1, g.H, g.W, device="cuda")
        ops.postprocess_argmax(lg.cuda(), l1, s1, crop=crop)
        assert torch.equal(lab, l1[0].cpu()) and torch.equal(sc, s1[0].cpu())
    if name == "shifted-3x3":
        assert int(cnt.max()) == 9                              # the shifted last tile over two regular ones
    if name == "grid-2x3":
        assert (g.ny, g.nx) == (2, 3) and int(cnt.max()) == 4


# ---------------------------------------------------------------- streaming over windows of tile rows
@pytest.mark.parametrize("name", ["shifted-3x3", "T150-96"])
def test_streaming_equals_one_shot(name):
    g, crop, lg, _, _, (p1, lab1, sc1) = _exact_case(name)
    lg = lg.cuda()
    T = lg.shape[1]
    p, lab, sc = _outputs(T, g)
    steps = list(tiling.merge_schedule(g.H, g.th, g.sy))
    assert len(steps) > 1
    for row0, rows, y0, y1 in steps:
        window = lg[row0 * g.nx:(row0 + rows) * g.nx].clone()    # only the window's tile rows, in a fresh buffer
        ops.tiled_merge(window, g, (row0, rows), (y0, y1), crop=crop, probs=p, labels=lab, score=sc)
        torch.cuda.synchronize()
        # rows outside [0, y1) still hold the sentinel
        assert bool((p[:, y1:] == -7).all()) and bool((lab[y1:] == -7).all()) and bool((sc[y1:] == -7).all())
    assert torch.equal(p.cpu(), p1) and torch.equal(lab.cpu(), lab1) and torch.equal(sc.cpu(), sc1)


def test_rows_before_the_range_are_not_touched_and_a_short_window_is_an_error():
    g, crop, lg, _, _, (p1, lab1, sc1) = _exact_case("shifted-3x3")
    lg = lg.cuda()
    p, lab, sc = _outputs(lg.shape[1], g)
    row0, rows, y0, y1 = list(tiling.merge_schedule(g.H, g.th, g.sy))[-1]
    assert y0 > 0
    ops.tiled_merge(lg[row0 * g.nx:(row0 + rows) * g.nx].clone(), g, (row0, rows), (y0, y1), crop=crop, probs=p,
                    labels=lab, score=sc)
    torch.cuda.synchronize()
    assert bool((p[:, :y0] == -7).all()) and bool((lab[:y0] == -7).all()) and bool((sc[:y0] == -7).all())
    assert torch.equal(p[:, y0:].cpu(), p1[:, y0:]) and torch.equal(lab[y0:].cpu(), lab1[y0:])
    # a window that omits a covering tile row
    assert rows >= 2
    with pytest.raises(RuntimeError, match="covered by tile rows"):
        ops.tiled_merge(lg[(row0 + 1) * g.nx:(row0 + rows) * g.nx].clone(), g, (row0 + 1, rows - 1), (y0, y1),
                        crop=crop, probs=p)


# ---------------------------------------------------------------- fp64 reference at widths that do not band
FP64 = {  # id: H, W, tile, stride, T, h, w
    "odd-3x3": (89, 91, 48, 24, 18, 12, 12),
    "T150-96": (301, 355, 128, 96, 150, 96, 96),
    "T847": (61, 45, 32, 16, 847, 24, 24),
    "downsample": (50, 39, (28, 64), (14, 32), 19, 40, 40),
    "rect-short": (33, 131, (64, 48), (32, 24), 5, 16, 12),
}


@pytest.mark.parametrize("name", list(FP64))
def test_against_fp64_reference(name):
    """fp64 on the host: per tile the sigmoid of the logits, F.interpolate(bilinear, align_corners=False) to
    the tile's extent, accumulated and divided by the cover count.  The rule of
    test_gpu_postprocess_argmax.py::test_against_fp64_reference, unchanged: a pixel is contested when its
    fp64 top-two gap is below 1e-5; uncontested pixels carry the fp64 argmax, contested ones a label within
    1e-5 of the maximum; scores and probabilities are within 1e-5; at most 0.5 % of the pixels are contested.
    The label form must also equal the argmax / max of the kernel's own probability form."""
    H, W, tile, stride, T, h, w = FP64[name]
    g = tiling.tile_grid(H, W, tile, stride)
    ch, cw = h, w
    lg = 3 * torch.randn(g.ny * g.nx, T, h, w, generator=torch.Generator().manual_seed(3000 + T + H))
    ref = torch.zeros(T, H, W, dtype=torch.float64)
    cnt = torch.zeros(H, W, dtype=torch.float64)
    for i, (oy, ox) in enumerate(_origins(g)):
        r = F.interpolate(lg[i:i + 1].double()[..., :ch, :cw].sigmoid(), size=(g.th, g.tw), mode="bilinear",
                          align_corners=False)[0]
        ref[:, oy:oy + g.th, ox:ox + g.tw] += r
        cnt[oy:oy + g.th, ox:ox + g.tw] += 1
    ref = ref / cnt
    top2 = ref.topk(2, dim=0).values
    contested = (top2[0] - top2[1]) < 1e-5
    p, _, _ = _fused(lg, g, (ch, cw), labels=False, score=False)
    _, lab, sc = _fused(lg, g, (ch, cw), probs=False)
    assert torch.equal(lab, p.argmax(0).int()) and torch.equal(sc, p.max(0).values)
    lab, sc = lab.long(), sc.double()
    assert int(lab.min()) >= 0 and int(lab.max()) < T
    picked = ref.gather(0, lab[None])[0]
    share = contested.float().mean().item()
    print(f"{name} T={T} {H}x{W}: contested {100 * share:.3f} %, max |probs - fp64| "
          f"{(p.double() - ref).abs().max().item():.2e}, max |score - fp64| {(sc - top2[0]).abs().max().item():.2e}, "
          f"max fp64 shortfall of the label {(top2[0] - picked).max().item():.2e}")
    assert share <= 0.005
    assert torch.equal(lab[~contested], ref.argmax(0)[~contested])
    assert ((top2[0] - picked)[contested] <= 1e-5).all()
    assert (sc - top2[0]).abs().max().item() <= 1e-5
    assert (p.double() - ref).abs().max().item() <= 1e-5


# ---------------------------------------------------------------- NaN / inf
def test_nan_ranks_highest_first_nan_wins():
    """Identity resize, two tiles of 24 x 24 at columns 0 and 12 of a 24 x 36 image: NaN planted in tile 0
    inside the overlap, +inf in tile 1 (sigmoid(NaN) = NaN, sigmoid(+inf) = 1; NaN + x = NaN)."""
    g = tiling.tile_grid(24, 36, 24, 12)
    assert (g.ny, g.nx, g.oxs) == (1, 2, (0, 12))
    lg = _levels((2, 9, 24, 24), seed=7)
    lg[0, 3, 10, 12:17] = float("nan")     # NaN at a class index > 0, image columns 12 .. 16 (both tiles cover)
    lg[0, 5, 1, :] = float("nan")
    lg[0, 2, 1, ::2] = float("nan")        # two NaNs at one pixel: the first (class 2) wins
    lg[1, 7, 3, 4] = float("inf")
    lg[1, 6, 5, 6] = float("inf")
    lg[1, 1, 10, 2] = float("inf")         # +inf in the other tile at image (10, 14), a pixel with a NaN
    ref, _ = _composition(lg, g, (24, 24))
    p, lab, sc = _fused(lg, g, (24, 24))
    # (a NaN also reaches the pixels whose second tap it is, as 0 * NaN, in both kernels)
    assert int(ref.argmax(0)[1, 0]) == 2 and int(ref.argmax(0)[1, 23]) == 5 and int(ref.argmax(0)[10, 14]) == 3
    assert torch.equal(lab, ref.argmax(0).int())
    assert torch.equal(p.isnan(), ref.isnan()) and int(p.isnan().sum()) >= 5 + 24 + 12
    assert torch.equal(sc.isnan(), ref.max(0).values.isnan())
    assert torch.allclose(p, ref, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(sc, ref.max(0).values, rtol=0, atol=0, equal_nan=True)


# ---------------------------------------------------------------- outputs not passed are not written
def test_outputs_not_passed_are_not_written():
    g = tiling.tile_grid(40, 56, 32, 16)
    lg = _levels((g.ny * g.nx, 5, 12, 12), seed=3).cuda()
    vol, labels, score = _outputs(5, g)
    ops.tiled_merge(lg, g, (0, g.ny), (0, g.H), labels=labels)
    torch.cuda.synchronize()
    assert int(labels.min()) >= 0
    assert bool((vol == -7).all()) and bool((score == -7).all())
    ops.tiled_merge(lg, g, (0, g.ny), (0, g.H), probs=vol)
    torch.cuda.synchronize()
    assert bool((vol >= 0).all()) and bool((score == -7).all())
    with pytest.raises(ValueError):
        ops.tiled_merge(lg, g, (0, g.ny), (0, g.H))
    with pytest.raises(RuntimeError, match="no output"):
        L.call("catseg_tiled_merge", lg.data_ptr(), 5, 12, 12, 12, 12, g.H, g.W, g.th, g.tw, g.sy, g.sx, 0, g.ny, 0,
               g.H, 0, 0, 0, None)


# ---------------------------------------------------------------- the tile gather
@pytest.mark.parametrize("H,W,tile,stride", [(90, 92, 48, 24), (33, 132, (64, 48), (32, 24))])
def test_tile_crops(H, W, tile, stride):
    g = tiling.tile_grid(H, W, tile, stride)
    image = torch.randn(3, H, W, generator=torch.Generator().manual_seed(H)).cuda()
    ch, cw = -(-g.th // 32) * 32, -(-g.tw // 32) * 32
    assert cw > g.tw and ch > g.th
    org = _origins(g)
    for i in range(0, len(org), 5):
        grp = org[i:i + 5]
        n = len(grp) * 3 * ch * cw
        buf = torch.full((n + 64,), float("nan"), device="cuda")        # poisoned: the canvas and a tail behind it
        canvas = buf[:n].view(len(grp), 3, ch, cw)
        ops.tile_crops(image, grp, g.th, g.tw, canvas)
        torch.cuda.synchronize()
        want = torch.zeros(len(grp), 3, ch, cw, device="cuda")
        for b, (oy, ox) in enumerate(grp):
            want[b, :, :g.th, :g.tw] = image[:, oy:oy + g.th, ox:ox + g.tw]
        assert torch.equal(canvas, want)
        assert bool(buf[n:].isnan().all())
