"""The tile grid of tiled inference (cat_seg/tiling.py) and its config rules, without a GPU: the per-axis
formula on fixed cases, cover and cover count over a sweep, the four properties of the streaming merge
schedule, the construction-time validation of MODEL.CATSEG_HIP.TILED, and the host-side argument checks of
the two C entry points (all run before any launch)."""
import ctypes as C

import pytest

from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg import tiling
from test_boundary_cpu import tiny_cfg

CASES = [  # (L, t, s) -> t', origins
    ((89, 48, 24), 48, [0, 24, 41]),
    ((301, 128, 96), 128, [0, 96, 173]),
    ((355, 128, 96), 128, [0, 96, 192, 227]),
    ((33, 64, 32), 33, [0]),
    ((131, 48, 24), 48, [0, 24, 48, 72, 83]),
]


@pytest.mark.parametrize("args,t1,origins", CASES)
def test_grid_1d_cases(args, t1, origins):
    assert tiling.grid_1d(*args) == (t1, origins)


def _formula(Lx, t, s):
    t1 = min(t, Lx)
    n = max(Lx - t1 + s - 1, 0) // s + 1
    return t1, [min(i * s, Lx - t1) for i in range(n)]


SWEEP = [(Lx, t, s) for t in (32, 48, 64) for s in (t // 2, 3 * t // 4, t) for Lx in range(1, 401)]


def test_grid_1d_covers_with_1_to_3_tiles():
    for Lx, t, s in SWEEP:
        t1, org = tiling.grid_1d(Lx, t, s)
        assert (t1, org) == _formula(Lx, t, s)
        assert org[0] == 0 and org[-1] + t1 == Lx and all(a < b for a, b in zip(org, org[1:]))
        count = [0] * Lx
        for o in org:
            for p in range(o, o + t1):
                count[p] += 1
        assert min(count) >= 1 and max(count) <= 3, (Lx, t, s)


def test_tile_grid_is_row_major_and_validates():
    g = tiling.tile_grid(33, 132, (64, 48), (32, 24))
    assert (g.th, g.tw, g.ny, g.nx) == (33, 48, 1, len(tiling.grid_1d(132, 48, 24)[1]))
    assert g.origins(0) == [(0, ox) for ox in tiling.grid_1d(132, 48, 24)[1]]
    g = tiling.tile_grid(90, 92, 48, 24)
    assert g.oys == (0, 24, 42) and g.oxs == (0, 24, 44) and tuple(g)[:6] == (90, 92, 48, 48, 24, 24)
    with pytest.raises(ValueError):
        tiling.tile_grid(100, 100, 64, 31)          # stride below TILE / 2
    with pytest.raises(ValueError):
        tiling.tile_grid(100, 100, 64, 65)          # stride above TILE


def test_merge_schedule_properties():
    for H, t, s in SWEEP:
        th, oys = tiling.grid_1d(H, t, s)
        steps = list(tiling.merge_schedule(H, t, s))
        # the [y0, y1) ranges partition [0, H) in order
        assert steps[0][2] == 0 and steps[-1][3] == H
        assert all(a[3] == b[2] for a, b in zip(steps, steps[1:])) and all(y0 < y1 for _, _, y0, y1 in steps)
        # row0 never decreases
        assert all(a[0] <= b[0] for a, b in zip(steps, steps[1:]))
        for row0, rows, y0, y1 in steps:
            assert 1 <= rows <= 3 and row0 >= 0 and row0 + rows <= len(oys)
            # each window holds every tile row that covers a row of [y0, y1)
            for r, oy in enumerate(oys):
                if oy < y1 and oy + th > y0:
                    assert row0 <= r < row0 + rows, (H, t, s, (row0, rows, y0, y1), r)


# ---------------------------------------------------------------- config
def _tiled(**over):
    return tiny_cfg(**{"MODEL.CATSEG_HIP.TILED.ENABLED": "True", **over})


def test_config_defaults_are_off():
    cfg = tiny_cfg()
    t = cfg.MODEL.CATSEG_HIP.TILED
    assert (t.ENABLED, t.TILE, t.STRIDE, t.BATCH) == (False, 384, 256, 8)
    assert build_model(cfg).tiled is False


def test_config_validation():
    m = build_model(_tiled(**{"MODEL.CATSEG_HIP.TILED.TILE": "64", "MODEL.CATSEG_HIP.TILED.STRIDE": "32"}))
    assert (m.tiled, m.tiled_tile, m.tiled_stride, m.tiled_batch) == (True, 64, 32, 8)
    with pytest.raises(ValueError, match="STRIDE"):
        build_model(_tiled(**{"MODEL.CATSEG_HIP.TILED.TILE": "64", "MODEL.CATSEG_HIP.TILED.STRIDE": "31"}))
    with pytest.raises(ValueError, match="STRIDE"):
        build_model(_tiled(**{"MODEL.CATSEG_HIP.TILED.TILE": "64", "MODEL.CATSEG_HIP.TILED.STRIDE": "96"}))
    with pytest.raises(ValueError, match="multiple"):
        build_model(_tiled(**{"MODEL.CATSEG_HIP.TILED.TILE": "48", "MODEL.CATSEG_HIP.TILED.STRIDE": "24"}))
    with pytest.raises(ValueError, match="SLIDING_WINDOW"):
        build_model(_tiled(**{"TEST.SLIDING_WINDOW": "True"}))
    with pytest.raises(ValueError, match="TTA_MERGE"):
        build_model(_tiled(**{"MODEL.CATSEG_HIP.TTA_MERGE": "device"}))
    with pytest.raises(ValueError, match="BATCH"):
        build_model(_tiled(**{"MODEL.CATSEG_HIP.TILED.BATCH": "33"}))


def test_forward_logits_refuses_tiled():
    m = build_model(_tiled()).eval()
    with pytest.raises(RuntimeError, match="TILED"):
        m.forward_logits([])


# ---------------------------------------------------------------- C entry points: checks before any launch
def test_abi_exports():
    lib = L.load()
    for name in ("catseg_tile_crops", "catseg_tiled_merge"):
        assert name in L.EXPORTED and hasattr(lib, name)
    assert lib.catseg_abi_version() == 1


def _merge(lib, *, T=3, h=8, w=8, crop=(8, 8), H=90, W=92, th=48, tw=48, sy=24, sx=24, row0=0, rows=3, y0=0, y1=90,
           probs=64, labels=64, score=0, logits=64):
    # the pointers are never dereferenced: every case fails a check on the host
    return lib.catseg_tiled_merge(logits, T, h, w, crop[0], crop[1], H, W, th, tw, sy, sx, row0, rows, y0, y1,
                                  probs, labels, score, None)


def test_tiled_merge_argument_checks():
    lib = L.load()
    bad = [dict(probs=0, labels=0), dict(labels=0, score=64), dict(logits=0), dict(T=0), dict(crop=(9, 8)),
           dict(th=91), dict(sy=23), dict(sx=49), dict(y0=5, y1=5), dict(y1=91), dict(row0=1, rows=3),
           dict(rows=0), dict(probs=66)]
    for kw in bad:
        assert _merge(lib, **kw) != 0, kw
        assert lib.catseg_last_error().startswith(b"tiled_merge:"), kw
    # tile rows of H = 90, t = 48, s = 24 start at 0, 24, 42: output row 41 is covered by rows 0 and 1, row 42 by all three
    assert _merge(lib, row0=0, rows=2, y0=0, y1=43) != 0
    err = lib.catseg_last_error()
    assert b"covered by tile rows 0 .. 2" in err and b"window holds 0 .. 1" in err
    assert _merge(lib, row0=1, rows=2, y0=24, y1=90) != 0
    assert b"covered by tile rows 0 .. 2" in lib.catseg_last_error()
    # a 16 x 64 output tile of a heavily downsampled tile does not fit the LDS stage
    assert _merge(lib, h=400, w=400, crop=(400, 400)) != 0
    err = lib.catseg_last_error()
    assert err.startswith(b"tiled_merge:") and b"LDS" in err


def test_tile_crops_argument_checks():
    lib = L.load()
    org = (C.c_int32 * 4)(0, 0, 42, 44)
    p = C.cast(org, C.c_void_p)

    def crops(image=64, H=90, W=92, origins=p, B=2, th=48, tw=48, canvas=64, ch=64, cw=64):
        return lib.catseg_tile_crops(image, H, W, origins, B, th, tw, canvas, ch, cw, None)

    for kw in (dict(image=0), dict(canvas=0), dict(origins=None), dict(B=0), dict(B=33), dict(th=91), dict(ch=47),
               dict(cw=47), dict(H=89)):
        assert crops(**kw) != 0, kw
        assert lib.catseg_last_error().startswith(b"tile_crops:"), kw
    assert crops(H=89) != 0
    assert b"origin (42, 44) of tile 1" in lib.catseg_last_error()
