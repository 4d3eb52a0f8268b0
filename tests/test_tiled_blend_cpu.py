"""The window weights of the tiled merge (cat_seg/tiling.py: window_weights / weight_sum), the property they
exist for (a linear ramp across a tile overlap, where the uniform merge steps), the exactness bound of their
sums, the host-side argument checks of catseg_tiled_blend (all run before any launch) and the two config keys
MODEL.CATSEG_HIP.TILED.WINDOW / GLOBAL, without a GPU."""
import pytest

from cat_seg import _lib as L
from cat_seg import build_model
from cat_seg import tiling
from test_boundary_cpu import tiny_cfg


# ---------------------------------------------------------------- the weights
def test_window_weights():
    assert tiling.window_weights(5, "pyramid") == [1, 2, 3, 2, 1]
    assert tiling.window_weights(6, "pyramid") == [1, 2, 3, 3, 2, 1]
    for t in (1, 2, 7, 48, 2048):
        w = tiling.window_weights(t, "pyramid")
        assert len(w) == t and min(w) >= 1 and all(isinstance(v, int) for v in w) and w == w[::-1]
        assert tiling.window_weights(t, "uniform") == [1] * t
    with pytest.raises(ValueError, match="window"):
        tiling.window_weights(5, "hann")
    with pytest.raises(ValueError, match="window"):
        tiling.weight_sum([0], 5, 5, "hann")


def _blend_1d(values, origins, t, Lx, kind):
    """fp64 blend of per-tile constant values along one axis: sum(w_i p_i) / sum(w_i)."""
    w = tiling.window_weights(t, kind)
    den = tiling.weight_sum(origins, t, Lx, kind)
    num = [0.0] * Lx
    for p, o in zip(values, origins):
        for l in range(t):
            num[o + l] += w[l] * p
    return [a / b for a, b in zip(num, den)]


def test_pyramid_ramps_where_uniform_steps():
    """A regular axis ((L - t) % s == 0, overlap v = t - s <= t / 2): at overlap position b = 1 .. v (counted
    from the pixel before the overlap) tile A weighs v + 1 - b and tile B weighs b, so the two sum to v + 1 and
    per-tile constants p_A, p_B blend to the linear ramp p_A + (p_B - p_A) b / (v + 1).  Its largest step
    between neighbouring pixels is |p_B - p_A| / (v + 1); the uniform merge of the same data jumps by
    |p_B - p_A| / 2 where a tile's cover begins or ends.  Expected values are derived, not measured."""
    Lx, t, s = 80, 32, 24
    tq, org = tiling.grid_1d(Lx, t, s)
    assert tq == t and (Lx - t) % s == 0 and org == [0, 24, 48]
    v = t - s
    assert v == 8 and 2 * v <= t
    den = tiling.weight_sum(org, t, Lx, "pyramid")
    for a in org[1:]:                                              # every overlap [a, a + v)
        assert den[a:a + v] == [v + 1] * v
    vals = [0.25, 0.75, 0.5]
    pyr = _blend_1d(vals, org, t, Lx, "pyramid")
    uni = _blend_1d(vals, org, t, Lx, "uniform")
    for i, a in enumerate(org[1:]):
        pa, pb = vals[i], vals[i + 1]
        for b in range(1, v + 1):
            assert pyr[a + b - 1] == pytest.approx(pa + (pb - pa) * b / (v + 1), abs=1e-15)
        assert pyr[a - 1] == pa and pyr[a + v] == pb               # outside the overlap: the tile's own value
        assert uni[a:a + v] == [(pa + pb) / 2] * v
    delta = max(abs(vals[i + 1] - vals[i]) for i in range(len(vals) - 1))
    step = lambda m: max(abs(m[i + 1] - m[i]) for i in range(Lx - 1))
    assert step(pyr) == pytest.approx(delta / (v + 1), abs=1e-15)
    assert step(uni) == pytest.approx(delta / 2, abs=1e-15)


@pytest.mark.parametrize("Lx,t,s", [(90, 48, 24), (80, 32, 24), (2048 * 3 - 5, 2048, 1024), (5000, 2048, 1024)])
def test_weight_sum_stays_exact_in_fp32(Lx, t, s):
    """Per axis at most 3 tiles cover a position and w <= (t + 1) / 2, so the sum is at most 1.5 t (the
    shifted last tile over two regular ones included); a pixel's sum(w) is the product of two such sums:
    at most 2.25 t^2 < 2^24 at t = 2048."""
    tq, org = tiling.grid_1d(Lx, t, s)
    den = tiling.weight_sum(org, tq, Lx, "pyramid")
    cnt = tiling.weight_sum(org, tq, Lx, "uniform")
    assert min(den) >= 1 and 1 <= min(cnt) and max(cnt) <= 3
    if (Lx, t, s) == (90, 48, 24):
        assert org == [0, 24, 42] and max(cnt) == 3                # the shifted last tile
    assert max(den) <= 1.5 * tq
    assert max(den) ** 2 <= 2.25 * tq * tq
    if t == 2048:
        assert max(den) ** 2 < 2 ** 24


# ---------------------------------------------------------------- C entry point: checks before any launch
def test_abi_export():
    lib = L.load()
    assert "catseg_tiled_blend" in L.EXPORTED and hasattr(lib, "catseg_tiled_blend")


def _blend(lib, *, T=3, h=8, w=8, crop=(8, 8), H=90, W=92, th=48, tw=48, sy=24, sx=24, row0=0, rows=3, y0=0, y1=90,
           window=1, glob=64, probs=64, labels=64, score=0, logits=64):
    # the pointers are never dereferenced: every case fails a check on the host
    return lib.catseg_tiled_blend(logits, T, h, w, crop[0], crop[1], H, W, th, tw, sy, sx, row0, rows, y0, y1,
                                  window, glob, probs, labels, score, None)


def test_tiled_blend_argument_checks():
    lib = L.load()
    bad = [dict(window=2), dict(window=-1), dict(glob=66), dict(probs=0, labels=0), dict(labels=0, score=64),
           dict(logits=0), dict(T=0), dict(crop=(9, 8)), dict(th=91), dict(sy=23), dict(y1=91),
           dict(row0=1, rows=3), dict(probs=66),
           # "pyramid" above an extent of 2048, per axis
           dict(H=4000, th=2049, sy=1100, rows=2, y1=4000), dict(W=4000, tw=2049, sx=1100)]
    for kw in bad:
        assert _blend(lib, **kw) != 0, kw
        assert lib.catseg_last_error().startswith(b"tiled_blend:"), kw
    assert _blend(lib, window=2) != 0 and b"window" in lib.catseg_last_error()
    assert _blend(lib, W=4000, tw=2049, sx=1100) != 0 and b"2048" in lib.catseg_last_error()
    assert _blend(lib, glob=66) != 0 and b"misaligned" in lib.catseg_last_error()
    assert _blend(lib, probs=0, labels=0) != 0 and b"no output" in lib.catseg_last_error()
    # the same window rule and message as catseg_tiled_merge
    assert _blend(lib, row0=0, rows=2, y0=0, y1=43) != 0
    err = lib.catseg_last_error()
    assert b"covered by tile rows 0 .. 2" in err and b"window holds 0 .. 1" in err
    # the LDS stage: the message names the views whose patch does not fit
    assert _blend(lib, h=400, w=400, crop=(400, 400), glob=0) != 0
    err = lib.catseg_last_error()
    assert err.startswith(b"tiled_blend:") and b"LDS" in err and b"of a tile" in err and b"global view" not in err
    assert _blend(lib, h=400, w=400, crop=(400, 400)) != 0
    err = lib.catseg_last_error()
    assert b"LDS" in err and b"global view" in err


# ---------------------------------------------------------------- config
def test_config_defaults():
    cfg = tiny_cfg()
    t = cfg.MODEL.CATSEG_HIP.TILED
    assert (t.WINDOW, t.GLOBAL) == ("uniform", False)
    m = build_model(cfg)
    assert (m.tiled_window, m.tiled_global) == ("uniform", False)


def test_config_validation():
    on = {"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": "64",
          "MODEL.CATSEG_HIP.TILED.STRIDE": "32"}
    m = build_model(tiny_cfg(**on, **{"MODEL.CATSEG_HIP.TILED.WINDOW": "pyramid",
                                      "MODEL.CATSEG_HIP.TILED.GLOBAL": "True"}))
    assert (m.tiled_window, m.tiled_global) == ("pyramid", True)
    with pytest.raises(ValueError, match="window"):
        build_model(tiny_cfg(**on, **{"MODEL.CATSEG_HIP.TILED.WINDOW": "hann"}))
    big = {"MODEL.CATSEG_HIP.TILED.ENABLED": "True", "MODEL.CATSEG_HIP.TILED.TILE": "2080",
           "MODEL.CATSEG_HIP.TILED.STRIDE": "1040"}
    assert build_model(tiny_cfg(**big)).tiled_tile == 2080         # fine for "uniform"
    with pytest.raises(ValueError, match="2048"):
        build_model(tiny_cfg(**big, **{"MODEL.CATSEG_HIP.TILED.WINDOW": "pyramid"}))
