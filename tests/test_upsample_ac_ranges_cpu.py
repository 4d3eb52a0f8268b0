"""Host check of the gather window catseg_upsample_ac_backward_rows walks (train_norm.hip ac_taps /
upsample_ac_bwd_kernel): for every coarse row q, every fine row whose bilinear taps
(align_corners=True, F.interpolate's source-index rule) put a non-zero weight on q lies inside the
[ylo, yhi] window the kernel loops over -- so the gather sees every contribution the scatter form
(torch's interpolate backward) would add.  fp32 arithmetic as on the device; one axis (the kernel
treats rows and columns alike), all H <= 129 and Hp <= H + 2.

The window is all fine rows when the coarse axis has one entry: ac_taps sends every fine row to
coarse row 0 with weight 1 then, and the inverse scale (H - 1) / (Hp - 1) the window is otherwise
built from does not exist.  `window_scaled_only` is the formula without that case; it misses rows
2 .. H-1 exactly when Hp == 1 and H >= 3, and the last test pins that down."""
import numpy as np

f32 = np.float32
H_MAX = 129


def ac_taps(H, Hp):
    """y0, y1, w1 of every fine row y < H (arrays)."""
    y = np.arange(H, dtype=f32)
    sc = f32(Hp - 1) / f32(H - 1) if H > 1 else f32(0)
    src = (sc * y).astype(f32)
    y0 = np.minimum(src.astype(np.int64), Hp - 1)
    y1 = np.where(y0 + 1 < Hp, y0 + 1, Hp - 1)
    return y0, y1, (src - y0.astype(f32)).astype(f32)


def weights(H, Hp):
    """w[y][q]: the weight of fine row y on coarse row q, summed over its two taps as the kernel does."""
    y0, y1, w1 = ac_taps(H, Hp)
    w = np.zeros((H, Hp), dtype=f32)
    rows = np.arange(H)
    np.add.at(w, (rows, y0), f32(1) - w1)
    np.add.at(w, (rows, y1), w1)
    return w


def window_scaled_only(H, Hp):
    """Per coarse row: fine rows with source coordinate in (q - 1, q + 1], widened by one row each way."""
    q = np.arange(Hp, dtype=f32)
    sy = f32(H - 1) / f32(Hp - 1) if Hp > 1 else f32(0)
    lo = np.floor(((q - f32(1)) * sy).astype(f32)).astype(np.int64) - 1
    hi = np.ceil(((q + f32(1)) * sy).astype(f32)).astype(np.int64) + 1
    return np.maximum(lo, 0), np.minimum(hi, H - 1)


def window(H, Hp):
    """The kernel's window."""
    if Hp == 1:
        return np.zeros(1, dtype=np.int64), np.full(1, H - 1, dtype=np.int64)
    return window_scaled_only(H, Hp)


def misses(win):
    """(H, Hp) pairs for which some contributing fine row lies outside the window of its coarse row."""
    bad = set()
    for H in range(1, H_MAX + 1):
        y = np.arange(H)[:, None]
        for Hp in range(1, H + 3):
            lo, hi = win(H, Hp)
            outside = (y < lo[None, :]) | (y > hi[None, :])
            if np.any((weights(H, Hp) != 0) & outside):
                bad.add((H, Hp))
    return bad


def test_window_covers_every_tap():
    assert misses(window) == set()


def test_weights_of_a_fine_row_sum_to_one():
    for H, Hp in [(24, 12), (7, 3), (6, 1), (9, 4), (4, 4), (3, 5), (1, 1), (129, 131)]:
        assert np.abs(weights(H, Hp).sum(1) - 1).max() < 1e-6


def test_scaled_window_alone_misses_the_single_row_grid():
    assert misses(window_scaled_only) == {(H, 1) for H in range(3, H_MAX + 1)}
