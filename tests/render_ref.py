"""Sequential numpy restatement of the label-map renderer's contract (include/catseg_hip_render.h; DESIGN.md
section 4, "Rendering"), written from the contract and not from the kernel: whole-array integer steps in the order
the contract gives them, the edge mask by comparing every shifted copy of the map, the cells by slicing.  The GPU
tests hold `ops.render_labels` to it bit for bit.  A plain module (imported as `render_ref`), not a conftest."""
import numpy as np


def rgb(v):
    """(r, g, b) or packed 0xRRGGBB -> int64 array of 3."""
    if isinstance(v, (int, np.integer)):
        return np.array([(v >> 16) & 255, (v >> 8) & 255, v & 255], np.int64)
    return np.asarray(v, np.int64).reshape(3)


def fold(labels, clamp_pred=-1):
    m = np.asarray(labels).astype(np.int64)
    return np.minimum(m, clamp_pred) if clamp_pred >= 0 else m


def s8(score):
    """256 for score >= 1, int(score * 256) for score > 0, else 0 (NaN compares false both times)."""
    s = np.asarray(score, np.float32)
    out = np.zeros(s.shape, np.int64)
    with np.errstate(invalid="ignore"):
        mid = (s > 0) & ~(s >= 1)
        out[mid] = np.floor(s[mid].astype(np.float64) * 256).astype(np.int64)
        out[s >= 1] = 256
    return out


def gray(img):
    """PIL's convert("L") of an (..., 3) uint8 array."""
    i = np.asarray(img).astype(np.int64)
    return (19595 * i[..., 0] + 38470 * i[..., 1] + 7471 * i[..., 2] + 32768) >> 16


def blend(i, c, a):
    return (np.asarray(i, np.int64) * (256 - a) + np.asarray(c, np.int64) * a + 128) >> 8


def source_index(n, m):
    """Source index of each of n destination pixels onto m source pixels: nearest by pixel centre."""
    x = np.arange(n, dtype=np.int64)
    return np.minimum(((2 * x + 1) * m) // (2 * n), m - 1)


def edge_mask(folded, edge_px):
    """True where a pixel of the map within Chebyshev distance edge_px holds another label; the outside of the map
    holds nothing."""
    m = np.asarray(folded)
    H, W = m.shape
    out = np.zeros((H, W), bool)
    for dy in range(-edge_px, edge_px + 1):
        for dx in range(-edge_px, edge_px + 1):
            if abs(dy) >= H or abs(dx) >= W:            # the shifted copy lies outside the map altogether
                continue
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
            yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
            out[ys, xs] |= m[ys, xs] != m[yq, xq]
    return out


def cell_mean(full, factor):
    """(H, W, 3) int -> (ceil(H / f), ceil(W / f), 3) uint8: (sum + n // 2) // n per cell, the last cells partial."""
    H, W, _ = full.shape
    if factor == 1:                                     # a cell is its pixel
        return full.astype(np.uint8)
    Ho, Wo = -(-H // factor), -(-W // factor)
    out = np.zeros((Ho, Wo, 3), np.uint8)
    for Y in range(Ho):
        for X in range(Wo):
            cell = full[Y * factor:min((Y + 1) * factor, H), X * factor:min((X + 1) * factor, W)].reshape(-1, 3)
            n = cell.shape[0]
            out[Y, X] = (cell.sum(0) + n // 2) // n
    return out


def full_colors(labels, palette, *, image=None, gray_image=True, alpha_q8=128, score=None, gt=None, ignore_label=255,
                error_rgb=(255, 0, 0), ignore_rgb=(0, 0, 0), edge_px=0, edge_rgb=(255, 255, 255),
                other_rgb=(0, 0, 0), clamp_pred=-1):
    """The full-resolution colours, (H, W, 3) int64.  image: (ih, iw, 3) uint8 (HWC)."""
    l = fold(labels, clamp_pred)
    H, W = l.shape
    pal = np.asarray(palette).astype(np.int64).reshape(-1, 3)
    P = pal.shape[0]
    inside = (l >= 0) & (l < P)
    c = np.where(inside[..., None], pal[np.where(inside, l, 0)], rgb(other_rgb)[None, None, :])
    a = np.full((H, W), int(alpha_q8), np.int64)
    if gt is not None:
        g = np.asarray(gt).astype(np.int64)
        c = np.where((g != l)[..., None], rgb(error_rgb)[None, None, :], c)
        c = np.where((g == ignore_label)[..., None], rgb(ignore_rgb)[None, None, :], c)
    if score is not None:
        a = (a * s8(score)) >> 8
    if image is not None:
        img = np.asarray(image)
        ih, iw, _ = img.shape
        src = img[source_index(H, ih)][:, source_index(W, iw)].astype(np.int64)
        if gray_image:
            src = np.repeat(gray(src)[..., None], 3, axis=2)
        c = blend(src, c, a[..., None])
    if edge_px > 0:
        c = np.where(edge_mask(l, edge_px)[..., None], rgb(edge_rgb)[None, None, :], c)
    return c


def render(labels, palette, *, factor=1, **kw):
    """(Ho, Wo, 3) uint8."""
    return cell_mean(full_colors(labels, palette, **kw), factor)
