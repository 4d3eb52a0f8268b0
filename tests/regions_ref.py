"""The numpy / scipy restatement of the connected-region and sieve contracts, which
ops.label_regions / ops.sieve_labels are held to exactly.  A plain module (imported from the test files), not a
conftest; tests/test_label_regions_cpu.py checks it against hand-written answers.

Regions: maximal sets of pixels of equal folded label connected under connectivity 4 or 8, numbered in row-major
order of their first pixel.  Sieve (one pass): a region of area < min_area takes the folded label of the touching
region of area >= min_area with the largest area, ties to the smallest region number; other pixels keep their value."""
import numpy as np
from scipy import ndimage

_STRUCT = {4: ndimage.generate_binary_structure(2, 1), 8: ndimage.generate_binary_structure(2, 2)}
# the forward half of the neighbourhood: every unordered neighbour pair once
_FORWARD = {4: ((0, 1), (1, 0)), 8: ((0, 1), (1, 0), (1, -1), (1, 1))}


def fold(m, clamp_pred=-1):
    m = np.asarray(m).astype(np.int64)
    return np.where(m >= clamp_pred, clamp_pred, m) if clamp_pred >= 0 else m


def regions(m, connectivity=8, clamp_pred=-1, score=None):
    """(region_ids (H, W) int32, table) of the map m: table = dict of label, area, first (R,) int32, bbox (R, 4) int32
    [x0, y0, x1, y1] (x1, y1 exclusive) and, with score, score_q16 (R,) int64 and score (R,) float32 (the mean)."""
    f = fold(m, clamp_pred)
    H, W = f.shape
    comp = np.zeros((H, W), np.int64)               # any numbering: per label, offset by what came before
    n = 0
    for v in np.unique(f):
        lab, k = ndimage.label(f == v, structure=_STRUCT[connectivity])
        comp[lab > 0] = lab[lab > 0] + n
        n += k
    flat = comp.ravel() - 1
    first = np.full(n, H * W, np.int64)
    np.minimum.at(first, flat, np.arange(H * W))
    order = np.argsort(first)                       # old number of the region that comes i-th
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n)
    ids = rank[flat].reshape(H, W)
    first = first[order]
    yy, xx = np.divmod(np.arange(H * W), W)
    idf = ids.ravel()
    x0, y0 = np.full(n, W), np.full(n, H)
    x1, y1 = np.zeros(n, np.int64), np.zeros(n, np.int64)
    np.minimum.at(x0, idf, xx)
    np.minimum.at(y0, idf, yy)
    np.maximum.at(x1, idf, xx + 1)
    np.maximum.at(y1, idf, yy + 1)
    table = {"label": f.ravel()[first].astype(np.int32), "area": np.bincount(idf, minlength=n).astype(np.int32),
             "bbox": np.stack([x0, y0, x1, y1], 1).astype(np.int32), "first": first.astype(np.int32)}
    if score is not None:
        q = np.rint(np.asarray(score, np.float32) * np.float32(65536.0)).astype(np.int64)
        q16 = np.zeros(n, np.int64)
        np.add.at(q16, idf, q.ravel())
        table["score_q16"] = q16
        table["score"] = (q16.astype(np.float64) / 65536.0 / table["area"].astype(np.float64)).astype(np.float32)
    return ids.astype(np.int32), table


def sieve(m, min_area, connectivity=8, clamp_pred=-1):
    """The sieved map (int32): np.maximum.at on the packed keys (area << 32) | (0xffffffff - region number)."""
    m = np.asarray(m)
    ids, t = regions(m, connectivity, clamp_pred)
    H, W = ids.shape
    area = t["area"].astype(np.int64)
    keys = np.zeros(len(area), np.uint64)
    for dy, dx in _FORWARD[connectivity]:
        a = ids[:H - dy, max(0, -dx):W - max(0, dx)].ravel().astype(np.int64)
        b = ids[dy:, max(0, dx):W - max(0, -dx)].ravel().astype(np.int64)
        for s, l in ((a, b), (b, a)):               # s the small side, l the large one
            sel = (s != l) & (area[s] < min_area) & (area[l] >= min_area)
            k = (area[l[sel]].astype(np.uint64) << np.uint64(32)) | (np.uint64(0xffffffff) - l[sel].astype(np.uint64))
            np.maximum.at(keys, s[sel], k)
    winner = (np.uint64(0xffffffff) - (keys & np.uint64(0xffffffff))).astype(np.int64)
    takes = keys != 0
    out = m.astype(np.int64).copy()
    pix = takes[ids]
    out[pix] = t["label"].astype(np.int64)[winner[ids[pix]]]
    return out.astype(np.int32)
