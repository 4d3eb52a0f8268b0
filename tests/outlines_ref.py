"""The sequential restatement of the region-outline contract ("Region outlines"), which
ops.region_outlines is held to exactly.  A plain module (imported from the test files), not a conftest;
tests/test_region_outlines_cpu.py checks it against hand-written answers.  Written from the rules: every directed
boundary edge is enumerated, the successor rule is applied one lattice unit at a time, and the cycles are read off.

Lattice: x in 0..W, y in 0..H, y down; directions E=0, S=1, W=2, N=3.  A directed unit edge is a boundary edge of
value r when the pixel on its right exists and has value r and the pixel on its left differs or is outside."""
import numpy as np

DX = (1, 0, -1, 0)
DY = (0, 1, 0, -1)


def _pixel(m, y, x):
    H, W = m.shape
    return int(m[y, x]) if 0 <= y < H and 0 <= x < W else None


def _sides(m, x, y, d):
    """(right, left) pixel of the unit edge that starts at vertex (x, y) and heads d."""
    if d == 0:                                      # heading E: right is below, left above
        return _pixel(m, y, x), _pixel(m, y - 1, x)
    if d == 1:                                      # heading S: right is the pixel to the left of the edge
        return _pixel(m, y, x - 1), _pixel(m, y, x)
    if d == 2:                                      # heading W: right is above
        return _pixel(m, y - 1, x - 1), _pixel(m, y, x - 1)
    return _pixel(m, y - 1, x), _pixel(m, y - 1, x - 1)   # heading N: right is the pixel to the right


def _boundary(m, x, y, d):
    """The value r of the boundary edge from (x, y) heading d, or None."""
    r, l = _sides(m, x, y, d)
    return r if r is not None and l != r else None


def _turn(m, x, y, d, r, connectivity):
    """Outgoing direction of the edge of value r that arrives at vertex (x, y) with direction d."""
    # the pixels ahead of the vertex: those beside the edge that would go straight on
    a, b = _sides(m, x, y, d)                       # ahead-right, ahead-left
    ar, br = a == r, b == r
    if ar and br:
        return (d + 3) % 4
    if ar:
        return d
    if br:
        return (d + 3) % 4 if connectivity == 8 else (d + 1) % 4
    return (d + 1) % 4


def trace(ids, connectivity=8):
    """The rings of the map: dict of ring_offset (NR + 1,) int32, ring_value (NR,) int32, ring_area2 (NR,) int64,
    vertices (K, 2) int32 [x, y]."""
    m = np.asarray(ids)
    assert m.ndim == 2 and connectivity in (4, 8)
    H, W = m.shape
    todo = {}                                       # (end vertex x, y, d) of every boundary edge -> its value
    for y in range(H + 1):
        for x in range(W + 1):
            for d in range(4):
                r = _boundary(m, x, y, d)
                if r is not None:
                    todo[(x + DX[d], y + DY[d], d)] = r
    key = lambda c: (c[1] * (W + 1) + c[0]) * 4 + c[2]
    rings = []
    while todo:
        first = next(iter(todo))
        r = todo[first]
        corners, cur = [], first
        while True:
            assert todo.pop(cur) == r               # a permutation: every edge is on exactly one ring
            x, y, d = cur
            o = _turn(m, x, y, d, r, connectivity)
            if o != d:
                corners.append(cur)
            cur = (x + DX[o], y + DY[o], o)
            if cur == first:
                break
        k = min(range(len(corners)), key=lambda i: key(corners[i]))
        corners = corners[k:] + corners[:k]
        rings.append((key(corners[0]), r, [(c[0], c[1]) for c in corners]))
    rings.sort(key=lambda t: t[0])
    off, val, area2, verts = [0], [], [], []
    for _, r, pts in rings:
        n = len(pts)
        area2.append(sum(pts[i][0] * pts[(i + 1) % n][1] - pts[(i + 1) % n][0] * pts[i][1] for i in range(n)))
        val.append(r)
        verts += pts
        off.append(len(verts))
    return {"ring_offset": np.asarray(off, np.int32), "ring_value": np.asarray(val, np.int32),
            "ring_area2": np.asarray(area2, np.int64),
            "vertices": np.asarray(verts, np.int32).reshape(-1, 2)}


def ring(out, j):
    """Vertices of ring j as a list of (x, y)."""
    o = np.asarray(out["ring_offset"])
    return [tuple(int(c) for c in p) for p in np.asarray(out["vertices"])[o[j]:o[j + 1]]]


def fill(out, value, H, W):
    """Even-odd fill of the rings of `value` as an (H, W) bool mask, from the rings' vertical segments: a segment at
    lattice column x between rows y0 and y1 toggles every pixel of those rows at or right of x."""
    acc = np.zeros((H, W), bool)
    for j in np.flatnonzero(np.asarray(out["ring_value"]) == value):
        pts = ring(out, j)
        for i, (x0, y0) in enumerate(pts):
            x1, y1 = pts[(i + 1) % len(pts)]
            if x0 == x1 and y0 != y1:
                acc[min(y0, y1):max(y0, y1), x0:] ^= True
    return acc
