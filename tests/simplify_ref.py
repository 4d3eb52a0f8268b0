"""The sequential restatement of the outline-simplification contract ("Outline
simplification"), which ops.simplify_outlines is held to exactly.  A plain module (imported from the test files), not
a conftest; tests/test_outline_simplify_cpu.py checks it against hand-derived answers.  Built on the rings of
tests/outlines_ref.py's `trace`.  Written from the rules: junctions from the lattice edges, nodes by walking every
ring edge one lattice unit at a time, arcs from the anchors, Douglas-Peucker over each arc with a list of open
segments.  Scores are int64 numpy arithmetic, exact under the contract's limits (H, W, t <= 16384)."""
import math

import numpy as np

import outlines_ref as O

MAX_SIDE = 16384


def tol2_q4(t):
    """round(16 t^2) as the host computes it."""
    return int(math.floor(16.0 * float(t) * float(t) + 0.5))


def junctions(ids):
    """(H + 1, W + 1) bool: at least 3 incident boundary edges, or a map corner."""
    m = np.asarray(ids)
    H, W = m.shape
    pad = np.empty((H + 2, W + 2), object)
    pad[:] = None                                   # outside: differs from every pixel (and from outside: never asked)
    pad[1:-1, 1:-1] = m
    j = np.zeros((H + 1, W + 1), bool)
    for y in range(H + 1):
        for x in range(W + 1):
            nw, ne, sw, se = pad[y, x], pad[y, x + 1], pad[y + 1, x], pad[y + 1, x + 1]
            differ = lambda a, b: a is None or b is None or a != b
            deg = ((x < W and differ(ne, se)) + (x > 0 and differ(nw, sw)) +
                   (y > 0 and differ(nw, ne)) + (y < H and differ(sw, se)))
            j[y, x] = deg >= 3 or (x in (0, W) and y in (0, H))
    return j


def ring_nodes(pts, junc):
    """[(x, y, anchor)] of one ring: its corners in order plus the junctions strictly inside its edges."""
    out = []
    n = len(pts)
    for i, (x0, y0) in enumerate(pts):
        x1, y1 = pts[(i + 1) % n]
        assert (x0 == x1) != (y0 == y1)
        out.append((x0, y0, bool(junc[y0, x0])))
        dx, dy = np.sign(x1 - x0), np.sign(y1 - y0)
        x, y = x0 + dx, y0 + dy
        while (x, y) != (x1, y1):
            if junc[y, x]:
                out.append((int(x), int(y), True))
            x, y = x + dx, y + dy
    return out


def ring_arcs(nodes, W):
    """[(start node, edges)] of one ring, arcs in ring order from its first anchor; a ring without anchors is one
    closed arc from its first node, which is its node of smallest vertex key."""
    n = len(nodes)
    anchors = [i for i, p in enumerate(nodes) if p[2]]
    if not anchors:
        assert min(range(n), key=lambda i: nodes[i][1] * (W + 1) + nodes[i][0]) == 0
        return [(0, n)]
    if len(anchors) == 1:
        return [(anchors[0], n)]
    return [(a, (anchors[(k + 1) % len(anchors)] - a) % n) for k, a in enumerate(anchors)]


def douglas_peucker(P, t2q4, W):
    """Indices kept among the nodes P ((n + 1, 2) int64 [x, y]; P[0] == P[n] for a closed arc): both ends, and the
    interior nodes the contract keeps."""
    n = len(P) - 1
    keep = {0, n}
    todo = [(0, n)]
    v = P[:, 1] * (W + 1) + P[:, 0]
    while todo:
        i, j = todo.pop()
        if j - i < 2:
            continue
        d = P[j] - P[i]
        rel = P[i + 1:j] - P[i]
        if d[0] == 0 and d[1] == 0:
            score, L = rel[:, 0] ** 2 + rel[:, 1] ** 2, 1
        else:
            score, L = (d[0] * rel[:, 1] - d[1] * rel[:, 0]) ** 2, int(d[0] ** 2 + d[1] ** 2)
        m = int(score.max())
        if 16 * m <= t2q4 * L:
            continue
        tied = np.flatnonzero(score == m)
        k = i + 1 + int(tied[np.argmin(v[i + 1:j][tied])])
        keep.add(k)
        todo += [(i, k), (k, j)]
    return sorted(keep)


def on_frame(a, b, H, W):
    """The edge a -> b lies on the map frame."""
    return (a[0] == b[0] and a[0] in (0, W)) or (a[1] == b[1] and a[1] in (0, H))


def detail(ids, outlines, t):
    """Per ring a dict: "nodes" [(x, y, anchor)], "arcs" [{"start", "len", "frame", "pos": kept
    positions 0 .. len inside the arc, "kept": their node numbers}], "kept"
    (sorted node numbers of the whole ring)."""
    m = np.asarray(ids)
    H, W = m.shape
    assert H <= MAX_SIDE and W <= MAX_SIDE and 0 <= t <= MAX_SIDE
    junc = junctions(m)
    q = tol2_q4(t)
    rings = []
    for r in range(len(outlines["ring_value"])):
        nodes = ring_nodes(O.ring(outlines, r), junc)
        n = len(nodes)
        kept, arcs = set(), []
        for start, length in ring_arcs(nodes, W):
            idx = [(start + k) % n for k in range(length + 1)]
            P = np.asarray([nodes[i][:2] for i in idx], np.int64)
            inner = P[1:-1]
            assert len({tuple(p) for p in inner.tolist()}) == len(inner)       # a repeated vertex is an anchor
            pos = douglas_peucker(P, q, W)
            k = [idx[i] for i in pos]
            frame = all(on_frame(P[i], P[i + 1], H, W) for i in range(length))
            arcs.append({"start": start, "len": length, "frame": frame, "pos": pos, "kept": k})
            kept.update(k)
        rings.append({"nodes": nodes, "arcs": arcs, "kept": sorted(kept)})
    return rings


def simplify(ids, outlines, t, rings=None):
    """The simplified rings: dict of ring_offset (NR + 1,) int32, ring_value (NR,) int32, ring_area2 (NR,) int64,
    ring_hole (NR,) uint8 and vertices (K', 2) int32 [x, y]; every ring holds its kept nodes in the source ring's
    order."""
    rings = detail(ids, outlines, t) if rings is None else rings
    off, area2, verts = [0], [], []
    for ring in rings:
        pts = [ring["nodes"][i][:2] for i in ring["kept"]]
        n = len(pts)
        area2.append(sum(pts[i][0] * pts[(i + 1) % n][1] - pts[(i + 1) % n][0] * pts[i][1] for i in range(n)))
        verts += pts
        off.append(len(verts))
    return {"ring_offset": np.asarray(off, np.int32),
            "ring_value": np.asarray(outlines["ring_value"], np.int32).copy(),
            "ring_area2": np.asarray(area2, np.int64),
            "ring_hole": (np.asarray(outlines["ring_area2"]) < 0).astype(np.uint8),
            "vertices": np.asarray(verts, np.int32).reshape(-1, 2)}


def count_nodes(rings):
    return sum(len(r["nodes"]) for r in rings)
