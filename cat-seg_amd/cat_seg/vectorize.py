"""Host side of the region outlines (ops.region_outlines; DESIGN.md section 4, "Region outlines"): the rings of
"regions_outlines" grouped by region and written as GeoJSON polygons.  Only the rings cross to the host; no
geometry is tested here: with the ids of `label_regions`, ring_value is the region number, every region has one
exterior ring (ring_area2 > 0), and a hole (ring_area2 < 0) belongs to the exterior ring of its own ring_value.

The simplified rings of ops.simplify_outlines ("regions_outlines_simplified") go through the same two functions:
their "ring_hole" says which rings are holes (a simplified ring's area can be 0 or change sign), and rings that
collapsed (fewer than 3 vertices, or ring_area2 == 0) are left out, a region whose exterior ring collapsed together
with its holes.
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np


def _host(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def rings_by_region(outlines: dict) -> dict:
    """{ring_value: [ring, ...]} of an outlines dict (device tensors or arrays), keys ascending: a stable sort of the
    rings by (value, hole), so the exterior ring comes first, then the holes in start order.  A ring is a dict of
    "vertices" ((n, 2) int32 [x, y], not closed) and "area2" (int).

    With "ring_hole" in the dict (the simplified rings of ops.simplify_outlines) that column decides exterior or
    hole instead of the sign of ring_area2, every ring also carries "hole" (bool), rings of fewer than 3 vertices
    or of area2 == 0 are left out, and so is a region whose exterior ring is left out, together with its holes."""
    off, val, a2, vert = (_host(outlines[k]) for k in ("ring_offset", "ring_value", "ring_area2", "vertices"))
    if "ring_hole" in outlines:
        return _simplified_by_region(off, val, a2, vert, _host(outlines["ring_hole"]) != 0)
    order = np.lexsort((a2 < 0, val))               # lexsort is stable; last key first
    out: dict = {}
    for j in order:
        out.setdefault(int(val[j]), []).append({"vertices": vert[off[j]:off[j + 1]], "area2": int(a2[j])})
    return out


def _simplified_by_region(off, val, a2, vert, hole) -> dict:
    gone = (np.diff(off) < 3) | (a2 == 0)
    lost = set(val[gone & ~hole].tolist())          # regions without an exterior ring
    out: dict = {}
    for j in np.lexsort((hole, val)):
        if gone[j] or int(val[j]) in lost:
            continue
        out.setdefault(int(val[j]), []).append({"vertices": vert[off[j]:off[j + 1]], "area2": int(a2[j]),
                                                "hole": bool(hole[j])})
    return out


def _coords(vertices, transform):
    x, y = vertices[:, 0].astype(np.float64), vertices[:, 1].astype(np.float64)
    if transform is not None:
        a, b, c, d, e, f = (float(v) for v in transform)
        x, y = a * x + b * y + c, d * x + e * y + f
        pts = [[float(u), float(v)] for u, v in zip(x, y)]
    else:
        pts = [[int(u), int(v)] for u, v in zip(x, y)]
    return pts + [pts[0]]                           # GeoJSON linear rings repeat their first position


def outlines_to_geojson(outlines: dict, regions_info: dict, class_names: Optional[Sequence[str]] = None,
                        transform: Optional[Sequence[float]] = None) -> dict:
    """A GeoJSON FeatureCollection with one Polygon feature per region, in region order: "coordinates" = the
    exterior ring, then the region's holes; "properties" = region, label, name (class_names[label] when given and
    in range, else None), area (pixels) and score (None without "score" in regions_info).  `transform`: six numbers
    (a, b, c, d, e, f) mapping lattice (x, y) to world (a x + b y + c, d x + e y + f), the affine order of
    rasterio / GDAL's GetGeoTransform reordered as (a, b, c, d, e, f); None keeps integer lattice coordinates.
    GeoJSON's right-hand rule is met when the transform flips y (e < 0), as north-up rasters do.

    `outlines` may be the simplified dict of ops.simplify_outlines: its "ring_hole" then decides exterior or hole,
    and collapsed rings and the regions whose exterior ring collapsed are omitted (rings_by_region), so there can be
    fewer features than regions; "region" still numbers them as regions_info does."""
    if transform is not None and len(transform) != 6:
        raise ValueError(f"outlines_to_geojson: transform must have 6 numbers, got {len(transform)}")
    groups = rings_by_region(outlines)
    label, area = _host(regions_info["label"]), _host(regions_info["area"])
    score = _host(regions_info["score"]) if "score" in regions_info else None
    simplified = "ring_hole" in outlines
    if simplified:
        values = np.unique(_host(outlines["ring_value"])).tolist()
    else:
        values = sorted(groups)
    if values != list(range(len(label))):
        raise ValueError("outlines_to_geojson: the rings' values are not the region numbers of regions_info")
    features = []
    for r in range(len(label)):
        if simplified:
            if r not in groups:
                continue
            rings = groups[r]
            if rings[0]["hole"] or not all(h["hole"] for h in rings[1:]):
                raise ValueError(f"outlines_to_geojson: region {r} does not have exactly one exterior ring")
        else:
            rings = groups[r]
            if rings[0]["area2"] <= 0 or any(h["area2"] >= 0 for h in rings[1:]):
                raise ValueError(f"outlines_to_geojson: region {r} does not have exactly one exterior ring")
        lab = int(label[r])
        name = class_names[lab] if class_names is not None and 0 <= lab < len(class_names) else None
        features.append({
            "type": "Feature",
            "geometry": {"type": "Polygon", "coordinates": [_coords(g["vertices"], transform) for g in rings]},
            "properties": {"region": r, "label": lab, "name": name, "area": int(area[r]),
                           "score": None if score is None else float(score[r])},
        })
    return {"type": "FeatureCollection", "features": features}
