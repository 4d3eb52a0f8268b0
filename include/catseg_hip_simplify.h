/* C ABI of the outline simplifier of libcatseg_hip.so; catseg_hip.h includes this header, which
 * follows its conventions: device pointers, `stream` a hipStream_t, 0 on success, CATSEG_ERR_ARG
 * for a bad argument (catseg_last_error() has the text), CATSEG_ERR_HIP for a failed launch. */
#ifndef CATSEG_HIP_SIMPLIFY_H
#define CATSEG_HIP_SIMPLIFY_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------
 * catseg_outline_simplify_* — the rings of catseg_region_outlines_write simplified on the device
 * by Douglas-Peucker, arc by arc: the boundary between two regions is one arc, so both
 * neighbours keep the same vertices.  No counterpart in the reference (its users simplify each
 * polygon alone on the host); the contract is DESIGN.md section 4, "Outline simplification".
 *   Inputs: the map ids [H][W] (row stride ld), the rings made for it (ring_offset of rings + 1
 *   ints, vertices of corners x 2 ints, and for _write ring_value and ring_area2), a tolerance t
 *   in pixels.  Limits: 1 <= H, W <= 16384, 0 <= t <= 16384, 1 <= rings <= corners.
 *   Junction: a lattice vertex with at least 3 incident boundary edges (the two pixels across an
 *   edge differ; outside the map differs from every pixel), or a map corner; connectivity plays no
 *   part (a diagonal pinch has degree 4).  Nodes of a ring: its corners in ring order plus every
 *   junction strictly inside one of its straight edges, in order along the edge; N = all nodes.  A
 *   node on a junction is an anchor and always kept.  Arcs: a ring with a >= 2 anchors has a arcs,
 *   each from one anchor to the next in ring order, wrapping at the ring's end; with 1 anchor one
 *   closed arc from it to itself; with none one closed arc from its first node (its node of
 *   smallest vertex key v = y (W + 1) + x) to itself.
 *   Douglas-Peucker in exact integers: for nodes P_i .. P_j of an arc, j - i >= 2, an interior P_k
 *   scores cross(P_j - P_i, P_k - P_i)^2 with L = |P_j - P_i|^2, or |P_k - P_i|^2 with L = 1 when
 *   P_i == P_j.  With m the largest score: 16 m <= tol2_q4 L drops every interior node, else the
 *   node of score m (ties: smallest v) is kept and both sides recurse; tol2_q4 = floor(16 t^2 +
 *   0.5), computed on the host.  Score and tie-break do not depend on the walking direction.
 *   Output: the same rings in the same order, each the kept nodes in the source ring's order:
 *   ring_offset' (rings + 1), ring_value (copied), ring_area2' (the int64 shoelace sum of the kept
 *   vertices; may be 0 or change sign), ring_hole (uint8, 1 where the source ring_area2 < 0) and
 *   vertices' (K' x 2).  A ring may end with 1 or 2 vertices.  Every result is a function of the
 *   input alone.  Crossings at large tolerances are not prevented; areas are not preserved.
 *   Two synchronising reads (N, K') size everything.
 *
 * catseg_outline_simplify_workspace  nodes < 0: bytes of the map workspace for (H, W, corners);
 *     nodes >= 0: bytes of the node workspace for that many corners and nodes; 0 for H or W
 *     outside 1 .. 16384, corners outside 1 .. 4 (H + 1) (W + 1) or nodes outside corners ..
 *     4 (H + 1) (W + 1).
 * catseg_outline_simplify_count      builds the junction bitmaps of the map, counts per corner
 *     itself and the junctions up to the next corner of its ring, and scans.  Afterwards
 *     ((int32_t*)workspace)[0] = N.  workspace: 16-byte aligned device memory.
 * catseg_outline_simplify_run        with the map workspace _count left for the same map and rings
 *     and nodes = N: writes the nodes, finds the arcs, runs Douglas-Peucker (no launch per round: a
 *     wave per arc, a workgroup per arc of at least 512 edges; every loop bounded by the arc's length)
 *     and scans the keep flags.  Afterwards ((int32_t*)node_workspace)[1] = K'.  Leaves the map
 *     workspace as it is.
 * catseg_outline_simplify_write      with the node workspace _run left: ring_offset[j] for
 *     j <= min(rings, ring_capacity) (the buffer has ring_capacity + 1 elements), ring_value[j],
 *     ring_area2[j] and ring_hole[j] for j < min(rings, ring_capacity), and vertices [2 p],
 *     [2 p + 1] = x, y of the kept node at position p < vertex_capacity (vertices: 8-byte
 *     aligned).  Never stores beyond a capacity, whatever the rings or the workspace hold; leaves
 *     the workspace as it is.
 * Every entry returns nonzero for bad arguments before anything is launched.
 * ------------------------------------------------------------------------- */
int64_t catseg_outline_simplify_workspace(int64_t H, int64_t W, int64_t corners, int64_t nodes);
int catseg_outline_simplify_count(const int32_t* ids, int64_t H, int64_t W, int64_t ld,
                                  const int32_t* ring_offset, int64_t rings, const int32_t* vertices,
                                  int64_t corners, void* workspace, int64_t workspace_bytes,
                                  void* stream);
int catseg_outline_simplify_run(const int32_t* ring_offset, int64_t rings, const int32_t* vertices,
                                int64_t corners, int64_t H, int64_t W, double tolerance,
                                const void* workspace, int64_t workspace_bytes, int64_t nodes,
                                void* node_workspace, int64_t node_workspace_bytes, void* stream);
int catseg_outline_simplify_write(const void* node_workspace, int64_t node_workspace_bytes, int64_t H,
                                  int64_t W, int64_t corners, int64_t nodes, int64_t rings,
                                  const int32_t* ring_value_in, const int64_t* ring_area2_in,
                                  int32_t* ring_offset, int32_t* ring_value, int64_t* ring_area2,
                                  uint8_t* ring_hole, int64_t ring_capacity, int32_t* vertices,
                                  int64_t vertex_capacity, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CATSEG_HIP_SIMPLIFY_H */
