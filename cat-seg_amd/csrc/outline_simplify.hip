// Outline simplification: the rings of catseg_region_outlines_write simplified by Douglas-Peucker on the device,
// arc by arc, so that the two regions on either side of a shared boundary keep the same vertices.  No counterpart
// in the reference; the contract is DESIGN.md section 4 ("Outline simplification"), the index and score logic
// outline_simplify_logic.h, which a host program runs too.
//
// Count, scan, write, as the outlines are traced.  Two workspaces, as two sizes are only known on the device:
//   map workspace (a function of H, W and K), filled by catseg_outline_simplify_count
//     junctions  one wave per word of 64 vertices of a lattice row: the junction flag of every vertex from its
//                2 x 2 pixels, the row bitmap by __ballot, the column bitmap by a 64-bit atomic OR (zeroed by a
//                memset on the stream).
//     count      one thread per source corner: 1 + the junctions strictly between it and the next corner of its
//                ring (popcounts over bitmap words), then scan_i32.h: node positions, N at word 0.
//   node workspace (a function of K and N), filled by catseg_outline_simplify_run
//     nodes      per corner: its node and the junction nodes behind it (packed x | y << 16, ring number, keep =
//                the node lies on a junction); per ring the position of its first node.
//     arcs       the anchor bitmap over node positions by __ballot; per anchor the distance to the next anchor of
//                its ring (found in the bitmap a word at a time, wrapping at the ring's end), per ring without
//                anchors one closed arc from its first node; arcs of at least 2 edges are compacted into a list
//                (scan), their number at word 2.
//     simplify   a wave per arc below OS_BLOCK_LEN edges, a workgroup per longer arc, both striding over the
//                list: os_douglas_peucker with lanes striding over the open segment and a cross-lane reduction
//                of (score, -v); the stack lives in the arc's own node slots and belongs to thread 0.  Nothing
//                waits for another workgroup, and every loop is bounded by the arc's length.
//     compact    scan of the keep flags: K' at word 1; the kept nodes in output order.
//   catseg_outline_simplify_write
//     per ring its offset, value and hole flag; per kept node its vertex and its shoelace term, added to the
//     ring's area2 by a 64-bit integer atomic (the same bits in any order).
// Every number read from a workspace or from the caller's rings is bounded before it indexes anything, so foreign
// or stale contents yield wrong rings, never a store outside the caller's capacities or a load outside the buffers.
#include "common.h"
#include "capi.h"
#include "outline_simplify_logic.h"
#include "scan_i32.h"

#include <math.h>

namespace {

constexpr int OS_HEAD = 4;                         // header ints of both workspaces: N | K' | arcs | -

struct OsMap {                                     // pixel (y, x) of the (strided) map
  const int32_t* ids;
  int64_t ld;
  DEV int operator()(int y, int x) const { return ids[(int64_t)y * ld + x]; }
};

bool os_shape_ok(int64_t H, int64_t W) { return H > 0 && W > 0 && H <= OS_MAX_SIDE && W <= OS_MAX_SIDE; }

int64_t os_pad4(int64_t n) { return (n + 3) / 4 * 4; }
int64_t os_blocks(int64_t n) { return (n + LR_SCAN - 1) / LR_SCAN; }

// map workspace (ints): head | cnt k4 | bsum nb4 | rowbits 2 * nwords | colbits 2 * (W + 1) * col_words
struct OsShape {
  int64_t vw, vh, row_words, col_words, nwords, k4, nb4;
  int64_t bytes() const {
    return (OS_HEAD + k4 + nb4 + 2 * nwords + 2 * vw * col_words) * (int64_t)sizeof(int32_t);
  }
};
OsShape os_shape(int64_t H, int64_t W, int64_t K) {
  OsShape s;
  s.vw = W + 1;
  s.vh = H + 1;
  s.row_words = (s.vw + RO_WORD - 1) / RO_WORD;
  s.col_words = (s.vh + RO_WORD - 1) / RO_WORD;
  s.nwords = s.vh * s.row_words;
  s.k4 = os_pad4(K);
  s.nb4 = os_pad4(os_blocks(K));
  return s;
}

// node workspace (ints): head | ringstart r4 | node | ring | keep | kpos | arclen | aidx | arcs | kxy (n4 each) |
//                        stack 2 * n4 | abits 2 * nw | bsum nb4
struct OsNodes {
  int64_t r4, n4, nw, nb4;
  int64_t bytes() const { return (OS_HEAD + r4 + 10 * n4 + 2 * nw + nb4) * (int64_t)sizeof(int32_t); }
};
OsNodes os_nodes(int64_t K, int64_t N) {
  OsNodes s;
  s.r4 = os_pad4(K + 1);                           // at most K rings (NR <= K is checked), and the closing entry
  s.n4 = os_pad4(N);
  s.nw = os_pad4((N + RO_WORD - 1) / RO_WORD) / 2 * 2;
  s.nb4 = os_pad4(os_blocks(N));
  return s;
}
struct OsNodePtrs {
  int32_t *head, *ringstart, *node, *ring, *keep, *kpos, *arclen, *aidx, *arcs, *kxy, *bsum;
  int2* stack;
  unsigned long long* abits;
};
OsNodePtrs os_node_ptrs(void* ws, const OsNodes& s) {
  OsNodePtrs p;
  p.head = (int32_t*)ws;
  p.ringstart = p.head + OS_HEAD;
  p.node = p.ringstart + s.r4;
  p.ring = p.node + s.n4;
  p.keep = p.ring + s.n4;
  p.kpos = p.keep + s.n4;
  p.arclen = p.kpos + s.n4;
  p.aidx = p.arclen + s.n4;
  p.arcs = p.aidx + s.n4;
  p.kxy = p.arcs + s.n4;
  p.stack = (int2*)(p.kxy + s.n4);
  p.abits = (unsigned long long*)(p.kxy + s.n4 + 2 * s.n4);
  p.bsum = (int32_t*)(p.abits + s.nw);
  return p;
}

DEV int os_clamp(int v, int lo, int hi) { return max(lo, min(v, hi)); }

// ---------------------------------------------------------------------------------------------------- count
__global__ __launch_bounds__(256) void os_junction_kernel(const int32_t* __restrict__ ids, int H, int W, int64_t ld,
                                                          int row_words, int col_words, int nwords,
                                                          unsigned long long* __restrict__ rowbits,
                                                          unsigned long long* colbits) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= nwords) return;                        // wave-uniform
  const int y = gw / row_words, xw = gw - y * row_words, x = xw * RO_WORD + lane;
  bool junction = false;
  if (x <= W) {
    int q[4];
    const unsigned have = ro_quad(OsMap{ids, ld}, x, y, H, W, q);
    junction = os_junction(q, have, x, y, H, W);
  }
  const unsigned long long m = __ballot(junction);
  if (lane == 0) rowbits[gw] = m;
  // x <= W here, y <= H: inside [W + 1][col_words]
  if (junction)
    __hip_atomic_fetch_or(colbits + (int64_t)x * col_words + (y >> 6), 1ull << (y & 63), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
}

// The edge that leaves corner i of the caller's rings: its ring, the ring's corner range [lo, hi) and the next
// corner j, all inside [0, K); line = the bit line the edge lies on and a, b its ends along it (null when the two
// corners are not the ends of a lattice-aligned edge inside the map).
struct OsEdge {
  int ring, lo, hi, j, p0, a, b;
  const unsigned long long* line;
};
DEV OsEdge os_edge(const int32_t* __restrict__ ring_offset, int NR, const int2* __restrict__ vertices, int K, int i,
                   int H, int W, int row_words, int col_words, const unsigned long long* __restrict__ rowbits,
                   const unsigned long long* __restrict__ colbits) {
  OsEdge e;
  e.ring = os_ring_of(ring_offset, NR, i);
  e.lo = os_clamp(ring_offset[e.ring], 0, K);
  e.hi = os_clamp(ring_offset[e.ring + 1], 0, K);
  e.j = i + 1 < e.hi ? i + 1 : e.lo;
  if (e.j < 0 || e.j >= K) e.j = i;
  const int2 v0 = vertices[i], v1 = vertices[e.j];
  const bool ok = v0.x >= 0 && v0.x <= W && v0.y >= 0 && v0.y <= H && v1.x >= 0 && v1.x <= W && v1.y >= 0 && v1.y <= H;
  e.p0 = ok ? os_pack(v0.x, v0.y) : 0;
  e.line = nullptr;
  e.a = e.b = 0;
  if (ok && v0.y == v1.y && v0.x != v1.x) {
    e.line = rowbits + (int64_t)v0.y * row_words;
    e.a = v0.x;
    e.b = v1.x;
  } else if (ok && v0.x == v1.x && v0.y != v1.y) {
    e.line = colbits + (int64_t)v0.x * col_words;
    e.a = v0.y;
    e.b = v1.y;
  }
  return e;
}

__global__ __launch_bounds__(256) void os_count_kernel(const int32_t* __restrict__ ring_offset, int NR,
                                                       const int2* __restrict__ vertices, int K, int H, int W,
                                                       int row_words, int col_words,
                                                       const unsigned long long* __restrict__ rowbits,
                                                       const unsigned long long* __restrict__ colbits,
                                                       int32_t* __restrict__ cnt) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= K) return;
  const int i = (int)i64;
  const OsEdge e = os_edge(ring_offset, NR, vertices, K, i, H, W, row_words, col_words, rowbits, colbits);
  cnt[i] = 1 + (e.line ? os_count_open(e.line, e.a, e.b) : 0);
}

// ------------------------------------------------------------------------------------------------------ run
__global__ __launch_bounds__(256) void os_node_kernel(const int32_t* __restrict__ ring_offset, int NR,
                                                      const int2* __restrict__ vertices, int K, int H, int W,
                                                      int row_words, int col_words,
                                                      const int32_t* __restrict__ map_ws,
                                                      const int32_t* __restrict__ off,
                                                      const unsigned long long* __restrict__ rowbits,
                                                      const unsigned long long* __restrict__ colbits, int cap,
                                                      int32_t* __restrict__ head, int32_t* __restrict__ ringstart,
                                                      int32_t* __restrict__ node, int32_t* __restrict__ ring,
                                                      int32_t* __restrict__ keep) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = os_clamp(map_ws[0], 0, cap);
  if (i64 == 0) {
    head[0] = n;
    ringstart[NR] = n;                             // NR <= K: inside ringstart's K + 1 entries
  }
  if (i64 >= K) return;
  const int i = (int)i64;
  const OsEdge e = os_edge(ring_offset, NR, vertices, K, i, H, W, row_words, col_words, rowbits, colbits);
  int p = off[i];
  if (p < 0 || p >= n) return;
  if (i == e.lo) ringstart[e.ring] = p;
  node[p] = e.p0;
  ring[p] = e.ring;
  keep[p] = os_bit(rowbits + (int64_t)os_y(e.p0) * row_words, os_x(e.p0)) ? 1 : 0;
  if (!e.line) return;
  const bool horizontal = e.line < colbits;        // the row bitmaps come first in the workspace
  const int fixed = horizontal ? os_y(e.p0) : os_x(e.p0);
  int cur = e.a;
  for (int it = 0; it <= OS_MAX_SIDE; ++it) {      // an edge holds fewer vertices than that
    cur = os_next_open(e.line, cur, e.b);
    if (cur < 0 || ++p >= n) break;
    node[p] = horizontal ? os_pack(cur, fixed) : os_pack(fixed, cur);
    ring[p] = e.ring;
    keep[p] = 1;
  }
}

// the anchor bitmap over node positions: a wave per word; words beyond N hold 0
__global__ __launch_bounds__(256) void os_anchor_kernel(const int32_t* __restrict__ head, int cap, int nw,
                                                        const int32_t* __restrict__ keep,
                                                        unsigned long long* __restrict__ abits) {
  const int lane = threadIdx.x & 63;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= nw) return;
  const int n = os_clamp(head[0], 0, cap);
  const int64_t p = w * RO_WORD + lane;
  const unsigned long long m = __ballot(p < n && keep[p] != 0);
  if (lane == 0) abits[w] = m;
}

// arclen[p] = the edges of the arc that starts at node p (0: none starts there), aidx[p] = 1 for an arc that can
// lose a node (at least 2 edges); the first node of a ring without anchors is kept
__global__ __launch_bounds__(256) void os_arc_kernel(const int32_t* __restrict__ head, int cap, int NR,
                                                     const int32_t* __restrict__ ringstart,
                                                     const int32_t* __restrict__ ring,
                                                     const unsigned long long* __restrict__ abits,
                                                     int32_t* __restrict__ keep, int32_t* __restrict__ arclen,
                                                     int32_t* __restrict__ aidx) {
  const int64_t p64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p64 >= cap) return;
  const int p = (int)p64;
  const int n = os_clamp(head[0], 0, cap);
  int len = 0;
  if (p < n) {
    const int r = os_clamp(ring[p], 0, NR - 1);
    const int s = os_clamp(ringstart[r], 0, n), e = os_clamp(ringstart[r + 1], 0, n);
    if (s <= p && p < e) {
      if (keep[p]) {
        int q = os_next_open(abits, p, e);
        if (q < 0) q = os_first_in(abits, s, p + 1);         // p itself at the latest
        len = q > p ? q - p : q >= s ? q + (e - s) - p : 0;
      } else if (p == s && os_first_in(abits, s, e) < 0) {
        len = e - s;
        keep[p] = 1;
      }
    }
  }
  arclen[p] = len;
  aidx[p] = len >= 2 ? 1 : 0;
}

__global__ __launch_bounds__(256) void os_arc_list_kernel(const int32_t* __restrict__ head, int cap,
                                                          const int32_t* __restrict__ arclen,
                                                          const int32_t* __restrict__ aidx,
                                                          int32_t* __restrict__ arcs) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= os_clamp(head[0], 0, cap) || arclen[p] < 2) return;
  const int a = aidx[p];
  if (a >= 0 && a < cap) arcs[a] = (int)p;
}

// One arc for os_douglas_peucker, run by a group of T threads (a wave or a workgroup of 256) in lockstep: every
// thread holds the same i, j, sp; thread 0 owns the stack and the keep flags.  Node k of the arc is node
// slot(k) = s + (p - s + k) % ringlen of the workspace; the arc's stack entries live at the same slots.
template <int T>
struct OsArc {
  const int32_t* __restrict__ nodes;
  int32_t* keep_flags;
  int2* stack;
  int s, ringlen, first, W, tid;
  OsBest* sh;                                      // T == 256: 4 wave results + 1 broadcast slot

  DEV int slot(int k) const {
    int o = first + k;                             // first in [0, ringlen), k in [0, ringlen]
    if (o >= ringlen) o -= ringlen;
    if (o >= ringlen) o -= ringlen;
    return s + o;
  }
  DEV int node_at(int k) const { return nodes[slot(k)]; }
  DEV int node(int k) const { return node_at(k); }
  DEV void keep(int k) {
    if (tid == 0) keep_flags[slot(k)] = 1;
  }
  DEV void push(int sp, int i, int j) {
    if (tid == 0) stack[slot(sp)] = make_int2(i, j);
  }
  DEV void pop(int sp, int& i, int& j) {
    int2 e = make_int2(0, 0);
    if (tid == 0) e = stack[slot(sp)];
    if (T == 64) {
      i = __shfl(e.x, 0, 64);
      j = __shfl(e.y, 0, 64);
    } else {
      __syncthreads();                             // the slot may still be read from the pop before
      if (tid == 0) sh[4] = OsBest{0, e.x, e.y};
      __syncthreads();
      i = sh[4].v;
      j = sh[4].k;
    }
  }
  DEV OsBest best(int i, int j, int pi, int pj) {
    OsBest b = os_none();
    for (int k = i + 1 + tid; k < j; k += T) {
      const int pk = node_at(k);
      b = os_pick(b, OsBest{os_score(pi, pj, pk), os_vkey(pk, W), k});
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      OsBest c;
      c.score = __shfl_xor(b.score, o, 64);
      c.v = __shfl_xor(b.v, o, 64);
      c.k = __shfl_xor(b.k, o, 64);
      b = os_pick(b, c);
    }
    if (T == 256) {
      if ((tid & 63) == 0) sh[tid >> 6] = b;
      __syncthreads();
      b = os_pick(os_pick(sh[0], sh[1]), os_pick(sh[2], sh[3]));
      __syncthreads();                             // sh is written again by the next pop or reduction
    }
    return b;
  }
};

// arcs a0, a0 + stride, ... of the list; T == 64 takes those below OS_BLOCK_LEN edges, T == 256 the others
template <int T>
__global__ __launch_bounds__(256) void os_simplify_kernel(const int32_t* __restrict__ head, int cap, int NR, int W,
                                                          long long tol2_q4,
                                                          const int32_t* __restrict__ ringstart,
                                                          const int32_t* __restrict__ ring,
                                                          const int32_t* __restrict__ node,
                                                          const int32_t* __restrict__ arclen,
                                                          const int32_t* __restrict__ arcs, int32_t* keep,
                                                          int2* stack) {
  __shared__ OsBest sh[5];
  const int n = os_clamp(head[0], 0, cap), na = os_clamp(head[2], 0, n);
  const int groups = T == 64 ? 4 : 1;
  const int64_t stride = (int64_t)gridDim.x * groups;
  for (int64_t a = (int64_t)blockIdx.x * groups + (T == 64 ? (threadIdx.x >> 6) : 0); a < na; a += stride) {
    const int p = arcs[a];                         // uniform over the group from here on
    if (p < 0 || p >= n) continue;
    const int len = arclen[p];
    if (len < 2 || (len >= OS_BLOCK_LEN) != (T == 256)) continue;
    const int r = os_clamp(ring[p], 0, NR - 1);
    const int s = os_clamp(ringstart[r], 0, n), e = os_clamp(ringstart[r + 1], 0, n);
    if (!(s <= p && p < e) || len > e - s) continue;
    OsArc<T> arc{node, keep, stack, s, e - s, p - s, W, T == 64 ? (int)(threadIdx.x & 63) : (int)threadIdx.x, sh};
    os_douglas_peucker(arc, len, tol2_q4);
  }
}

__global__ __launch_bounds__(256) void os_copy_kernel(const int32_t* __restrict__ head, int cap,
                                                      const int32_t* __restrict__ keep, int32_t* __restrict__ kpos) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= cap) return;
  kpos[p] = (p < os_clamp(head[0], 0, cap) && keep[p] != 0) ? 1 : 0;
}

__global__ __launch_bounds__(256) void os_kept_kernel(const int32_t* __restrict__ head, int cap,
                                                      const int32_t* __restrict__ keep,
                                                      const int32_t* __restrict__ kpos,
                                                      const int32_t* __restrict__ node, int32_t* __restrict__ kxy) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= os_clamp(head[0], 0, cap) || keep[p] == 0) return;
  const int q = kpos[p];
  if (q >= 0 && q < cap) kxy[q] = node[p];
}

// ---------------------------------------------------------------------------------------------------- write
DEV int os_kept_before(const int32_t* head, const int32_t* kpos, int n, int p) {   // p in [0, n]
  return p < n ? kpos[p] : os_clamp(head[1], 0, n);
}

__global__ __launch_bounds__(256) void os_ring_kernel(const int32_t* __restrict__ head, int cap, int NR,
                                                      const int32_t* __restrict__ ringstart,
                                                      const int32_t* __restrict__ kpos,
                                                      const int32_t* __restrict__ value_in,
                                                      const long long* __restrict__ area2_in,
                                                      int32_t* __restrict__ ring_offset,
                                                      int32_t* __restrict__ ring_value,
                                                      long long* __restrict__ ring_area2,
                                                      uint8_t* __restrict__ ring_hole, int64_t ring_cap) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > NR || r > ring_cap) return;
  const int n = os_clamp(head[0], 0, cap);
  ring_offset[r] = os_kept_before(head, kpos, n, r == NR ? n : os_clamp(ringstart[r], 0, n));
  if (r == NR || r == ring_cap) return;
  ring_value[r] = value_in[r];
  ring_area2[r] = 0;
  ring_hole[r] = area2_in[r] < 0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void os_write_kernel(const int32_t* __restrict__ head, int cap, int NR,
                                                       const int32_t* __restrict__ ringstart,
                                                       const int32_t* __restrict__ ring,
                                                       const int32_t* __restrict__ keep,
                                                       const int32_t* __restrict__ kpos,
                                                       const int32_t* __restrict__ kxy, long long* ring_area2,
                                                       int64_t ring_cap, int2* __restrict__ vertices,
                                                       int64_t vertex_cap) {
  const int64_t p64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = os_clamp(head[0], 0, cap);
  if (p64 >= n || keep[p64] == 0) return;
  const int p = (int)p64;
  const int q = kpos[p];
  if (q < 0 || q >= n) return;
  const int r = os_clamp(ring[p], 0, NR - 1);
  const int a = os_kept_before(head, kpos, n, os_clamp(ringstart[r], 0, n));
  const int b = os_kept_before(head, kpos, n, os_clamp(ringstart[r + 1], 0, n));
  const int qn = os_clamp(q + 1 < b ? q + 1 : a, 0, n - 1);
  const int p0 = kxy[q], p1 = kxy[qn];
  if (q < vertex_cap) vertices[q] = make_int2(os_x(p0), os_y(p0));
  if (r < ring_cap)
    __hip_atomic_fetch_add((unsigned long long*)ring_area2 + r,
                           (unsigned long long)ro_area_term(os_x(p0), os_y(p0), os_x(p1), os_y(p1)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

unsigned os_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int64_t catseg_outline_simplify_workspace(int64_t H, int64_t W, int64_t corners, int64_t nodes) {
  if (!os_shape_ok(H, W) || corners < 1 || corners > 4 * (H + 1) * (W + 1)) return 0;
  if (nodes < 0) return os_shape(H, W, corners).bytes();
  // a corner contributes itself and fewer than max(H, W) junctions; each lattice vertex is a node of <= 4 rings
  if (nodes < corners || nodes > 4 * (H + 1) * (W + 1)) return 0;
  return os_nodes(corners, nodes).bytes();
}

#define OS_RINGS_CHECKS(name)                                                                               \
  CATSEG_CHECK(os_shape_ok(H, W), name ": need 1 <= H, W <= 16384 (the scores are exact int64 products)");  \
  CATSEG_CHECK(corners >= 1 && corners <= 4 * (H + 1) * (W + 1), name ": corners must be in 1 .. 4 (H + 1) (W + 1)"); \
  CATSEG_CHECK(rings >= 1 && rings <= corners, name ": rings must be in 1 .. corners");                     \
  const OsShape sh = os_shape(H, W, corners)

#define OS_INPUT_CHECKS(name)                                                                               \
  CATSEG_CHECK(ring_offset && vertices, name ": null pointer (ring_offset, vertices)");                     \
  CATSEG_CHECK(((uintptr_t)ring_offset % 4) == 0 && ((uintptr_t)vertices % 8) == 0,                         \
               name ": misaligned pointer (ring_offset 4 bytes, vertices 8 bytes)")

#define OS_MAP_WS_CHECKS(name)                                                                              \
  CATSEG_CHECK(workspace && ((uintptr_t)workspace % 16) == 0, name ": workspace null or not 16-byte aligned"); \
  CATSEG_CHECK(workspace_bytes >= sh.bytes(),                                                               \
               name ": workspace smaller than catseg_outline_simplify_workspace(H, W, corners, -1)")

#define OS_NODE_WS_CHECKS(name)                                                                             \
  CATSEG_CHECK(nodes >= corners && nodes <= 4 * (H + 1) * (W + 1),                                          \
               name ": nodes must be in corners .. 4 (H + 1) (W + 1)");                                     \
  CATSEG_CHECK(node_workspace && ((uintptr_t)node_workspace % 16) == 0,                                     \
               name ": node workspace null or not 16-byte aligned");                                        \
  const OsNodes ns = os_nodes(corners, nodes);                                                              \
  CATSEG_CHECK(node_workspace_bytes >= ns.bytes(),                                                          \
               name ": node workspace smaller than catseg_outline_simplify_workspace(H, W, corners, nodes)")

extern "C" int catseg_outline_simplify_count(const int32_t* ids, int64_t H, int64_t W, int64_t ld,
                                             const int32_t* ring_offset, int64_t rings, const int32_t* vertices,
                                             int64_t corners, void* workspace, int64_t workspace_bytes,
                                             void* stream) {
  CATSEG_CHECK(ids && ((uintptr_t)ids % 4) == 0, "outline_simplify_count: ids null or misaligned");
  OS_RINGS_CHECKS("outline_simplify_count");
  CATSEG_CHECK(ld >= W, "outline_simplify_count: the row stride ld must be >= W");
  OS_INPUT_CHECKS("outline_simplify_count");
  OS_MAP_WS_CHECKS("outline_simplify_count");
  int32_t* ws = (int32_t*)workspace;
  int32_t* cnt = ws + OS_HEAD;
  int32_t* bsum = cnt + sh.k4;
  unsigned long long* rowbits = (unsigned long long*)(bsum + sh.nb4);
  unsigned long long* colbits = rowbits + sh.nwords;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(colbits, 0, (size_t)(sh.vw * sh.col_words) * 8, st) != hipSuccess)
    return catseg_launch_status("outline_simplify_count");
  hipLaunchKernelGGL(os_junction_kernel, dim3((unsigned)((sh.nwords + 3) / 4)), dim3(256), 0, st, ids, (int)H, (int)W,
                     ld, (int)sh.row_words, (int)sh.col_words, (int)sh.nwords, rowbits, colbits);
  hipLaunchKernelGGL(os_count_kernel, dim3(os_grid(corners)), dim3(256), 0, st, ring_offset, (int)rings,
                     (const int2*)vertices, (int)corners, (int)H, (int)W, (int)sh.row_words, (int)sh.col_words,
                     rowbits, colbits, cnt);
  lr_scan_launch(cnt, corners, bsum, ws, st);
  return catseg_launch_status("outline_simplify_count");
}

extern "C" int catseg_outline_simplify_run(const int32_t* ring_offset, int64_t rings, const int32_t* vertices,
                                           int64_t corners, int64_t H, int64_t W, double tolerance,
                                           const void* workspace, int64_t workspace_bytes, int64_t nodes,
                                           void* node_workspace, int64_t node_workspace_bytes, void* stream) {
  OS_RINGS_CHECKS("outline_simplify_run");
  OS_INPUT_CHECKS("outline_simplify_run");
  CATSEG_CHECK(tolerance >= 0.0 && tolerance <= (double)OS_MAX_SIDE,
               "outline_simplify_run: the tolerance must be in 0 .. 16384 pixels");
  OS_MAP_WS_CHECKS("outline_simplify_run");
  OS_NODE_WS_CHECKS("outline_simplify_run");
  const int32_t* ws = (const int32_t*)workspace;
  const int32_t* off = ws + OS_HEAD;
  const unsigned long long* rowbits = (const unsigned long long*)(off + sh.k4 + sh.nb4);
  const unsigned long long* colbits = rowbits + sh.nwords;
  const OsNodePtrs np = os_node_ptrs(node_workspace, ns);
  hipStream_t st = (hipStream_t)stream;
  const int cap = (int)nodes, NR = (int)rings;
  const long long tol2_q4 = os_tol2_q4(tolerance);
  if (hipMemsetAsync(np.head, 0, (size_t)(OS_HEAD + ns.r4) * 4, st) != hipSuccess)
    return catseg_launch_status("outline_simplify_run");
  hipLaunchKernelGGL(os_node_kernel, dim3(os_grid(corners)), dim3(256), 0, st, ring_offset, NR,
                     (const int2*)vertices, (int)corners, (int)H, (int)W, (int)sh.row_words, (int)sh.col_words, ws,
                     off, rowbits, colbits, cap, np.head, np.ringstart, np.node, np.ring, np.keep);
  hipLaunchKernelGGL(os_anchor_kernel, dim3((unsigned)((ns.nw + 3) / 4)), dim3(256), 0, st, np.head, cap, (int)ns.nw,
                     np.keep, np.abits);
  hipLaunchKernelGGL(os_arc_kernel, dim3(os_grid(nodes)), dim3(256), 0, st, np.head, cap, NR, np.ringstart, np.ring,
                     np.abits, np.keep, np.arclen, np.aidx);
  lr_scan_launch(np.aidx, nodes, np.bsum, np.head + 2, st);
  hipLaunchKernelGGL(os_arc_list_kernel, dim3(os_grid(nodes)), dim3(256), 0, st, np.head, cap, np.arclen, np.aidx,
                     np.arcs);
  // both grids stride over the arc list: enough groups to fill the device, never more than there can be arcs
  const int64_t cus = std::max(1, catseg_device_cus());
  const unsigned wave_blocks = (unsigned)std::min<int64_t>(cus * 32, (nodes / 2 + 3) / 4 + 1);
  const unsigned big_blocks = (unsigned)std::min<int64_t>(cus * 4, nodes / OS_BLOCK_LEN + 1);
  hipLaunchKernelGGL(os_simplify_kernel<64>, dim3(wave_blocks), dim3(256), 0, st, np.head, cap, NR, (int)W, tol2_q4,
                     np.ringstart, np.ring, np.node, np.arclen, np.arcs, np.keep, np.stack);
  hipLaunchKernelGGL(os_simplify_kernel<256>, dim3(big_blocks), dim3(256), 0, st, np.head, cap, NR, (int)W, tol2_q4,
                     np.ringstart, np.ring, np.node, np.arclen, np.arcs, np.keep, np.stack);
  hipLaunchKernelGGL(os_copy_kernel, dim3(os_grid(nodes)), dim3(256), 0, st, np.head, cap, np.keep, np.kpos);
  lr_scan_launch(np.kpos, nodes, np.bsum, np.head + 1, st);
  hipLaunchKernelGGL(os_kept_kernel, dim3(os_grid(nodes)), dim3(256), 0, st, np.head, cap, np.keep, np.kpos, np.node,
                     np.kxy);
  return catseg_launch_status("outline_simplify_run");
}

extern "C" int catseg_outline_simplify_write(const void* node_workspace, int64_t node_workspace_bytes, int64_t H,
                                             int64_t W, int64_t corners, int64_t nodes, int64_t rings,
                                             const int32_t* ring_value_in, const int64_t* ring_area2_in,
                                             int32_t* ring_offset, int32_t* ring_value, int64_t* ring_area2,
                                             uint8_t* ring_hole, int64_t ring_capacity, int32_t* vertices,
                                             int64_t vertex_capacity, void* stream) {
  OS_RINGS_CHECKS("outline_simplify_write");
  OS_NODE_WS_CHECKS("outline_simplify_write");
  CATSEG_CHECK(ring_value_in && ring_area2_in && ((uintptr_t)ring_value_in % 4) == 0 &&
                   ((uintptr_t)ring_area2_in % 8) == 0,
               "outline_simplify_write: source ring columns null or misaligned");
  CATSEG_CHECK(ring_capacity >= 0 && vertex_capacity >= 0, "outline_simplify_write: negative capacity");
  CATSEG_CHECK(ring_offset && ((uintptr_t)ring_offset % 4) == 0,
               "outline_simplify_write: ring_offset (ring_capacity + 1 ints) null or misaligned");
  CATSEG_CHECK(ring_capacity == 0 || (ring_value && ring_area2 && ring_hole),
               "outline_simplify_write: null ring column");
  CATSEG_CHECK(((uintptr_t)ring_value % 4) == 0 && ((uintptr_t)ring_area2 % 8) == 0,
               "outline_simplify_write: misaligned ring column");
  CATSEG_CHECK(vertex_capacity == 0 || vertices, "outline_simplify_write: null vertices");
  CATSEG_CHECK(((uintptr_t)vertices % 8) == 0, "outline_simplify_write: vertices must be 8-byte aligned");
  const OsNodePtrs np = os_node_ptrs(const_cast<void*>(node_workspace), ns);
  hipStream_t st = (hipStream_t)stream;
  const int cap = (int)nodes, NR = (int)rings;
  hipLaunchKernelGGL(os_ring_kernel, dim3(os_grid(std::min(rings, ring_capacity) + 1)), dim3(256), 0, st, np.head, cap,
                     NR, np.ringstart, np.kpos, ring_value_in, (const long long*)ring_area2_in, ring_offset, ring_value,
                     (long long*)ring_area2, ring_hole, ring_capacity);
  hipLaunchKernelGGL(os_write_kernel, dim3(os_grid(nodes)), dim3(256), 0, st, np.head, cap, NR, np.ringstart, np.ring,
                     np.keep, np.kpos, np.kxy, (long long*)ring_area2, ring_capacity, (int2*)vertices, vertex_capacity);
  return catseg_launch_status("outline_simplify_write");
}
