// Region outlines: the boundaries of the regions of an int32 map traced into polygon rings, on the device.  No
// counterpart in the reference; the contract is DESIGN.md section 4 ("Region outlines"), the index logic
// region_outlines_logic.h, which a host program runs too.
//
// Count, scan, write, twice: once over the lattice vertices (how many corners, K) and once over the corners
// (how many rings, NR).  Two workspaces, as two sizes are only known on the device:
//   map workspace (a function of H, W), filled by catseg_region_outlines_count
//     count   one wave per word of 64 vertices of a lattice row: the corners of every vertex from its 2 x 2
//             pixels, one __ballot mask per incoming direction (the row bitmaps of E and W are these masks), the
//             word's corner count, and for S / N a bit in the column bitmaps by a 64-bit atomic OR (OR commutes;
//             the bitmaps are zeroed by a memset on the stream).
//     scan    scan_i32.h over the word counts; K at word 0.
//   ring workspace (a function of K), filled by catseg_region_outlines_rank
//     link    the same waves: every corner's number (word offset + popcounts), its key, and its successor: the
//             first corner along its outgoing ray with that incoming direction, found in the bitmaps a word at
//             a time, then numbered from the masks of the word it lies in.
//     jump    ceil(log2 K) launches of pointer jumping, double-buffered (a round reads one buffer and writes the
//             other: no waiting between workgroups).  One pass carries both the ring's smallest corner and the
//             distance to it (ro_jump), so start and rank come out of the same rounds.
//     final   rank, start flag and ring length per corner; two scans in key order: start flags -> ring number
//             (NR at word 1), lengths at the starts -> ring_offset (their sum at word 2).
//   catseg_region_outlines_write
//     every corner stores (x, y) at ring_offset[ring] + rank and adds its shoelace term to the ring's area2 by a
//     64-bit integer atomic (the same bits in any order); a ring's start stores its offset and value.
// Every number read from a workspace is bounded before it indexes anything, so a foreign or stale workspace
// yields wrong rings, never a store outside the caller's capacities or a load outside the buffers.
#include "common.h"
#include "capi.h"
#include "region_outlines_logic.h"
#include "scan_i32.h"

namespace {

constexpr int RO_HEAD = 4;                         // header ints of both workspaces; keeps the arrays 16-byte aligned

struct RoMap {                                     // pixel (y, x) of the (strided) map
  const int32_t* ids;
  int64_t ld;
  DEV int operator()(int y, int x) const { return ids[(int64_t)y * ld + x]; }
};

struct RoBits {                                    // the bitmaps of the map workspace
  const unsigned long long* mask4;                 // [word][4]
  const unsigned long long* colbits;               // [2][W + 1][col_words]: S, N
  int row_words, col_words, W;
  DEV unsigned long long row(int d, int y, int xw) const { return mask4[((int64_t)y * row_words + xw) * 4 + d]; }
  DEV unsigned long long col(int d, int x, int yw) const {
    return colbits[((int64_t)(d >> 1) * (W + 1) + x) * col_words + yw];
  }
};

struct RoShape {
  int64_t vw, vh, row_words, col_words, nwords, nw4, nb, nb4, colwords;
};

bool ro_shape_ok(int64_t H, int64_t W) {
  const int64_t lim = (int64_t)1 << 31;
  return H > 0 && W > 0 && H < lim && W < lim && H * W < lim && 4 * (H + 1) * (W + 1) < lim;
}

RoShape ro_shape(int64_t H, int64_t W) {           // ro_shape_ok(H, W)
  RoShape s;
  s.vw = W + 1;
  s.vh = H + 1;
  s.row_words = (s.vw + RO_WORD - 1) / RO_WORD;
  s.col_words = (s.vh + RO_WORD - 1) / RO_WORD;
  s.nwords = s.vh * s.row_words;
  s.nw4 = (s.nwords + 3) / 4 * 4;
  s.nb = (s.nwords + LR_SCAN - 1) / LR_SCAN;
  s.nb4 = (s.nb + 3) / 4 * 4;
  s.colwords = 2 * s.vw * s.col_words;
  return s;
}

// map workspace (ints): head | cnt nw4 | bsum nb4 | mask4 8 * nwords | colbits 2 * colwords
int64_t ro_map_bytes(const RoShape& s) {
  return (RO_HEAD + s.nw4 + s.nb4 + 8 * s.nwords + 2 * s.colwords) * (int64_t)sizeof(int32_t);
}

struct RoRing {
  int64_t k4, nb, nb4;
};
RoRing ro_ring(int64_t K) {
  RoRing r;
  r.k4 = (K + 3) / 4 * 4;
  r.nb = (K + LR_SCAN - 1) / LR_SCAN;
  r.nb4 = (r.nb + 3) / 4 * 4;
  return r;
}
// ring workspace (ints): head | key | succ | start | rank | ringno | ringoff (k4 each) | bsum nb4 | jump 2 x 4 * k4
int64_t ro_ring_bytes(const RoRing& r) { return (RO_HEAD + 14 * r.k4 + r.nb4) * (int64_t)sizeof(int32_t); }

// the vertex of this lane: a wave owns word gw of the lattice; code = ro_corners of the vertex (0 beyond the row)
DEV unsigned ro_lane_code(const RoMap& g, int H, int W, int conn8, int x, int y) {
  if (x > W) return 0u;
  int q[4];
  const unsigned have = ro_quad(g, x, y, H, W, q);
  return ro_corners(q, have, conn8 != 0);
}

__global__ __launch_bounds__(256) void ro_count_kernel(const int32_t* __restrict__ ids, int H, int W, int64_t ld,
                                                       int conn8, int row_words, int col_words, int nwords,
                                                       int32_t* __restrict__ cnt,
                                                       unsigned long long* __restrict__ mask4,
                                                       unsigned long long* colbits) {
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= nwords) return;                        // wave-uniform
  const int y = gw / row_words, xw = gw - y * row_words, x = xw * RO_WORD + lane;
  const unsigned code = ro_lane_code(RoMap{ids, ld}, H, W, conn8, x, y);
  unsigned long long m[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) m[d] = __ballot(ro_is_corner(code, d));
  if (lane == 0) cnt[gw] = ro_popc(m[0]) + ro_popc(m[1]) + ro_popc(m[2]) + ro_popc(m[3]);
  if (lane < 4) mask4[(int64_t)gw * 4 + lane] = lane == 0 ? m[0] : lane == 1 ? m[1] : lane == 2 ? m[2] : m[3];
  // x <= W here (code != 0), y <= H: inside [2][W + 1][col_words]
  if (ro_is_corner(code, 1))
    __hip_atomic_fetch_or(colbits + (int64_t)x * col_words + (y >> 6), 1ull << (y & 63), __ATOMIC_RELAXED,
                          __HIP_MEMORY_SCOPE_AGENT);
  if (ro_is_corner(code, 3))
    __hip_atomic_fetch_or(colbits + ((int64_t)(W + 1) + x) * col_words + (y >> 6), 1ull << (y & 63),
                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// key, successor and the first jump state of every corner below cap
__global__ __launch_bounds__(256) void ro_link_kernel(const int32_t* __restrict__ ids, int H, int W, int64_t ld,
                                                      int conn8, int row_words, int col_words, int nwords,
                                                      const int32_t* __restrict__ map_ws,
                                                      const int32_t* __restrict__ off,
                                                      const unsigned long long* __restrict__ mask4,
                                                      const unsigned long long* __restrict__ colbits, int cap,
                                                      int32_t* __restrict__ ring_ws, int32_t* __restrict__ key,
                                                      int32_t* __restrict__ succ, int4* __restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) ring_ws[0] = max(0, min(map_ws[0], cap));
  const int lane = threadIdx.x & 63;
  const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= nwords) return;                        // wave-uniform
  const int y = gw / row_words, xw = gw - y * row_words, x = xw * RO_WORD + lane;
  const unsigned code = ro_lane_code(RoMap{ids, ld}, H, W, conn8, x, y);
  unsigned long long m[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) m[d] = __ballot(ro_is_corner(code, d));
  if (!(code & 15u)) return;
  const int base = off[gw];
  const RoBits bits{mask4, colbits, row_words, col_words, W};
#pragma unroll 1
  for (int d = 0; d < 4; ++d) {
    if (!ro_is_corner(code, d)) continue;
    const int i = ro_corner_index(base, m, lane, d);
    if ((unsigned)i >= (unsigned)cap) continue;
    const int o = ro_out(code, d);
    const int c = ro_successor(bits, x, y, o, H, W);
    const int x1 = (o & 1) ? x : c, y1 = (o & 1) ? c : y;
    int j = i;                                     // no successor inside the lattice or below cap: a ring of its own
    if (c >= 0 && x1 <= W && y1 <= H) {
      const int64_t w1 = (int64_t)y1 * row_words + (x1 >> 6);
      unsigned long long m1[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) m1[e] = mask4[w1 * 4 + e];
      const int t = ro_corner_index(off[w1], m1, x1 & 63, o);
      if ((unsigned)t < (unsigned)cap) j = t;
    }
    key[i] = (y * (W + 1) + x) * 4 + d;
    succ[i] = j;
    state[i] = make_int4(j, i, 0, 0);
  }
}

DEV int ro_n(const int32_t* ring_ws, int cap) { return max(0, min(ring_ws[0], cap)); }

__global__ __launch_bounds__(256) void ro_jump_kernel(const int32_t* __restrict__ ring_ws, int cap, int round,
                                                      const int4* __restrict__ in, int4* __restrict__ out) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = ro_n(ring_ws, cap);
  if (i64 >= n) return;
  const int i = (int)i64;
  const int4 a = in[i];
  const int4 b = in[(unsigned)a.x < (unsigned)n ? a.x : i];
  const RoJump r = ro_jump(RoJump{a.x, a.y, a.z}, RoJump{b.x, b.y, b.z}, round);
  out[i] = make_int4(r.nxt, r.mn, r.off, 0);
}

// start, rank and the two scan inputs of every corner; corners in [n, cap) get zeros (the scans run over cap)
__global__ __launch_bounds__(256) void ro_final_kernel(const int32_t* __restrict__ ring_ws, int cap,
                                                       const int4* __restrict__ state,
                                                       const int32_t* __restrict__ succ, int32_t* __restrict__ start,
                                                       int32_t* __restrict__ rank, int32_t* __restrict__ ringno,
                                                       int32_t* __restrict__ ringoff) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i64 >= cap) return;
  const int i = (int)i64;
  const int n = ro_n(ring_ws, cap);
  int s = i, rk = 0, len = 0;
  if (i < n) {
    const int4 st = state[i];
    s = (unsigned)st.y < (unsigned)n ? st.y : i;
    const int after = succ[s];
    len = ro_ring_length((unsigned)after < (unsigned)n ? state[after].z : 0);
    rk = ro_rank(len, st.z);
  }
  const bool is_start = i < n && s == i;
  start[i] = s;
  rank[i] = rk;
  ringno[i] = is_start ? 1 : 0;
  ringoff[i] = is_start ? len : 0;
}

__global__ __launch_bounds__(256) void ro_area_init_kernel(const int32_t* __restrict__ ring_ws, int64_t ring_cap,
                                                           long long* __restrict__ area2) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ring_cap || i >= (int64_t)ring_ws[1]) return;
  area2[i] = 0;
}

__global__ __launch_bounds__(256) void ro_write_kernel(const int32_t* __restrict__ ids, int H, int W, int64_t ld,
                                                       const int32_t* __restrict__ ring_ws, int cap,
                                                       const int32_t* __restrict__ key,
                                                       const int32_t* __restrict__ succ,
                                                       const int32_t* __restrict__ start,
                                                       const int32_t* __restrict__ rank,
                                                       const int32_t* __restrict__ ringno,
                                                       const int32_t* __restrict__ ringoff,
                                                       int32_t* __restrict__ ring_offset,
                                                       int32_t* __restrict__ ring_value, long long* ring_area2,
                                                       int64_t ring_cap, int2* __restrict__ vertices,
                                                       int64_t vertex_cap) {
  const int64_t i64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = ro_n(ring_ws, cap);
  if (i64 == 0) {                                  // the closing entry of ring_offset
    const int nr = ring_ws[1];
    if (nr >= 0 && (int64_t)nr <= ring_cap) ring_offset[nr] = ring_ws[2];
  }
  if (i64 >= n) return;
  const int i = (int)i64;
  const int s = (unsigned)start[i] < (unsigned)n ? start[i] : i;
  const int ring = ringno[s], first = ringoff[s];
  const int nvert = (W + 1) * (H + 1);
  const unsigned k0 = (unsigned)key[i] >> 2, d0 = (unsigned)key[i] & 3u;
  const int j = (unsigned)succ[i] < (unsigned)n ? succ[i] : i;
  const unsigned k1 = (unsigned)key[j] >> 2;
  const int y0 = (int)(k0 / (unsigned)(W + 1)), x0 = (int)k0 - y0 * (W + 1);
  const int y1 = (int)(k1 / (unsigned)(W + 1)), x1 = (int)k1 - y1 * (W + 1);
  const bool ring_ok = ring >= 0 && (int64_t)ring < ring_cap;
  if (ring_ok)
    __hip_atomic_fetch_add((unsigned long long*)ring_area2 + ring, (unsigned long long)ro_area_term(x0, y0, x1, y1),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const int64_t pos = (int64_t)first + rank[i];
  if (first >= 0 && rank[i] >= 0 && pos < vertex_cap) vertices[pos] = make_int2(x0, y0);
  if (s == i) {
    if (ring >= 0 && (int64_t)ring <= ring_cap) ring_offset[ring] = first;
    if (ring_ok) {                                 // the value on the ring's right: pixel q[d_in] of the start vertex
      const int py = y0 - (d0 == 1 || d0 == 2 ? 1 : 0), px = x0 - (d0 == 0 || d0 == 1 ? 1 : 0);
      ring_value[ring] = ((int)k0 < nvert && px >= 0 && px < W && py >= 0 && py < H) ? ids[(int64_t)py * ld + px] : 0;
    }
  }
}

}  // namespace

extern "C" int64_t catseg_region_outlines_workspace(int64_t H, int64_t W, int64_t corners) {
  if (!ro_shape_ok(H, W)) return 0;
  if (corners < 0) return ro_map_bytes(ro_shape(H, W));
  if (corners > 4 * (H + 1) * (W + 1)) return 0;
  return ro_ring_bytes(ro_ring(corners));
}

#define RO_COMMON_CHECKS(name)                                                                              \
  CATSEG_CHECK(ids, name ": null pointer (ids)");                                                           \
  CATSEG_CHECK(H > 0 && W > 0, name ": H and W must be positive");                                          \
  CATSEG_CHECK(ro_shape_ok(H, W), name ": need H * W < 2^31 and 4 (H + 1) (W + 1) < 2^31 (corner keys are int32)"); \
  CATSEG_CHECK(ld >= W, name ": the row stride ld must be >= W");                                           \
  CATSEG_CHECK(((uintptr_t)ids % 4) == 0, name ": misaligned pointer (ids 4 bytes)");                       \
  const RoShape sh = ro_shape(H, W)

#define RO_MAP_WS_CHECKS(name)                                                                              \
  CATSEG_CHECK(workspace && ((uintptr_t)workspace % 16) == 0, name ": workspace null or not 16-byte aligned"); \
  CATSEG_CHECK(workspace_bytes >= ro_map_bytes(sh),                                                         \
               name ": workspace smaller than catseg_region_outlines_workspace(H, W, -1)")

#define RO_RING_WS_CHECKS(name)                                                                             \
  CATSEG_CHECK(corners >= 1 && corners <= 4 * sh.vh * sh.vw, name ": corners must be in 1 .. 4 (H + 1) (W + 1)"); \
  CATSEG_CHECK(ring_workspace && ((uintptr_t)ring_workspace % 16) == 0,                                     \
               name ": ring workspace null or not 16-byte aligned");                                        \
  const RoRing rg = ro_ring(corners);                                                                       \
  CATSEG_CHECK(ring_workspace_bytes >= ro_ring_bytes(rg),                                                   \
               name ": ring workspace smaller than catseg_region_outlines_workspace(H, W, corners)")

extern "C" int catseg_region_outlines_count(const int32_t* ids, int64_t H, int64_t W, int64_t ld, int connectivity,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
  RO_COMMON_CHECKS("region_outlines_count");
  RO_MAP_WS_CHECKS("region_outlines_count");
  CATSEG_CHECK(connectivity == 4 || connectivity == 8, "region_outlines_count: connectivity must be 4 or 8");
  int32_t* ws = (int32_t*)workspace;
  int32_t* cnt = ws + RO_HEAD;
  int32_t* bsum = cnt + sh.nw4;
  unsigned long long* mask4 = (unsigned long long*)(bsum + sh.nb4);
  unsigned long long* colbits = mask4 + 4 * sh.nwords;
  hipStream_t st = (hipStream_t)stream;
  if (hipMemsetAsync(colbits, 0, (size_t)sh.colwords * 8, st) != hipSuccess)
    return catseg_launch_status("region_outlines_count");
  hipLaunchKernelGGL(ro_count_kernel, dim3((unsigned)((sh.nwords + 3) / 4)), dim3(256), 0, st, ids, (int)H, (int)W, ld,
                     connectivity == 8, (int)sh.row_words, (int)sh.col_words, (int)sh.nwords, cnt, mask4, colbits);
  lr_scan_launch(cnt, sh.nwords, bsum, ws, st);
  return catseg_launch_status("region_outlines_count");
}

extern "C" int catseg_region_outlines_rank(const int32_t* ids, int64_t H, int64_t W, int64_t ld, int connectivity,
                                           const void* workspace, int64_t workspace_bytes, int64_t corners,
                                           void* ring_workspace, int64_t ring_workspace_bytes, void* stream) {
  RO_COMMON_CHECKS("region_outlines_rank");
  RO_MAP_WS_CHECKS("region_outlines_rank");
  CATSEG_CHECK(connectivity == 4 || connectivity == 8, "region_outlines_rank: connectivity must be 4 or 8");
  RO_RING_WS_CHECKS("region_outlines_rank");
  const int32_t* ws = (const int32_t*)workspace;
  const int32_t* off = ws + RO_HEAD;
  const unsigned long long* mask4 = (const unsigned long long*)(off + sh.nw4 + sh.nb4);
  const unsigned long long* colbits = mask4 + 4 * sh.nwords;
  int32_t* rws = (int32_t*)ring_workspace;
  int32_t* key = rws + RO_HEAD;
  int32_t* succ = key + rg.k4;
  int32_t* start = succ + rg.k4;
  int32_t* rank = start + rg.k4;
  int32_t* ringno = rank + rg.k4;
  int32_t* ringoff = ringno + rg.k4;
  int32_t* bsum = ringoff + rg.k4;
  int4* state[2] = {(int4*)(bsum + rg.nb4), (int4*)(bsum + rg.nb4) + rg.k4};
  hipStream_t st = (hipStream_t)stream;
  const int cap = (int)corners;
  hipLaunchKernelGGL(ro_link_kernel, dim3((unsigned)((sh.nwords + 3) / 4)), dim3(256), 0, st, ids, (int)H, (int)W, ld,
                     connectivity == 8, (int)sh.row_words, (int)sh.col_words, (int)sh.nwords, ws, off, mask4, colbits,
                     cap, rws, key, succ, state[0]);
  const unsigned blocks = (unsigned)((corners + 255) / 256);
  const int rounds = ro_rounds(corners);
  for (int r = 0; r < rounds; ++r)
    hipLaunchKernelGGL(ro_jump_kernel, dim3(blocks), dim3(256), 0, st, rws, cap, r, state[r & 1], state[(r + 1) & 1]);
  hipLaunchKernelGGL(ro_final_kernel, dim3(blocks), dim3(256), 0, st, rws, cap, state[rounds & 1], succ, start, rank,
                     ringno, ringoff);
  lr_scan_launch(ringno, corners, bsum, rws + 1, st);
  lr_scan_launch(ringoff, corners, bsum, rws + 2, st);
  return catseg_launch_status("region_outlines_rank");
}

extern "C" int catseg_region_outlines_write(const int32_t* ids, int64_t H, int64_t W, int64_t ld,
                                            const void* ring_workspace, int64_t ring_workspace_bytes, int64_t corners,
                                            int32_t* ring_offset, int32_t* ring_value, int64_t* ring_area2,
                                            int64_t ring_capacity, int32_t* vertices, int64_t vertex_capacity,
                                            void* stream) {
  RO_COMMON_CHECKS("region_outlines_write");
  RO_RING_WS_CHECKS("region_outlines_write");
  CATSEG_CHECK(ring_capacity >= 0 && vertex_capacity >= 0, "region_outlines_write: negative capacity");
  CATSEG_CHECK(ring_offset && ((uintptr_t)ring_offset % 4) == 0,
               "region_outlines_write: ring_offset (ring_capacity + 1 ints) null or misaligned");
  CATSEG_CHECK(ring_capacity == 0 || (ring_value && ring_area2), "region_outlines_write: null ring column");
  CATSEG_CHECK(((uintptr_t)ring_value % 4) == 0 && ((uintptr_t)ring_area2 % 8) == 0,
               "region_outlines_write: misaligned ring column");
  CATSEG_CHECK(vertex_capacity == 0 || vertices, "region_outlines_write: null vertices");
  CATSEG_CHECK(((uintptr_t)vertices % 8) == 0, "region_outlines_write: vertices must be 8-byte aligned");
  const int32_t* rws = (const int32_t*)ring_workspace;
  const int32_t* key = rws + RO_HEAD;
  const int32_t* succ = key + rg.k4;
  const int32_t* start = succ + rg.k4;
  const int32_t* rank = start + rg.k4;
  const int32_t* ringno = rank + rg.k4;
  const int32_t* ringoff = ringno + rg.k4;
  hipStream_t st = (hipStream_t)stream;
  // at most `corners` rings exist: the grid of the init pass never exceeds the write pass's
  const int64_t rows = std::min(ring_capacity, corners);
  if (rows > 0)
    hipLaunchKernelGGL(ro_area_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, rws, ring_capacity,
                       (long long*)ring_area2);
  hipLaunchKernelGGL(ro_write_kernel, dim3((unsigned)((corners + 255) / 256)), dim3(256), 0, st, ids, (int)H, (int)W, ld,
                     rws, (int)corners, key, succ, start, rank, ringno, ringoff, ring_offset, ring_value,
                     (long long*)ring_area2, ring_capacity, (int2*)vertices, vertex_capacity);
  return catseg_launch_status("region_outlines_write");
}
