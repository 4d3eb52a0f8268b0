// Connected regions of an int32 label map, their table, and the small-region sieve, on the device.  No
// counterpart in the reference; the contract is DESIGN.md section 4 ("Connected regions and the sieve").
//
//   fold(l) = (clamp_pred >= 0 && l >= clamp_pred) ? clamp_pred : l          (label_runs.hip's fold)
//   a region is a maximal set of pixels of equal folded label connected under 4- or 8-connectivity;
//   regions are numbered in row-major order of their first pixel p = y * W + x (the region's minimum p).
//
// Labelling is union-find with min-index roots over a global parent array of H * W ints (workspace),
// in three launches; the index / union / key logic is label_regions_logic.h, which a host program runs too:
//   tile     one workgroup per 64 x 64 tile: labels into LDS, a parent array in LDS that starts at every
//            pixel's horizontal run start (one __ballot per row), the runs of neighbouring rows joined by
//            LDS atomics (one join per pair of touching runs, with path splitting), then every pixel's tile
//            root, as a global index, stored to parent.  Plain stores: nothing else reads parent in this launch.
//   border   one thread per pixel on the low side of a tile border: joins across the border.  Roots written
//            by other workgroups IN THIS LAUNCH are chased, so every access to parent is an agent-scope
//            relaxed atomic (sc1 loads that bypass the per-CU L1, fetch_min at the L2 / memory): the per-XCD
//            L2s are not coherent and a plain load may return a line cached before another workgroup's
//            union.  Any value so read is a former or current ancestor (<= the index), which is all that
//            cc_find / cc_union need; nothing waits for another workgroup.
//   flatten  every pixel's root, stored back (agent-scope, as pixels of other workgroups are read while
//            they are rewritten: old value or root, both ancestors).  The same pass makes what the consumer
//            needs: the root flags of every 64 pixels (count + 64-bit mask, for the compaction), or the
//            area at each root (for the sieve).
// The launch count depends on (H, W) only (the border launch is absent for a single tile); no flag, no
// spinning, no readback.  Ids, table and sieved map are functions of the input: roots are minima, numbers come
// from a scan in index order, and the table and keys are integer atomics (add / min / max commute).
//
// Compaction: scan_i32.h over the per-64-pixel root counts; R at workspace word 0.  The write pass gives
// every pixel seg_off[root / 64] + popcount(mask[root / 64] below root) and accumulates the table rows
// (area, bbox, the Q16 score sum) with one atomic per (wave, row of 64 pixels, region) for the first regions
// of a row (12) and one per pixel beyond; a root writes its row's label and first pixel itself.
//
// Sieve: areas at the root index (flatten), one pass over the forward neighbour pairs of differing roots
// posts (area << 32 | ~root) of the large side to the small side's key by a 64-bit atomic max, one pass
// writes the labels.  No value crosses to the host.
#include "common.h"
#include "capi.h"
#include "label_regions_logic.h"
#include "scan_i32.h"

namespace {

constexpr int CC_HEAD = 4;                         // workspace header (ints): [0] = R; keeps the arrays 16-byte aligned
constexpr int CC_WRITE_ROWS = 16;                  // rows of a workgroup of the write pass (4 per wave)
constexpr int CC_GROUPS = 12;                      // regions of a 64-pixel row reduced in the wave before per-pixel atomics

struct LdsMem {                                    // the tile's parent array: workgroup scope is the LDS's own
  int* p;
  DEV int load(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  DEV int fetch_min(int i, int v) {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
};
struct AgentMem {                                  // the global parent array while other workgroups write it
  int* p;
  DEV int load(int i) { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
  DEV int fetch_min(int i, int v) {
    return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
struct AgentKeys {
  unsigned long long* k;
  DEV void fetch_max(int i, unsigned long long v) {
    __hip_atomic_fetch_max(k + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};
struct LdsLabels {
  const int* t;
  DEV int operator()(int i) const { return t[i]; }
};
struct MapLabels {                                 // folded label of pixel (y, x) of the (strided) map
  const int32_t* labels;
  int64_t ld;
  int clamp;
  DEV int operator()(int y, int x) const { return cc_fold(labels[(int64_t)y * ld + x], clamp); }
};

// tile-local union-find; parent[p] = the tile root of p as a global index
__global__ __launch_bounds__(256) void cc_tile_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t ld,
                                                      int clamp, int conn8, int tiles_x, int32_t* __restrict__ parent) {
  __shared__ int lab[CC_TILE * CC_TILE];
  __shared__ int par[CC_TILE * CC_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y0 = ty * CC_TILE, x0 = tx * CC_TILE;
  const int th = min(CC_TILE, H - y0), tw = min(CC_TILE, W - x0);
  // positions beyond the map are clamped into it: their LDS values are never compared (every step below
  // tests ly < th, lx < tw), so the loads are unconditional
  const int xs = min(x0 + lane, W - 1);
  // a wave owns whole tile rows, one lane per column: the run starts of a row are one __ballot mask
#pragma unroll 4
  for (int i = 0; i < CC_TILE / 4; ++i) {
    const int ly = wv + 4 * i;
    const int y = min(y0 + ly, H - 1);
    const int v = cc_fold(labels[(int64_t)y * ld + xs], clamp);
    const int prev = __shfl_up(v, 1, 64);
    const unsigned long long starts = __ballot(lane == 0 || lane >= tw || v != prev);
    lab[ly * CC_TILE + lane] = v;
    par[ly * CC_TILE + lane] = ly * CC_TILE + cc_run_start(starts, lane);
  }
  __syncthreads();
  LdsMem m{par};
  const LdsLabels L{lab};
  if (lane < tw) {
    for (int i = 0; i < CC_TILE / 4; ++i) {
      const int ly = wv + 4 * i;
      if (ly < th) cc_tile_pixel(m, L, ly, lane, tw, conn8 != 0);
    }
  }
  __syncthreads();
  if (lane < tw) {
    for (int i = 0; i < CC_TILE / 4; ++i) {
      const int ly = wv + 4 * i;
      if (ly < th) cc_tile_settle(m, L, ly, lane);
    }
  }
  __syncthreads();
  if (lane < tw) {
    for (int i = 0; i < CC_TILE / 4; ++i) {
      const int ly = wv + 4 * i;
      if (ly < th) {
        const int r = cc_find(m, ly * CC_TILE + lane);
        parent[(y0 + ly) * W + x0 + lane] = (y0 + (r >> 6)) * W + x0 + (r & 63);     // < H * W < 2^31
      }
    }
  }
}

// joins across the tile borders: thread t < nv takes pixel (t % H, 64 * (t / H + 1)) of a vertical border,
// the others pixel (64 * ((t - nv) / W + 1), (t - nv) % W) of a horizontal one
__global__ __launch_bounds__(256) void cc_border_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t ld,
                                                        int clamp, int conn8, int64_t nv, int64_t total,
                                                        int32_t* parent) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  AgentMem m{parent};
  const MapLabels G{labels, ld, clamp};
  if (t < nv) {
    const int b = (int)(t / H), y = (int)(t - (int64_t)b * H);
    cc_border_vertical(m, G, y, (b + 1) * CC_TILE, H, W, conn8 != 0);
  } else {
    const int64_t u = t - nv;
    const int b = (int)(u / W), x = (int)(u - (int64_t)b * W);
    cc_border_horizontal(m, G, (b + 1) * CC_TILE, x, H, W, conn8 != 0);
  }
}

// adds n to area[key] for the active lanes, one atomic per distinct key for the first CC_GROUPS keys of the wave
DEV void cc_wave_count(bool active, int key, int32_t* area) {
  const int lane = threadIdx.x & 63;
  bool todo = active;
#pragma unroll 1
  for (int it = 0; it < CC_GROUPS; ++it) {
    const unsigned long long left = __ballot(todo);
    if (!left) break;                              // wave-uniform
    const int leader = __builtin_ctzll(left);
    const int k = __shfl(key, leader, 64);
    const bool mine = todo && key == k;
    const unsigned long long mm = __ballot(mine);
    if (lane == leader) __hip_atomic_fetch_add(area + k, __popcll(mm), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    todo = todo && !mine;
  }
  if (todo) __hip_atomic_fetch_add(area + key, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// every pixel to its root.  AREA = false: the root flags of the wave's 64 pixels (seg = their count,
// mask = the flags); AREA = true: area[root] += 1 (area zeroed before the launch)
template <bool AREA>
__global__ __launch_bounds__(256) void cc_flatten_kernel(int32_t* parent, int64_t n, int32_t* __restrict__ seg,
                                                         unsigned long long* __restrict__ mask,
                                                         int32_t* __restrict__ area) {
  const int64_t p64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool in = p64 < n;
  const int p = in ? (int)p64 : 0;
  AgentMem m{parent};
  int r = p;
  if (in) {
    r = cc_find(m, p);
    __hip_atomic_store(parent + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (AREA) {
    cc_wave_count(in, r, area);
  } else {
    const unsigned long long f = __ballot(in && r == p);
    if ((threadIdx.x & 63) == 0 && in) {
      seg[p >> 6] = __popcll(f);
      mask[p >> 6] = f;
    }
  }
}

// rows [0, min(R, capacity)) of the accumulated table columns to the identities of their atomics
__global__ __launch_bounds__(256) void cc_table_init_kernel(const int32_t* __restrict__ head, int64_t capacity,
                                                            int32_t* __restrict__ area, int32_t* __restrict__ bbox,
                                                            long long* __restrict__ score_q16) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= capacity || i >= (int64_t)head[0]) return;
  area[i] = 0;
  bbox[4 * i + 0] = 0x7fffffff;
  bbox[4 * i + 1] = 0x7fffffff;
  bbox[4 * i + 2] = 0;
  bbox[4 * i + 3] = 0;
  if (score_q16) score_q16[i] = 0;
}

DEV long long cc_shfl_xor64(long long v, int o) {
  const int lo = __shfl_xor((int)(unsigned)(unsigned long long)v, o, 64);
  const int hi = __shfl_xor((int)((unsigned long long)v >> 32), o, 64);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

DEV void cc_row_atomics(int id, int n, int xa, int xb, int y, bool has_score, long long q, int32_t* area,
                        int32_t* bbox, long long* score_q16) {
  __hip_atomic_fetch_add(area + id, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_min(bbox + 4 * (int64_t)id + 0, xa, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_min(bbox + 4 * (int64_t)id + 1, y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(bbox + 4 * (int64_t)id + 2, xb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_fetch_max(bbox + 4 * (int64_t)id + 3, y + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (has_score) __hip_atomic_fetch_add(score_q16 + id, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// region ids and the table: a workgroup owns 64 columns x CC_WRITE_ROWS rows, a wave whole rows of 64 pixels
__global__ __launch_bounds__(256) void cc_write_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t ld,
                                                       int clamp, const float* __restrict__ score, int64_t ld_score,
                                                       const int32_t* __restrict__ parent,
                                                       const int32_t* __restrict__ seg,
                                                       const unsigned long long* __restrict__ mask,
                                                       int32_t* __restrict__ region_ids, int64_t ld_ids,
                                                       int32_t* __restrict__ t_label, int32_t* __restrict__ t_area,
                                                       int32_t* __restrict__ t_bbox, int32_t* __restrict__ t_first,
                                                       long long* __restrict__ t_score, int64_t capacity,
                                                       int tiles_x) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
  const int x0 = bx * CC_TILE, x = x0 + lane;
  const bool has_score = score != nullptr;
#pragma unroll 1
  for (int i = 0; i < CC_WRITE_ROWS / 4; ++i) {
    const int y = by * CC_WRITE_ROWS + wv + 4 * i;
    if (y >= H) break;                             // wave-uniform
    const bool in = x < W;
    int id = 0;
    long long q = 0;
    bool todo = false;
    if (in) {
      const int p = y * W + x;
      int root = parent[p];
      if ((unsigned)root >= (unsigned)(H * W)) root = p;      // a foreign workspace indexes nothing outside seg / mask
      id = cc_region_id(seg[root >> 6], mask[root >> 6], root);
      region_ids[(int64_t)y * ld_ids + x] = id;
      todo = (int64_t)id < capacity;               // nothing is stored at a row >= capacity
      if (todo && root == p) {
        t_label[id] = cc_fold(labels[(int64_t)y * ld + x], clamp);
        t_first[id] = p;
      }
      if (has_score && todo) q = cc_score_q16(score[(int64_t)y * ld_score + x]);
    }
#pragma unroll 1
    for (int it = 0; it < CC_GROUPS; ++it) {
      const unsigned long long left = __ballot(todo);
      if (!left) break;                            // wave-uniform
      const int leader = __builtin_ctzll(left);
      const int k = __shfl(id, leader, 64);
      const bool mine = todo && id == k;
      const unsigned long long mm = __ballot(mine);
      long long s = mine ? q : 0;
      if (has_score && (mm & (mm - 1)) != 0) {       // more than one pixel (wave-uniform): sum over the wave
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += cc_shfl_xor64(s, o);
      }
      if (lane == leader)
        cc_row_atomics(k, __popcll(mm), x0 + __builtin_ctzll(mm), x0 + 64 - __builtin_clzll(mm), y, has_score, s,
                       t_area, t_bbox, t_score);
      todo = todo && !mine;
    }
    if (todo) cc_row_atomics(id, 1, x, x + 1, y, has_score, q, t_area, t_bbox, t_score);
  }
}

// forward neighbour pairs of differing roots: the large side's key to the small side
__global__ __launch_bounds__(256) void cc_sieve_pairs_kernel(const int32_t* __restrict__ parent,
                                                             const int32_t* __restrict__ area, int H, int W, int conn8,
                                                             int min_area, unsigned long long* keys) {
  const int64_t p64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p64 >= (int64_t)H * W) return;
  const int p = (int)p64;
  const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
  const int rp = parent[p];
  const int ap = area[rp];
  AgentKeys K{keys};
  const bool down = y + 1 < H;
  if (x + 1 < W) {
    const int rq = parent[p + 1];
    if (rq != rp) cc_sieve_pair(K, rp, ap, rq, area[rq], min_area);
  }
  if (down) {
    const int rq = parent[p + W];
    if (rq != rp) cc_sieve_pair(K, rp, ap, rq, area[rq], min_area);
    if (conn8) {
      if (x > 0) {
        const int rd = parent[p + W - 1];
        if (rd != rp) cc_sieve_pair(K, rp, ap, rd, area[rd], min_area);
      }
      if (x + 1 < W) {
        const int rd = parent[p + W + 1];
        if (rd != rp) cc_sieve_pair(K, rp, ap, rd, area[rd], min_area);
      }
    }
  }
}

// a pixel of a small region with a large neighbour takes that region's folded label; every other pixel
// keeps its value
__global__ __launch_bounds__(256) void cc_sieve_out_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t ld,
                                                           int clamp, const int32_t* __restrict__ parent,
                                                           const int32_t* __restrict__ area,
                                                           const unsigned long long* __restrict__ keys, int min_area,
                                                           int32_t* __restrict__ out, int64_t ld_out) {
  const int64_t p64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p64 >= (int64_t)H * W) return;
  const int p = (int)p64;
  const int y = (int)((unsigned)p / (unsigned)W), x = p - y * W;
  const int r = parent[p];
  const int src = cc_sieve_source(r, area[r], keys[r], min_area);
  int v = labels[(int64_t)y * ld + x];
  if (src != r && (unsigned)src < (unsigned)(H * W)) {   // the bound: a key of a foreign workspace reads nothing outside the map
    const int ys = (int)((unsigned)src / (unsigned)W), xs = src - ys * W;
    v = cc_fold(labels[(int64_t)ys * ld + xs], clamp);
  }
  out[(int64_t)y * ld_out + x] = v;
}

struct CcShape {
  int64_t n, n4, nseg, nseg4, nb, tiles_x, tiles_y, nv, nh;
};

bool cc_shape_ok(int64_t H, int64_t W) {
  return H > 0 && W > 0 && H < ((int64_t)1 << 31) && W < ((int64_t)1 << 31) && H * W < ((int64_t)1 << 31);
}

// H, W > 0 and H * W < 2^31 (checked by the callers)
CcShape cc_shape(int64_t H, int64_t W) {
  CcShape s;
  s.n = H * W;
  s.n4 = (s.n + 3) / 4 * 4;
  s.nseg = (s.n + 63) / 64;
  s.nseg4 = (s.nseg + 3) / 4 * 4;
  s.nb = (s.nseg + LR_SCAN - 1) / LR_SCAN;
  s.tiles_x = (W + CC_TILE - 1) / CC_TILE;
  s.tiles_y = (H + CC_TILE - 1) / CC_TILE;
  s.nv = (s.tiles_x - 1) * H;
  s.nh = (s.tiles_y - 1) * W;
  return s;
}

// count layout (ints): head | parent n4 | seg nseg4 | mask 2 * nseg4 | bsum nb
// sieve layout (ints): head | parent n4 | area n4 | keys 2 * n4
int64_t cc_workspace_bytes(const CcShape& s, bool sieve) {
  const int64_t ints = sieve ? CC_HEAD + 4 * s.n4 : CC_HEAD + s.n4 + 3 * s.nseg4 + s.nb;
  return ints * (int64_t)sizeof(int32_t);
}

// the three labelling launches; parent = workspace + CC_HEAD
template <bool AREA>
void cc_label_launch(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp, int connectivity,
                     const CcShape& s, int32_t* parent, int32_t* seg, unsigned long long* mask, int32_t* area,
                     hipStream_t st) {
  const int conn8 = connectivity == 8;
  hipLaunchKernelGGL(cc_tile_kernel, dim3((unsigned)(s.tiles_x * s.tiles_y)), dim3(256), 0, st, labels, (int)H, (int)W,
                     ld, clamp, conn8, (int)s.tiles_x, parent);
  const int64_t total = s.nv + s.nh;
  if (total > 0)
    hipLaunchKernelGGL(cc_border_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, labels, (int)H, (int)W,
                       ld, clamp, conn8, s.nv, total, parent);
  hipLaunchKernelGGL(cc_flatten_kernel<AREA>, dim3((unsigned)((s.n + 255) / 256)), dim3(256), 0, st, parent, s.n, seg,
                     mask, area);
}

}  // namespace

extern "C" int64_t catseg_label_regions_workspace(int64_t H, int64_t W, int sieve) {
  return cc_shape_ok(H, W) ? cc_workspace_bytes(cc_shape(H, W), sieve != 0) : 0;
}

#define CC_COMMON_CHECKS(name, sieve)                                                                       \
  CATSEG_CHECK(labels && workspace, name ": null pointer (labels, workspace)");                             \
  CATSEG_CHECK(H > 0 && W > 0, name ": H and W must be positive");                                          \
  CATSEG_CHECK(cc_shape_ok(H, W), name ": need H * W < 2^31 (pixel indices are int32)");                    \
  CATSEG_CHECK(ld >= W, name ": the row stride ld must be >= W");                                           \
  CATSEG_CHECK(((uintptr_t)labels % 4) == 0 && ((uintptr_t)workspace % 16) == 0,                            \
               name ": misaligned pointer (labels 4 bytes, workspace 16 bytes)");                           \
  const CcShape sh = cc_shape(H, W);                                                                        \
  CATSEG_CHECK(workspace_bytes >= cc_workspace_bytes(sh, sieve),                                            \
               name ": workspace smaller than catseg_label_regions_workspace(H, W, sieve)")

extern "C" int catseg_label_regions_count(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                          int connectivity, void* workspace, int64_t workspace_bytes, void* stream) {
  CC_COMMON_CHECKS("label_regions_count", false);
  CATSEG_CHECK(connectivity == 4 || connectivity == 8, "label_regions_count: connectivity must be 4 or 8");
  int32_t* ws = (int32_t*)workspace;
  int32_t* parent = ws + CC_HEAD;
  int32_t* seg = parent + sh.n4;
  unsigned long long* mask = (unsigned long long*)(seg + sh.nseg4);
  int32_t* bsum = seg + 3 * sh.nseg4;
  hipStream_t st = (hipStream_t)stream;
  cc_label_launch<false>(labels, H, W, ld, clamp_pred, connectivity, sh, parent, seg, mask, nullptr, st);
  lr_scan_launch(seg, sh.nseg, bsum, ws, st);
  return catseg_launch_status("label_regions_count");
}

extern "C" int catseg_label_regions_write(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                          const float* score, int64_t ld_score, const void* workspace,
                                          int64_t workspace_bytes, int32_t* region_ids, int64_t ld_ids,
                                          int32_t* label, int32_t* area, int32_t* bbox, int32_t* first,
                                          int64_t* score_q16, int64_t capacity, void* stream) {
  CC_COMMON_CHECKS("label_regions_write", false);
  CATSEG_CHECK(region_ids && ((uintptr_t)region_ids % 4) == 0, "label_regions_write: region_ids null or misaligned");
  CATSEG_CHECK(ld_ids >= W, "label_regions_write: the row stride ld_ids must be >= W");
  CATSEG_CHECK(capacity >= 0, "label_regions_write: negative capacity");
  CATSEG_CHECK(capacity == 0 || (label && area && bbox && first), "label_regions_write: null table pointer");
  CATSEG_CHECK(((uintptr_t)label % 4) == 0 && ((uintptr_t)area % 4) == 0 && ((uintptr_t)bbox % 4) == 0 &&
                   ((uintptr_t)first % 4) == 0 && ((uintptr_t)score_q16 % 8) == 0,
               "label_regions_write: misaligned table pointer");
  CATSEG_CHECK((score == nullptr) == (score_q16 == nullptr) || capacity == 0,
               "label_regions_write: score and score_q16 go together");
  CATSEG_CHECK(!score || (((uintptr_t)score % 4) == 0 && ld_score >= W),
               "label_regions_write: score misaligned or its row stride < W");
  const int32_t* ws = (const int32_t*)workspace;
  const int32_t* parent = ws + CC_HEAD;
  const int32_t* seg = parent + sh.n4;
  const unsigned long long* mask = (const unsigned long long*)(seg + sh.nseg4);
  hipStream_t st = (hipStream_t)stream;
  // at most H * W rows exist: the grid of the init pass never exceeds the map's
  const int64_t rows = std::min(capacity, sh.n);
  if (rows > 0)
    hipLaunchKernelGGL(cc_table_init_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, ws, capacity, area,
                       bbox, (long long*)score_q16);
  const int64_t gy = (H + CC_WRITE_ROWS - 1) / CC_WRITE_ROWS;
  CATSEG_CHECK(sh.tiles_x * gy < ((int64_t)1 << 31), "label_regions_write: grid out of range");
  hipLaunchKernelGGL(cc_write_kernel, dim3((unsigned)(sh.tiles_x * gy)), dim3(256), 0, st, labels, (int)H, (int)W,
                     ld, clamp_pred, capacity > 0 ? score : nullptr, ld_score, parent, seg, mask, region_ids, ld_ids,
                     label, area, bbox, first, (long long*)score_q16, capacity, (int)sh.tiles_x);
  return catseg_launch_status("label_regions_write");
}

extern "C" int catseg_sieve_labels(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                   int connectivity, int64_t min_area, int32_t* out, int64_t ld_out, void* workspace,
                                   int64_t workspace_bytes, void* stream) {
  CC_COMMON_CHECKS("sieve_labels", true);
  CATSEG_CHECK(connectivity == 4 || connectivity == 8, "sieve_labels: connectivity must be 4 or 8");
  CATSEG_CHECK(min_area >= 1, "sieve_labels: min_area must be >= 1");
  CATSEG_CHECK(out && ((uintptr_t)out % 4) == 0, "sieve_labels: out null or misaligned");
  CATSEG_CHECK(ld_out >= W, "sieve_labels: the row stride ld_out must be >= W");
  {
    const uintptr_t a0 = (uintptr_t)labels, a1 = a0 + (uintptr_t)(((H - 1) * ld + W) * 4);
    const uintptr_t b0 = (uintptr_t)out, b1 = b0 + (uintptr_t)(((H - 1) * ld_out + W) * 4);
    CATSEG_CHECK(a1 <= b0 || b1 <= a0, "sieve_labels: out must not overlap labels");
  }
  int32_t* ws = (int32_t*)workspace;
  int32_t* parent = ws + CC_HEAD;
  int32_t* area = parent + sh.n4;
  unsigned long long* keys = (unsigned long long*)(area + sh.n4);
  hipStream_t st = (hipStream_t)stream;
  const int ma = (int)std::min<int64_t>(min_area, 0x7fffffff);                // areas are < 2^31
  if (hipMemsetAsync(area, 0, (size_t)sh.n4 * 12, st) != hipSuccess) return catseg_launch_status("sieve_labels");
  cc_label_launch<true>(labels, H, W, ld, clamp_pred, connectivity, sh, parent, nullptr, nullptr, area, st);
  const unsigned blocks = (unsigned)((sh.n + 255) / 256);
  hipLaunchKernelGGL(cc_sieve_pairs_kernel, dim3(blocks), dim3(256), 0, st, parent, area, (int)H, (int)W,
                     connectivity == 8, ma, keys);
  hipLaunchKernelGGL(cc_sieve_out_kernel, dim3(blocks), dim3(256), 0, st, labels, (int)H, (int)W, ld, clamp_pred, parent,
                     area, keys, ma, out, ld_out);
  return catseg_launch_status("sieve_labels");
}
