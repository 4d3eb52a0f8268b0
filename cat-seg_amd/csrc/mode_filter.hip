// The majority (mode) filter and the mode-resampled overviews of an int32 label map (include/catseg_hip_mode.h;
// DESIGN.md section 4, "Mode filter and overviews").  One launch each, no workspace, integer only after the score's
// conversion to a weight, the logic in mode_filter_logic.h.  No dictionary and no cap on the number of distinct
// labels: the labels that vote are visited in ascending order, the next one found by a minimum reduction.
//
// catseg_mode_filter, a workgroup of 256 threads per 64 x 16 output tile:
//   stage    the labels and the votes (mf_votes) of the tile plus a halo of r = size / 2, at most 78 x 30, into
//            LDS; a position outside the map holds no vote, which is all the clipping of the windows takes; the
//            first mask is the votes themselves (every label): its windowed sum is the pixel's total;
//   sums     separably: rs[row][x] = the sum of the mask over [x - r, x + r] for the 16 + 2r rows, a wave per row,
//            the lanes on consecutive dwords (no bank conflict); then a thread owns column x of 4 consecutive rows
//            and walks the 4 + 2r row sums of its column once;
//   keep     per pixel the best (sum, label), the own label's sum and the total stay in registers;
//   sweep    the next mask = the votes where the label is the next candidate, else 0, and, in the same sweep, the
//            minimum key above that candidate (a wave reduction by shuffles, the four waves' minima through LDS):
//            the candidate after it.
// Two barriers per candidate.  The loop ends when no key is left: at most one pass per staged position, plus one.
// A footprint with a single label takes the total's pass and one candidate's, and writes what it read.
//
// catseg_mode_overview, a group of G = mo_group(factor) lanes per f x f cell, 64 / G cells per wave, 4 waves per
// workgroup: lane l of a group owns pixels l, l + G, ... of its cell (at most 16), kept in LDS slots only it reads
// ([slot][lane]: consecutive lanes on consecutive dwords), so no barrier is needed; total, next candidate and
// candidate sum are xor-butterfly reductions inside the group.  The loop runs while any cell of the wave has a
// candidate left and is bounded by the cell's size.
// No workgroup waits for another; every map index is 64-bit.
#include "common.h"
#include "capi.h"
#include "mode_filter_logic.h"

namespace {

constexpr int MF_LW = MF_TILE_W + MF_MAX_SIZE - 1;   // 78
constexpr int MF_LH = MF_TILE_H + MF_MAX_SIZE - 1;   // 30
constexpr int MF_ROWS = MF_TILE_H / 4;               // rows of a tile one thread owns
constexpr int MO_SLOTS = MF_MAX_FACTOR * MF_MAX_FACTOR / 64;   // pixels of a cell one lane owns, at most

struct MfArgs {
  const int32_t* labels;
  const float* score;
  int32_t* out;
  int64_t ld, ld_score, ld_out;
  int H, W, r, rule_half, has_novote, novote_label, fill;
};

struct MoArgs {
  const int32_t* labels;
  const float* score;
  int32_t *out, *votes, *total;
  int64_t ld, ld_score, cells;
  int H, W, Wo, factor, group, has_novote, novote_label;
};

// reductions over aligned groups of `width` lanes (a power of two, at most 64); every lane gets the result
__device__ __forceinline__ int64_t group_min_i64(int64_t v, int width) {
  for (int o = 1; o < width; o <<= 1) {
    const int lo = __shfl_xor((int)(uint32_t)v, o, 64), hi = __shfl_xor((int)(v >> 32), o, 64);
    const int64_t t = (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
    v = t < v ? t : v;
  }
  return v;
}

__device__ __forceinline__ int group_sum_i32(int v, int width) {
  for (int o = 1; o < width; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(256) void mode_filter_kernel(MfArgs a) {
  __shared__ int lab[MF_LH * MF_LW];                 // pixel (x, y) at (y - y0 + r, x - x0 + r)
  __shared__ int vot[MF_LH * MF_LW];
  __shared__ int msk[MF_LH * MF_LW];
  __shared__ int rs[MF_LH * MF_TILE_W];
  __shared__ int64_t red[4];
  const int r = a.r, H = a.H, W = a.W, LW = MF_TILE_W + 2 * r, LH = MF_TILE_H + 2 * r, n = LW * LH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = blockIdx.x * MF_TILE_W, y0 = blockIdx.y * MF_TILE_H;

  int64_t part = MF_NO_KEY;
  for (int i = tid; i < n; i += 256) {
    const int yy = i / LW, xx = i - yy * LW, x = x0 - r + xx, y = y0 - r + yy;
    int l = 0, v = 0;
    if (x >= 0 && x < W && y >= 0 && y < H) {
      l = a.labels[(int64_t)y * a.ld + x];
      v = mf_votes(l, a.score != nullptr, a.score ? a.score[(int64_t)y * a.ld_score + x] : 0.0f, a.has_novote != 0,
                   a.novote_label);
    }
    lab[i] = l;
    vot[i] = v;
    msk[i] = v;
    part = mf_next_key(part, MF_FIRST, l, v);
  }
  part = group_min_i64(part, 64);
  if (lane == 0) red[wave] = part;
  __syncthreads();

  const int px = lane, py = wave * MF_ROWS;          // this thread's pixels: column px, rows py .. py + 3 of the tile
  int own[MF_ROWS], own_sum[MF_ROWS], total[MF_ROWS];
  MfBest best[MF_ROWS];
#pragma unroll
  for (int j = 0; j < MF_ROWS; ++j) {
    own[j] = lab[(py + j + r) * LW + px + r];
    own_sum[j] = 0, total[j] = 0;
    best[j] = MfBest{0, own[j]};
  }

  int64_t cand = MF_NO_KEY;                          // the label of the mask in msk; none in pass 0 (the totals)
  for (int pass = 0; pass <= n; ++pass) {
    int64_t next = red[0];                           // the candidate after `cand`, the same in every thread
#pragma unroll
    for (int w = 1; w < 4; ++w) next = red[w] < next ? red[w] : next;
    for (int i = tid; i < LH * MF_TILE_W; i += 256) {
      const int* row = msk + (i >> 6) * LW + (i & 63);            // row[q]: column x0 + (i & 63) - r + q
      rs[i] = mf_span_sum(0, 2 * r, [&](int q) { return row[q]; });
    }
    __syncthreads();
    int s[MF_ROWS];
#pragma unroll
    for (int j = 0; j < MF_ROWS; ++j) s[j] = 0;
    for (int q = 0; q < MF_ROWS + 2 * r; ++q) {
      const int v = rs[(py + q) * MF_TILE_W + px];
#pragma unroll
      for (int j = 0; j < MF_ROWS; ++j) s[j] += (q >= j && q <= j + 2 * r) ? v : 0;
    }
    if (pass == 0) {
#pragma unroll
      for (int j = 0; j < MF_ROWS; ++j) total[j] = s[j];
    } else {
      const int c = mf_label(cand);
#pragma unroll
      for (int j = 0; j < MF_ROWS; ++j) {
        best[j] = mf_offer(best[j], s[j], c);
        own_sum[j] = own[j] == c ? s[j] : own_sum[j];
      }
    }
    if (next == MF_NO_KEY) break;
    cand = next;
    const int c = mf_label(cand);
    part = MF_NO_KEY;
    for (int i = tid; i < n; i += 256) {
      const int l = lab[i], v = vot[i];
      msk[i] = l == c ? v : 0;
      part = mf_next_key(part, cand, l, v);
    }
    part = group_min_i64(part, 64);
    if (lane == 0) red[wave] = part;
    __syncthreads();
  }

  const int x = x0 + px;
#pragma unroll
  for (int j = 0; j < MF_ROWS; ++j) {
    const int y = y0 + py + j;
    if (x < W && y < H)
      a.out[(int64_t)y * a.ld_out + x] = mf_decide(own[j], own_sum[j], best[j], total[j], a.rule_half != 0,
                                                   a.has_novote != 0, a.novote_label, a.fill != 0);
  }
}

__global__ __launch_bounds__(256) void mode_overview_kernel(MoArgs a) {
  __shared__ int lab[4][MO_SLOTS][64];
  __shared__ int vot[4][MO_SLOTS][64];               // -1: no pixel of the map
  const int f = a.factor, G = a.group, H = a.H, W = a.W;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = lane & (G - 1);
  const int64_t cell = ((int64_t)blockIdx.x * 4 + wave) * (64 / G) + lane / G;
  const bool live = cell < a.cells;
  const int Y = live ? (int)(cell / a.Wo) : 0, X = live ? (int)(cell - (int64_t)Y * a.Wo) : 0;
  const int npx = f * f, slots = (npx + G - 1) / G;

  int tot = 0;
  int64_t next = MF_NO_KEY, least = MF_NO_KEY;       // least: the smallest label of the cell, voting or not
  for (int k = 0; k < slots; ++k) {
    const int p = gl + k * G, cy = p / f, cx = p - cy * f, y = Y * f + cy, x = X * f + cx;
    int l = 0, v = -1;
    if (live && p < npx && y < H && x < W) {
      l = a.labels[(int64_t)y * a.ld + x];
      v = mf_votes(l, a.score != nullptr, a.score ? a.score[(int64_t)y * a.ld_score + x] : 0.0f, a.has_novote != 0,
                   a.novote_label);
      tot += v;
      least = mf_key(l) < least ? mf_key(l) : least;
    }
    lab[wave][k][lane] = l;
    vot[wave][k][lane] = v;
    next = mf_next_key(next, MF_FIRST, l, v);
  }
  tot = group_sum_i32(tot, G);
  next = group_min_i64(next, G);
  least = group_min_i64(least, G);
  MfBest best = {0, a.has_novote ? a.novote_label : (least == MF_NO_KEY ? 0 : mf_label(least))};

  for (int it = 0; it <= npx; ++it) {
    if (!__any(next != MF_NO_KEY)) break;            // no cell of this wave has a candidate left
    const int64_t cand = next;
    const bool has = cand != MF_NO_KEY;
    const int c = has ? mf_label(cand) : 0;
    int s = 0;
    int64_t after = MF_NO_KEY;
    for (int k = 0; k < slots; ++k) {
      const int l = lab[wave][k][lane], v = vot[wave][k][lane];
      s += (has && v > 0 && l == c) ? v : 0;
      after = mf_next_key(after, cand, l, v);
    }
    s = group_sum_i32(s, G);
    after = group_min_i64(after, G);
    if (has) best = mf_offer(best, s, c);
    next = after;
  }
  if (live && gl == 0) {
    a.out[cell] = best.label;
    a.votes[cell] = best.sum;
    a.total[cell] = tot;
  }
}

bool mf_side(int64_t v) { return v >= 1 && v <= MF_MAX_SIDE; }

// the H rows of W elements at a with row stride lda share no element with those at b with row stride ldb
bool mf_disjoint(const int32_t* a, int64_t lda, const int32_t* b, int64_t ldb, int64_t H, int64_t W) {
  const int32_t *ae = a + (H - 1) * lda + W, *be = b + (H - 1) * ldb + W;
  if (ae <= b || be <= a) return true;
  if (lda != ldb || ((uintptr_t)a - (uintptr_t)b) % 4) return false;
  int64_t d = (b - a) % lda;                         // two views of one pitched buffer: columns apart
  if (d < 0) d += lda;
  return d >= W && d <= lda - W;
}

}  // namespace

extern "C" int catseg_mode_filter(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int size, int rule_half,
                                  const float* score, int64_t ld_score, int has_novote, int novote_label, int fill,
                                  int32_t* out, int64_t ld_out, void* stream) {
  CATSEG_CHECK(labels && out, "mode_filter: null pointer");
  CATSEG_CHECK(mf_side(H) && mf_side(W), "mode_filter: H and W must lie in 1 .. 16384");
  CATSEG_CHECK(size >= MF_MIN_SIZE && size <= MF_MAX_SIZE && (size & 1), "mode_filter: size must be odd, 3 .. 15");
  CATSEG_CHECK(ld >= W && ld_out >= W && (!score || ld_score >= W), "mode_filter: a row stride is smaller than W");
  CATSEG_CHECK(((uintptr_t)labels % 4) == 0 && ((uintptr_t)score % 4) == 0 && ((uintptr_t)out % 4) == 0,
               "mode_filter: misaligned pointer");
  CATSEG_CHECK(mf_disjoint(labels, ld, out, ld_out, H, W), "mode_filter: out overlaps labels");
  MfArgs a = {};
  a.labels = labels, a.score = score, a.out = out, a.ld = ld, a.ld_score = ld_score, a.ld_out = ld_out;
  a.H = (int)H, a.W = (int)W, a.r = size / 2, a.rule_half = rule_half != 0, a.has_novote = has_novote != 0;
  a.novote_label = novote_label, a.fill = fill != 0;
  hipLaunchKernelGGL(mode_filter_kernel,
                     dim3((unsigned)((W + MF_TILE_W - 1) / MF_TILE_W), (unsigned)((H + MF_TILE_H - 1) / MF_TILE_H)),
                     dim3(256), 0, (hipStream_t)stream, a);
  return catseg_launch_status("mode_filter");
}

extern "C" int catseg_mode_overview(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int factor,
                                    const float* score, int64_t ld_score, int has_novote, int novote_label,
                                    int32_t* out_labels, int32_t* votes, int32_t* total, void* stream) {
  CATSEG_CHECK(labels && out_labels && votes && total, "mode_overview: null pointer");
  CATSEG_CHECK(mf_side(H) && mf_side(W), "mode_overview: H and W must lie in 1 .. 16384");
  CATSEG_CHECK(factor >= MF_MIN_FACTOR && factor <= MF_MAX_FACTOR, "mode_overview: factor must lie in 2 .. 32");
  CATSEG_CHECK(ld >= W && (!score || ld_score >= W), "mode_overview: a row stride is smaller than W");
  CATSEG_CHECK(((uintptr_t)labels % 4) == 0 && ((uintptr_t)score % 4) == 0 && ((uintptr_t)out_labels % 4) == 0 &&
                   ((uintptr_t)votes % 4) == 0 && ((uintptr_t)total % 4) == 0,
               "mode_overview: misaligned pointer");
  MoArgs a = {};
  a.labels = labels, a.score = score, a.out = out_labels, a.votes = votes, a.total = total;
  a.ld = ld, a.ld_score = ld_score, a.H = (int)H, a.W = (int)W, a.factor = factor, a.group = mo_group(factor);
  a.Wo = (int)((W + factor - 1) / factor);
  a.cells = (int64_t)a.Wo * ((H + factor - 1) / factor);
  a.has_novote = has_novote != 0, a.novote_label = novote_label;
  const int64_t per_block = 4 * (64 / a.group);
  hipLaunchKernelGGL(mode_overview_kernel, dim3((unsigned)((a.cells + per_block - 1) / per_block)), dim3(256), 0,
                     (hipStream_t)stream, a);
  return catseg_launch_status("mode_overview");
}
