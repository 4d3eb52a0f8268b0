// Tiled inference at native resolution: the tile gather and the merge of the tiles' logits on the device.
//
// The grid (one definition, cat_seg/tiling.py): per axis, image extent L, tile t' = min(t, L), stride s,
//   n = max(L - t' + s - 1, 0) / s + 1,   o_i = min(i s, L - t')   (the last tile is shifted back, never padded)
// tiles row-major, every tile of extent (th, tw).  The host passes (L, t', s, n) per axis as scalars; the
// kernels only evaluate o_i and the range of tiles that meet an interval (TmAxis below).
//
// catseg_tile_crops   B tiles of one fp32 image [3][H][W] -> canvas [B][3][ch][cw], zero beyond (th, tw).
// catseg_tiled_merge  for output rows [y0, y1) of the image:
//   p_i(t, y - oy_i, x - ox_i) = the value catseg_postprocess forms on its banded path for tile i, i.e.
//                  (h, w, crop_h, crop_w) -> (th, tw): the value of post_tile.h
//   s = 0; s = s + p_i over the tiles that cover (y, x), in row-major tile order (0 + p = p exactly: p >= +0
//   or NaN);  m = s * (1.0f / (float)count(y, x))
//   probs[t][y][x] = m;  labels[y][x] = first maximum of m over t;  score[y][x] = that maximum
// No atomics and one fixed order per element: deterministic.  The label form and the probability form are
// one template, so labels / score equal the argmax / max of the probability form bit for bit.
// catseg_tiled_blend  the same merge with a window over every tile and, optionally, a global view (one
//   definition of the integers, cat_seg/tiling.py: window_weights / weight_sum):
//   w(l) of local coordinate l of an axis of tile extent t': "uniform" 1, "pyramid" min(l + 1, t' - l) (an
//   integer >= 1);  w_i = w(y - oy_i) * w(x - ox_i), an integer product converted to fp32 (exact: the entry
//   refuses "pyramid" above t' = 2048, so sum(w) <= 2.25 t'^2 < 2^24)
//   s = 0; s = s + (w_i * p_i) over the covering tiles in row-major order: a multiply and an add, two
//   roundings, never one fma;  m = s * (1.0f / (float)sum(w)),  sum(w) = (sum over the covering tile rows of
//   w_y) * (sum over the covering tile columns of w_x), an integer product
//   With global_logits (T, h, w), the whole scene resized to the tile's extent and run like a tile:
//   g(t, y, x) = the value catseg_postprocess forms for them with (crop_h, crop_w) -> (H, W) (pt_patch /
//   pt_taps of post_tile.h, the single-view form of post_argmax.hip);  the output is 0.5f * (m + g): an add,
//   then an exact halving (the reference's (outputs + global_output) / 2.).  It is one more step at the end of
//   every class chunk, through the same two LDS buffers.  "uniform" without a global view is
//   catseg_tiled_merge's arithmetic exactly (1.0f * p = p, sum(w) = count).
//
// The merge is post_tta_kernel's shape (post_tile.h: one workgroup per 16 x 64 output tile, a thread owns 4
// consecutive pixels of a row and 4 x TC fp32 sums for a chunk of TC classes; one step = (chunk, view), the
// view's source patch staged in LDS with the sigmoid applied once per source logit, two buffers, one
// barrier per step).  What differs:
//  * a view is a TILE of the grid and covers only a sub-rectangle of the output.  The views of a workgroup
//    are the tiles that meet its 16 x 64 region: tile rows [r0, r1] x tile columns [c0, c1], a contiguous
//    range per axis (1 x 1 inside a tile, 2 x 2 across a corner, up to 3 per axis where the shifted last
//    tile overlaps two regular ones).  Only their patches are staged, and of each only the part the
//    region's intersection with the tile reads: local rows / columns [la, lb] of the tile.
//  * the cover set differs per pixel inside a workgroup: a pixel adds a view's value only when the tile
//    covers it (a select on the four pixels' cover bits; the taps of an uncovered pixel are clamped into
//    the staged patch and its value is dropped), and the 1 / count scale is per pixel.
//  * TC and the LDS stage follow from one bound, the patch of a full 16 x 64 region of one tile (every
//    tile has the same crop and extent): NPP passes of 256 elements, TC = min(8, 16 / NPP), as there.  At
//    the production geometry (96 x 96 logits -> 384 x 384 tiles) the patch is 7 x 19 floats: NPP = 1, TC = 8,
//    2 x 133 x 12 floats = 12.8 KB of LDS per workgroup.
//
// NaN ranks above every number and the first NaN wins.  Built like post_tta.o (Makefile).
#include <type_traits>
#include "common.h"
#include "capi.h"
#include "post_tile.h"

namespace {

constexpr int pt_tc(int npp) { return npp == 1 ? 8 : PT_SLOTS / npp; }   // classes per chunk, as post_tta.hip

// one axis of the grid; n and t are the host's (cat_seg/tiling.py's formula)
struct TmAxis {
  int L, t, s, n;
};
__host__ DEV int tm_origin(const TmAxis& a, int i) { return std::min(i * a.s, a.L - a.t); }
// first / last tile that meets position p (0 <= p < L); the tiles between them meet [p_first, p_last] too
__host__ DEV int tm_first(const TmAxis& a, int p) { return std::min(p >= a.t ? (p - a.t) / a.s + 1 : 0, a.n - 1); }
__host__ DEV int tm_last(const TmAxis& a, int p) { return a.L - a.t <= p ? a.n - 1 : std::min(p / a.s, a.n - 1); }

struct TmView {                                  // one tile as seen from one workgroup
  PtPatch g;
  int oy, ox, la, lb, ca, cb;                    // origin; local rows [la, lb] and columns [ca, cb] read
};

// The taps of the 4 pixels at image (y, x .. x + 3) in the tile of `v`: pt_taps on the tile's local
// coordinates, clamped into the part of the tile this workgroup reads (so into the staged patch; a clamped
// pixel is not covered and its value is dropped).  cov: bit k set when the tile covers pixel k.
template <int TCP>
DEV unsigned tm_taps(const TmView& v, int y, int x, int th, int tw, PtTaps& t) {
  const PtPatch& g = v.g;
  const float sy = (float)g.ch / (float)th, sx = (float)g.cw / (float)tw;
  const int ly = y - v.oy;
  const bool rowin = ly >= 0 && ly < th;
  int y0, y1;
  lin_idx(min(max(ly, v.la), v.lb), g.ch, sy, y0, y1, t.ly);
  const int ro0 = min(y0 - g.ya, g.pr - 1) * g.pc, ro1 = min(y1 - g.ya, g.pr - 1) * g.pc;
  unsigned cov = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int lx = x + k - v.ox;
    cov |= (unsigned)(rowin && lx >= 0 && lx < tw) << k;
    int x0, x1;
    lin_idx(min(max(lx, v.ca), v.cb), g.cw, sx, x0, x1, t.lx[k]);
    const int o0 = min(x0 - g.xa, g.pc - 1), o1 = min(x1 - g.xa, g.pc - 1);
    t.t00[k] = (ro0 + o0) * TCP;
    t.t01[k] = (ro0 + o1) * TCP;
    t.t10[k] = (ro1 + o0) * TCP;
    t.t11[k] = (ro1 + o1) * TCP;
  }
  return cov;
}

// the window weight of local coordinate l of an axis of tile extent t (cat_seg/tiling.py: window_weights)
DEV int tm_weight(int win, int l, int t) { return win ? min(l + 1, t - l) : 1; }

// a product and a sum that stay two roundings (never contracted into one fma): what lets the blend be
// restated with two elementwise ops
DEV float tm_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
DEV float tm_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}

struct TmBlend {                                 // what catseg_tiled_blend adds to the merge's arguments
  int win, PRg, PCg;                             // window (0 uniform, 1 pyramid); the global view's patch bound
  const float* glg;                              // the global view's logits [T][h][w] (GLOB only)
};

// BLEND = false is catseg_tiled_merge (bl is not read); BLEND adds the window weights, GLOB the global view
// as step K of every class chunk.
// Registers: the merge's NPP = 1 instantiations sit just under the 168 VGPRs of 3 waves per SIMD, and with the
// merge's loop order in accumulate the 4 weights push the blend's past it (176 / 192 VGPRs, 2 waves: 1705 us
// for the pyramid label form, 1367 us with that instantiation held to 168; tools/micro_tiled_merge.py --blend).
// With the pixels as the outer loop the window-only kernels take 144 / 136 and keep 3 waves (1353 us); the
// kernels with a global view take 205 / 196 (2 waves).  The merge's instantiations keep their loop order and
// are compiled as before.
template <bool LABELS, int NPP, bool BLEND, bool GLOB>
__global__ __launch_bounds__(256) void tiled_merge_kernel(const float* __restrict__ lg, int T, int h, int w, int ch,
                                                          int cw, const TmAxis ay, const TmAxis ax, int row0, int y0,
                                                          int y1, int PR, int PC, float* __restrict__ probs,
                                                          int32_t* __restrict__ labels, float* __restrict__ score,
                                                          int cap, int chunks_per_z, int out_vec, const TmBlend bl) {
  const int win = bl.win, PRg = bl.PRg, PCg = bl.PCg;
  const float* __restrict__ glg = bl.glg;
  constexpr int TC = pt_tc(NPP);                 // classes per chunk
  constexpr int TCP = pt_tcp(TC);                // their padded LDS stride
  constexpr int VW = pt_vw(TC);                  // classes per LDS read
  // the accumulate nest: class groups outside, pixels inside for the merge; pixels outside for the blend, so
  // that a pixel's taps and weight die before the next pixel's are needed (see Registers above)
  constexpr int NA = BLEND ? 4 : TC / VW, NB = BLEND ? TC / VW : 4;
  extern __shared__ float smem[];                // [2][cap][TCP], pr * pc elements of each used
  const int tid = threadIdx.x;
  const int H = ay.L, W = ax.L, th = ay.t, tw = ax.t;
  const int ty0 = y0 + blockIdx.y * PT_ROWS, tx0 = blockIdx.x * PT_COLS;
  const int ty1 = min(ty0 + PT_ROWS, y1) - 1, tx1 = min(tx0 + PT_COLS, W) - 1;   // last row / column of the region
  const int y = ty0 + (tid >> 4), x = tx0 + ((tid & 15) << 2);
  const int64_t plane = (int64_t)h * w;
  const int tbeg = blockIdx.z * chunks_per_z * TC;
  const int tend = min(T, tbeg + chunks_per_z * TC);
  if (tbeg >= tend) return;

  // the tiles that meet this region: rows [r0, r1] x columns [c0, c1], walked row-major
  const int r0 = tm_first(ay, ty0), r1 = tm_last(ay, ty1);
  const int c0 = tm_first(ax, tx0), c1 = tm_last(ax, tx1);
  const int nc = c1 - c0 + 1, K = (r1 - r0 + 1) * nc;
  const int KS = GLOB ? K + 1 : K;               // steps of a class chunk: the tiles, then the global view

  // view k: its origin, the part of it the region reads, the source patch of that part
  auto geo = [&](int k) {
    TmView v;
    if constexpr (GLOB) {
      if (k == K) {                              // the global view: the region's patch of (ch, cw) -> (H, W)
        v = TmView{};
        v.g = pt_patch(ty0, tx0, ch, cw, 0, H, W, PRg, PCg);
        return v;
      }
    }
    const int r = r0 + k / nc, c = c0 + k % nc;
    v.oy = tm_origin(ay, r);
    v.ox = tm_origin(ax, c);
    v.la = max(ty0 - v.oy, 0);
    v.lb = min(ty1 - v.oy, th - 1);
    v.ca = max(tx0 - v.ox, 0);
    v.cb = min(tx1 - v.ox, tw - 1);
    PtPatch& g = v.g;
    g.ch = ch;
    g.cw = cw;
    g.flip = 0;
    const float sy = (float)ch / (float)th, sx = (float)cw / (float)tw;
    int yb, xb, tmp;
    float lt;
    lin_idx(v.la, ch, sy, g.ya, tmp, lt);
    lin_idx(v.ca, cw, sx, g.xa, tmp, lt);
    lin_idx(v.lb, ch, sy, tmp, yb, lt);
    lin_idx(v.cb, cw, sx, tmp, xb, lt);
    g.pr = min(yb - g.ya + 1, PR);
    g.pc = min(xb - g.xa + 1, PC);
    return v;
  };
  PtStage<TC, NPP> stage;
  auto load_step = [&](const TmView& v, int k, int t0) {
    int off[NPP];
    pt_offsets<NPP>(v.g, tid, w, off);
    if constexpr (GLOB) {
      if (k == K) {
        stage.load(glg, plane, off, t0, T);
        return;
      }
    }
    const int64_t slot = (int64_t)(r0 + k / nc - row0) * ax.n + (c0 + k % nc);
    stage.load(lg + slot * T * plane, plane, off, t0, T);
  };

  // 1 / count of this thread's pixels: the tile rows that cover y times the tile columns that cover x + k
  // (BLEND: 1 / sum(w), the covering rows' w_y summed times the covering columns' w_x summed, as integers)
  float rK[4];
  {
    int ny = 0;
    for (int r = r0; r <= r1; ++r) {
      const int ly = y - tm_origin(ay, r);
      ny += (ly >= 0 && ly < th) ? (BLEND ? tm_weight(win, ly, th) : 1) : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int nx = 0;
      for (int c = c0; c <= c1; ++c) {
        const int lx = x + k - tm_origin(ax, c);
        nx += (lx >= 0 && lx < tw) ? (BLEND ? tm_weight(win, lx, tw) : 1) : 0;
      }
      rK[k] = 1.0f / (float)max(ny * nx, 1);     // 0 only beyond the region: never stored
    }
  }

  float acc[TC * 4];                             // [class of the chunk][pixel]: the sum over the covering tiles
  auto accumulate = [&](const float* buf, const TmView& v, auto first) {
    PtTaps tp;
    const unsigned cov = tm_taps<TCP>(v, y, x, th, tw, tp);
    float wgt[BLEND ? 4 : 1];                    // w_i of the 4 pixels (of no meaning where the tile does not cover)
    if constexpr (BLEND) {
      const int wy = tm_weight(win, y - v.oy, th);
#pragma unroll
      for (int k = 0; k < 4; ++k) wgt[k] = (float)(wy * tm_weight(win, x + k - v.ox, tw));
    }
#pragma unroll
    for (int ia = 0; ia < NA; ++ia) {
#pragma unroll
      for (int ib = 0; ib < NB; ++ib) {
        const int gI = (BLEND ? ib : ia) * VW, k = BLEND ? ia : ib;
        float val[VW];
        pt_lerp<VW>(buf + tp.t00[k] + gI, buf + tp.t01[k] + gI, buf + tp.t10[k] + gI, buf + tp.t11[k] + gI, tp.lx[k],
                    tp.ly, val);
        const bool c = (cov >> k) & 1;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          float& s = acc[(gI + e) * 4 + k];
          if constexpr (BLEND) {
            const float wp = tm_mul(wgt[k], val[e]);
            if constexpr (decltype(first)::value) s = c ? wp : 0.f;      // s = 0 + w p
            else s = c ? tm_add(s, wp) : s;                               // s = s + (w_i * p_i), in tile order
          } else {
            if constexpr (decltype(first)::value) s = c ? val[e] : 0.f;   // s = 0 + p
            else s = c ? s + val[e] : s;                                    // s = s + p_i, in tile order
          }
        }
      }
    }
  };
  // the last step of a chunk with a global view: acc becomes the final value 0.5f * (m + g)
  auto accumulate_global = [&](const float* buf, const PtPatch& gp) {
    PtTaps tp;
    pt_taps<TCP>(gp, y, x, H, W, tp);
#pragma unroll
    for (int ia = 0; ia < NA; ++ia) {
#pragma unroll
      for (int ib = 0; ib < NB; ++ib) {
        const int gI = (BLEND ? ib : ia) * VW, k = BLEND ? ia : ib;
        float val[VW];
        pt_lerp<VW>(buf + tp.t00[k] + gI, buf + tp.t01[k] + gI, buf + tp.t10[k] + gI, buf + tp.t11[k] + gI, tp.lx[k],
                    tp.ly, val);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          float& s = acc[(gI + e) * 4 + k];
          s = 0.5f * tm_add(tm_mul(s, rK[k]), val[e]);
        }
      }
    }
  };

  float best[4];
  int arg[4];
  bool bnan[4];                                  // this pixel's best is a NaN
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    best[k] = -INFINITY;
    arg[k] = 0;
    bnan[k] = false;
  }
  const bool inside = y <= ty1 && x < W;
  const int64_t o = (int64_t)y * W + x;
  const bool vec_ok = pt_vec_ok(x, W, out_vec, o);
  // after the last view of a chunk: scale (done already with a global view), then store or compare
  // (post_tta_kernel's finish)
  auto finish = [&](int t0) {
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      float m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = GLOB ? acc[tt * 4 + k] : acc[tt * 4 + k] * rK[k];
      if constexpr (LABELS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          // strict >: the first maximum wins; NaN above every number, the first NaN wins
          const bool vn = pt_is_nan_bits(m[k]);
          const bool take = (vn || m[k] > best[k]) && !bnan[k];
          bnan[k] = bnan[k] || (take && vn);
          best[k] = take ? m[k] : best[k];
          arg[k] = take ? t0 + tt : arg[k];
        }
      } else {
        if (inside && t0 + tt < T) {
          float* p = probs + (int64_t)(t0 + tt) * H * W + o;
          if (vec_ok) {
            *reinterpret_cast<float4*>(p) = make_float4(m[0], m[1], m[2], m[3]);
          } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
              if (x + k < W) p[k] = m[k];
          }
        }
      }
    }
  };

  TmView gc = geo(0);
  load_step(gc, 0, tbeg);
  stage.template write<true>(smem, tid, gc.g.pr * gc.g.pc);
  __syncthreads();
  int cur = 0;
  for (int t0 = tbeg; t0 < tend; t0 += TC) {
    for (int k = 0; k < KS; ++k) {
      const int kn = k + 1 < KS ? k + 1 : 0;
      const int tn = k + 1 < KS ? t0 : t0 + TC;
      const bool more = tn < tend;
      TmView gn = gc;
      if (more) {                                // in flight while this step is accumulated
        gn = geo(kn);
        load_step(gn, kn, tn);
      }
      const float* buf = smem + cur * cap * TCP;
      if (GLOB && k == K) accumulate_global(buf, gc.g);
      else if (k == 0) accumulate(buf, gc, std::true_type{});
      else accumulate(buf, gc, std::false_type{});
      if (k == KS - 1) finish(t0);
      cur ^= 1;
      if (more) stage.template write<true>(smem + cur * cap * TCP, tid, gn.g.pr * gn.g.pc);
      __syncthreads();
      gc = gn;
    }
  }

  if constexpr (LABELS) {
    if (inside) pt_store_labels(labels, score, o, x, W, vec_ok, arg, best);
  }
}

constexpr int TC_MAXB = 32;

struct TileOrigins {                             // passed by value in the kernel arguments (256 bytes)
  int oy[TC_MAXB], ox[TC_MAXB];
};

// one thread per canvas element; the canvas is written whole (zero beyond the tile)
__global__ __launch_bounds__(256) void tile_crops_kernel(const float* __restrict__ image, int H, int W,
                                                         const TileOrigins org, int th, int tw,
                                                         float* __restrict__ canvas, int ch, int cw) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y, b = blockIdx.z / 3, c = blockIdx.z % 3;
  if (x >= cw) return;
  float v = 0.f;
  if (y < th && x < tw) v = image[((int64_t)c * H + org.oy[b] + y) * W + org.ox[b] + x];
  canvas[(((int64_t)b * 3 + c) * ch + y) * cw + x] = v;
}

}  // namespace

extern "C" int catseg_tile_crops(const float* image, int H, int W, const int32_t* origins, int B, int th, int tw,
                                 float* canvas, int ch, int cw, void* stream) {
  char msg[192];
  CATSEG_CHECK(image && origins && canvas, "tile_crops: null pointer (image, origins, canvas)");
  CATSEG_CHECK(B >= 1 && B <= TC_MAXB, "tile_crops: B must be in [1, 32]");
  CATSEG_CHECK(H > 0 && W > 0 && th > 0 && tw > 0 && th <= H && tw <= W, "tile_crops: need 0 < (th, tw) <= (H, W)");
  CATSEG_CHECK(ch >= th && cw >= tw && ch <= 65535, "tile_crops: the canvas (ch, cw) must hold the tile (ch <= 65535)");
  TileOrigins org = {};
  for (int b = 0; b < B; ++b) {
    const int oy = origins[2 * b], ox = origins[2 * b + 1];
    if (!(oy >= 0 && oy <= H - th && ox >= 0 && ox <= W - tw)) {
      snprintf(msg, sizeof msg, "tile_crops: origin (%d, %d) of tile %d leaves the image (%d, %d) with tile (%d, %d)", oy,
               ox, b, H, W, th, tw);
      CATSEG_FAIL(msg);
    }
    org.oy[b] = oy;
    org.ox[b] = ox;
  }
  const dim3 grid((unsigned)((cw + 255) / 256), (unsigned)ch, (unsigned)(3 * B));
  hipLaunchKernelGGL(tile_crops_kernel, grid, dim3(256), 0, (hipStream_t)stream, image, H, W, org, th, tw, canvas, ch, cw);
  return catseg_launch_status("tile_crops");
}

// The host side of both merges.  who: the entry's name in front of every message; blend: catseg_tiled_blend
// (window and global_logits then apply), else catseg_tiled_merge.
static int tm_run(const char* who, bool blend, const float* logits, int T, int h, int w, int crop_h, int crop_w, int H,
                  int W, int th, int tw, int sy, int sx, int row0, int rows, int y0, int y1, int window,
                  const float* global_logits, float* probs, int32_t* labels, float* score, void* stream) {
  char msg[256];
#define TM_CHECK(cond, text)                   \
  do {                                         \
    if (!(cond)) {                             \
      catseg_set_error("%s: %s", who, text);   \
      return CATSEG_ERR_ARG;                   \
    }                                          \
  } while (0)
  TM_CHECK(logits, "null pointer (logits)");
  TM_CHECK(probs || labels, "no output (probs and labels are both NULL)");
  TM_CHECK(labels || !score, "score needs labels");
  TM_CHECK(T > 0 && H > 0 && W > 0, "T, H, W must be positive");
  TM_CHECK(h > 0 && w > 0 && crop_h > 0 && crop_h <= h && crop_w > 0 && crop_w <= w, "need 0 < crop <= (h, w)");
  TM_CHECK(th > 0 && th <= H && tw > 0 && tw <= W, "need 0 < (th, tw) <= (H, W)");
  // an axis no longer than its tile has one tile (th == H: th is t' = min(t, H)) and its stride plays no part
  TM_CHECK(sy > 0 && sx > 0 && (th == H || (2 * (int64_t)sy >= th && sy <= th)) &&
               (tw == W || (2 * (int64_t)sx >= tw && sx <= tw)),
           "need tile / 2 <= stride <= tile per axis");
  TM_CHECK(window == 0 || window == 1, "window must be 0 (uniform) or 1 (pyramid)");
  // sum(w) <= 2.25 t'^2 per pixel must stay below 2^24 for the fp32 weights to be exact
  TM_CHECK(window == 0 || (th <= 2048 && tw <= 2048), "the pyramid window needs a tile extent of at most 2048");
  TM_CHECK(0 <= y0 && y0 < y1 && y1 <= H, "need 0 <= y0 < y1 <= H");
  const TmAxis ay = {H, th, sy, (int)(((int64_t)H - th + sy - 1) / sy + 1)};
  const TmAxis ax = {W, tw, sx, (int)(((int64_t)W - tw + sx - 1) / sx + 1)};
  TM_CHECK(row0 >= 0 && rows >= 1 && (int64_t)row0 + rows <= ay.n,
           "the window [row0, row0 + rows) leaves the grid's tile rows");
  const int need0 = tm_first(ay, y0), need1 = tm_last(ay, y1 - 1);
  if (need0 < row0 || need1 >= row0 + rows) {
    snprintf(msg, sizeof msg, "%s: output rows [%d, %d) are covered by tile rows %d .. %d, the window holds "
             "%d .. %d", who, y0, y1, need0, need1, row0, row0 + rows - 1);
    CATSEG_FAIL(msg);
  }
  TM_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)probs % 4) == 0 && ((uintptr_t)labels % 4) == 0 &&
               ((uintptr_t)score % 4) == 0 && ((uintptr_t)global_logits % 4) == 0,
           "misaligned pointer");
  const int64_t gx = ((int64_t)W + PT_COLS - 1) / PT_COLS, gy = ((int64_t)(y1 - y0) + PT_ROWS - 1) / PT_ROWS;
  TM_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535, "grid out of range (need ceil((y1 - y0) / 16) <= 65535)");
  TM_CHECK((int64_t)h * w < ((int64_t)1 << 31), "source plane too large");
  // source patch of a full region inside one tile, and of a region of the global view (the scene resized to
  // a tile's extent, so (crop) -> (H, W)): the larger sizes the LDS stage and picks the instantiation.  With
  // th <= H and tw <= W the global bound never exceeds the tile's; the max states the rule, not a case.
  const int64_t PR = pt_patch_bound(PT_ROWS, crop_h, th), PC = pt_patch_bound(PT_COLS, crop_w, tw);
  const int64_t PRg = global_logits ? pt_patch_bound(PT_ROWS, crop_h, H) : 0;
  const int64_t PCg = global_logits ? pt_patch_bound(PT_COLS, crop_w, W) : 0;
  const int64_t cap = std::max(PR * PC, PRg * PCg);
  if (cap > PT_CAP) {
    const bool tile_over = PR * PC > PT_CAP, glob_over = PRg * PCg > PT_CAP;
    snprintf(msg, sizeof msg, PT_PATCH_MSG("%s", "%s"), who,
             tile_over && glob_over ? " of a tile and of the global view"
             : glob_over            ? " of the global view"
                                    : " of a tile");
    CATSEG_FAIL(msg);
  }
#undef TM_CHECK
  const int npp = pt_npp(cap);
  const int tc = pt_tc(npp);
  const int chunks = (T + tc - 1) / tc;
  // 16-byte stores: a probability row starts at t * H * W + y * W, so W % 4 == 0 is needed there
  const int probs_vec = ((uintptr_t)probs % 16) == 0 && W % 4 == 0;
  const int labels_vec = ((uintptr_t)labels % 16) == 0 && ((uintptr_t)score % 16) == 0;
  const TmBlend bl = {window, (int)PRg, (int)PCg, global_logits};
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto lab, dim3 grid, int cpz) {
    constexpr bool LAB = decltype(lab)::value;
    pt_dispatch(npp, [&](auto n) {
      constexpr int NPP = decltype(n)::value;
      const size_t lds = (size_t)2 * cap * pt_tcp(pt_tc(NPP)) * 4;
      auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), lds, st, logits, T, h, w, crop_h, crop_w, ay, ax, row0, y0, y1,
                           (int)PR, (int)PC, probs, labels, score, (int)cap, cpz, LAB ? labels_vec : probs_vec, bl);
      };
      if (!blend) go(tiled_merge_kernel<LAB, NPP, false, false>);
      else if (global_logits) go(tiled_merge_kernel<LAB, NPP, true, true>);
      else go(tiled_merge_kernel<LAB, NPP, true, false>);
    });
  };
  if (probs) {
    // split the class chunks over grid z until there are about 4 workgroups per compute unit
    const int64_t tiles = gx * gy;
    const int64_t want = std::max<int64_t>(1, ((int64_t)4 * catseg_device_cus() + tiles - 1) / tiles);
    const int nz = (int)std::min<int64_t>(std::min<int64_t>(want, chunks), 65535);
    const int cpz = (chunks + nz - 1) / nz;
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)((chunks + cpz - 1) / cpz));
    launch(std::false_type{}, grid, cpz);
    const int rc = catseg_launch_status(who);
    if (rc != CATSEG_OK) return rc;
  }
  if (labels) {
    const dim3 grid((unsigned)gx, (unsigned)gy, 1);
    launch(std::true_type{}, grid, chunks);
    return catseg_launch_status(who);
  }
  return CATSEG_OK;
}

extern "C" int catseg_tiled_merge(const float* logits, int T, int h, int w, int crop_h, int crop_w, int H, int W, int th,
                                  int tw, int sy, int sx, int row0, int rows, int y0, int y1, float* probs,
                                  int32_t* labels, float* score, void* stream) {
  return tm_run("tiled_merge", false, logits, T, h, w, crop_h, crop_w, H, W, th, tw, sy, sx, row0, rows, y0, y1, 0,
                nullptr, probs, labels, score, stream);
}

extern "C" int catseg_tiled_blend(const float* logits, int T, int h, int w, int crop_h, int crop_w, int H, int W, int th,
                                  int tw, int sy, int sx, int row0, int rows, int y0, int y1, int window,
                                  const float* global_logits, float* probs, int32_t* labels, float* score,
                                  void* stream) {
  return tm_run("tiled_blend", true, logits, T, h, w, crop_h, crop_w, H, W, th, tw, sy, sx, row0, rows, y0, y1, window,
                global_logits, probs, labels, score, stream);
}
