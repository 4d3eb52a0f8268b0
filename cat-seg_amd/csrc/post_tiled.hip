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

template <bool LABELS, int NPP>
__global__ __launch_bounds__(256) void tiled_merge_kernel(const float* __restrict__ lg, int T, int h, int w, int ch,
                                                          int cw, const TmAxis ay, const TmAxis ax, int row0, int y0,
                                                          int y1, int PR, int PC, float* __restrict__ probs,
                                                          int32_t* __restrict__ labels, float* __restrict__ score,
                                                          int cap, int chunks_per_z, int out_vec) {
  constexpr int TC = pt_tc(NPP);                 // classes per chunk
  constexpr int TCP = pt_tcp(TC);                // their padded LDS stride
  constexpr int VW = pt_vw(TC);                  // classes per LDS read
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

  // view k: its origin, the part of it the region reads, the source patch of that part
  auto geo = [&](int k) {
    TmView v;
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
    const int64_t slot = (int64_t)(r0 + k / nc - row0) * ax.n + (c0 + k % nc);
    stage.load(lg + slot * T * plane, plane, off, t0, T);
  };

  // 1 / count of this thread's pixels: the tile rows that cover y times the tile columns that cover x + k
  float rK[4];
  {
    int ny = 0;
    for (int r = r0; r <= r1; ++r) {
      const int ly = y - tm_origin(ay, r);
      ny += (ly >= 0 && ly < th) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int nx = 0;
      for (int c = c0; c <= c1; ++c) {
        const int lx = x + k - tm_origin(ax, c);
        nx += (lx >= 0 && lx < tw) ? 1 : 0;
      }
      rK[k] = 1.0f / (float)max(ny * nx, 1);     // 0 only beyond the region: never stored
    }
  }

  float acc[TC * 4];                             // [class of the chunk][pixel]: the sum over the covering tiles
  auto accumulate = [&](const float* buf, const TmView& v, auto first) {
    PtTaps tp;
    const unsigned cov = tm_taps<TCP>(v, y, x, th, tw, tp);
#pragma unroll
    for (int gI = 0; gI < TC; gI += VW) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float val[VW];
        pt_lerp<VW>(buf + tp.t00[k] + gI, buf + tp.t01[k] + gI, buf + tp.t10[k] + gI, buf + tp.t11[k] + gI, tp.lx[k],
                    tp.ly, val);
        const bool c = (cov >> k) & 1;
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          float& s = acc[(gI + e) * 4 + k];
          if constexpr (decltype(first)::value) s = c ? val[e] : 0.f;   // s = 0 + p
          else s = c ? s + val[e] : s;                                    // s = s + p_i, in tile order
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
  // after the last view of a chunk: scale, then store or compare (post_tta_kernel's finish)
  auto finish = [&](int t0) {
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      float m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = acc[tt * 4 + k] * rK[k];
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
    for (int k = 0; k < K; ++k) {
      const int kn = k + 1 < K ? k + 1 : 0;
      const int tn = k + 1 < K ? t0 : t0 + TC;
      const bool more = tn < tend;
      TmView gn = gc;
      if (more) {                                // in flight while this step is accumulated
        gn = geo(kn);
        load_step(gn, kn, tn);
      }
      const float* buf = smem + cur * cap * TCP;
      if (k == 0) accumulate(buf, gc, std::true_type{});
      else accumulate(buf, gc, std::false_type{});
      if (k == K - 1) finish(t0);
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

extern "C" int catseg_tiled_merge(const float* logits, int T, int h, int w, int crop_h, int crop_w, int H, int W, int th,
                                  int tw, int sy, int sx, int row0, int rows, int y0, int y1, float* probs,
                                  int32_t* labels, float* score, void* stream) {
  char msg[224];
  CATSEG_CHECK(logits, "tiled_merge: null pointer (logits)");
  CATSEG_CHECK(probs || labels, "tiled_merge: no output (probs and labels are both NULL)");
  CATSEG_CHECK(labels || !score, "tiled_merge: score needs labels");
  CATSEG_CHECK(T > 0 && H > 0 && W > 0, "tiled_merge: T, H, W must be positive");
  CATSEG_CHECK(h > 0 && w > 0 && crop_h > 0 && crop_h <= h && crop_w > 0 && crop_w <= w,
               "tiled_merge: need 0 < crop <= (h, w)");
  CATSEG_CHECK(th > 0 && th <= H && tw > 0 && tw <= W, "tiled_merge: need 0 < (th, tw) <= (H, W)");
  // an axis no longer than its tile has one tile (th == H: th is t' = min(t, H)) and its stride plays no part
  CATSEG_CHECK(sy > 0 && sx > 0 && (th == H || (2 * (int64_t)sy >= th && sy <= th)) &&
                   (tw == W || (2 * (int64_t)sx >= tw && sx <= tw)),
               "tiled_merge: need tile / 2 <= stride <= tile per axis");
  CATSEG_CHECK(0 <= y0 && y0 < y1 && y1 <= H, "tiled_merge: need 0 <= y0 < y1 <= H");
  const TmAxis ay = {H, th, sy, (int)(((int64_t)H - th + sy - 1) / sy + 1)};
  const TmAxis ax = {W, tw, sx, (int)(((int64_t)W - tw + sx - 1) / sx + 1)};
  CATSEG_CHECK(row0 >= 0 && rows >= 1 && (int64_t)row0 + rows <= ay.n,
               "tiled_merge: the window [row0, row0 + rows) leaves the grid's tile rows");
  const int need0 = tm_first(ay, y0), need1 = tm_last(ay, y1 - 1);
  if (need0 < row0 || need1 >= row0 + rows) {
    snprintf(msg, sizeof msg, "tiled_merge: output rows [%d, %d) are covered by tile rows %d .. %d, the window holds "
             "%d .. %d", y0, y1, need0, need1, row0, row0 + rows - 1);
    CATSEG_FAIL(msg);
  }
  CATSEG_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)probs % 4) == 0 && ((uintptr_t)labels % 4) == 0 &&
                   ((uintptr_t)score % 4) == 0,
               "tiled_merge: misaligned pointer");
  const int64_t gx = ((int64_t)W + PT_COLS - 1) / PT_COLS, gy = ((int64_t)(y1 - y0) + PT_ROWS - 1) / PT_ROWS;
  CATSEG_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535, "tiled_merge: grid out of range (need ceil((y1 - y0) / 16) <= 65535)");
  CATSEG_CHECK((int64_t)h * w < ((int64_t)1 << 31), "tiled_merge: source plane too large");
  // source patch of a full region inside one tile: sizes the LDS stage and picks the instantiation
  const int64_t PR = pt_patch_bound(PT_ROWS, crop_h, th), PC = pt_patch_bound(PT_COLS, crop_w, tw);
  const int64_t cap = PR * PC;
  if (cap > PT_CAP) {
    snprintf(msg, sizeof msg, PT_PATCH_MSG("tiled_merge", " of a tile"));
    CATSEG_FAIL(msg);
  }
  const int npp = pt_npp(cap);
  const int tc = pt_tc(npp);
  const int chunks = (T + tc - 1) / tc;
  // 16-byte stores: a probability row starts at t * H * W + y * W, so W % 4 == 0 is needed there
  const int probs_vec = ((uintptr_t)probs % 16) == 0 && W % 4 == 0;
  const int labels_vec = ((uintptr_t)labels % 16) == 0 && ((uintptr_t)score % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
  auto launch = [&](auto lab, dim3 grid, int cpz) {
    constexpr bool LAB = decltype(lab)::value;
    pt_dispatch(npp, [&](auto n) {
      constexpr int NPP = decltype(n)::value;
      const size_t lds = (size_t)2 * cap * pt_tcp(pt_tc(NPP)) * 4;
      hipLaunchKernelGGL((tiled_merge_kernel<LAB, NPP>), grid, dim3(256), lds, st, logits, T, h, w, crop_h, crop_w, ay, ax,
                         row0, y0, y1, (int)PR, (int)PC, probs, labels, score, (int)cap, cpz,
                         LAB ? labels_vec : probs_vec);
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
    const int rc = catseg_launch_status("tiled_merge");
    if (rc != CATSEG_OK) return rc;
  }
  if (labels) {
    const dim3 grid((unsigned)gx, (unsigned)gy, 1);
    launch(std::true_type{}, grid, chunks);
    return catseg_launch_status("tiled_merge");
  }
  return CATSEG_OK;
}
