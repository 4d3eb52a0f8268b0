// The 16 x 64 output tile that the fused postprocess kernels share (post_argmax.hip: one view, argmax
// over the classes; post_tta.hip: the merge of K views): one definition of everything that makes their
// values equal catseg_postprocess's banded path (post_sep_kernel / post_band_kernel, misc.hip) and each
// other, bit for bit.  A value is lin_idx taps, the optional sigmoid 1 / (1 + __expf(-logit)) on the SOURCE
// logit, top = fma(lx, r0[x1] - r0[x0], r0[x0]), bot likewise, fma(ly, bot - top, top).
//
// A workgroup of 256 threads owns one tile; a thread owns 4 consecutive pixels of a row.  The tile's source
// patch (pr x pc floats per class) is staged in LDS for a chunk of TC classes: a thread stages PT_SLOTS =
// NPP * TC floats, patch elements tid + 256 j (j < NPP, NPP the compile-time number of 256-element passes
// over the patch) of TC classes, so every slot's class and LDS offset are compile-time and no index is
// divided in a loop.  LDS keeps the chunk's classes innermost, [patch element][TCP], so the 4 taps of a
// pixel are read for 4 classes at a time (ds_read_b128 at TC >= 4) at immediate offsets; TCP pads TC to
// 4 * odd floats, which spreads neighbouring patch elements over the 16-byte LDS slots.
//
// Both objects are built with NaNs honoured and without SLP re-packing (Makefile).
#pragma once
#include <algorithm>
#include <type_traits>
#include "common.h"
#include "resize_idx.h"

constexpr int PT_ROWS = 16, PT_COLS = 64;      // output tile: 256 threads x 4 pixels of a row
constexpr int PT_SLOTS = 16;                   // staged floats per thread and chunk
constexpr int PT_CAP = PT_SLOTS * 256;         // largest source patch of one class, floats

constexpr int pt_tcp(int tc) { return tc == 16 ? 20 : tc == 8 ? 12 : tc; }   // 4 * odd at TC >= 4
constexpr int pt_vw(int tc) { return tc >= 4 ? 4 : tc; }                     // classes per LDS read

// NaN on the bits, as confusion_kernel (evaluate.hip)
DEV bool pt_is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

struct PtPatch {                               // one view's source patch of a tile
  int ya, xa, pr, pc, ch, cw, flip;
};

// The source patch of the tile at (ty0, tx0) for a crop of (ch, cw): first and last tap row / column (the
// taps are non-decreasing in the output index).  pr x pc is what is staged; the host's PR x PC bounds it
// and sizes the buffers.  A mirrored view reads output columns [x0, x1] at [W - 1 - x1, W - 1 - x0].
DEV PtPatch pt_patch(int ty0, int tx0, int ch, int cw, int flip, int H, int W, int PR, int PC) {
  PtPatch g;
  g.ch = ch;
  g.cw = cw;
  g.flip = flip;
  const float sy = (float)ch / (float)H, sx = (float)cw / (float)W;
  const int tx1 = min(tx0 + PT_COLS, W) - 1;   // last column of the tile inside the image
  const int xlo = flip ? W - 1 - tx1 : tx0, xhi = flip ? W - 1 - tx0 : tx1;
  int yb, xb, tmp;
  float lt;
  lin_idx(ty0, ch, sy, g.ya, tmp, lt);
  lin_idx(xlo, cw, sx, g.xa, tmp, lt);
  lin_idx(min(ty0 + PT_ROWS, H) - 1, ch, sy, tmp, yb, lt);
  lin_idx(xhi, cw, sx, tmp, xb, lt);
  g.pr = min(yb - g.ya + 1, PR);
  g.pc = min(xb - g.xa + 1, PC);
  return g;
}

struct PtTaps {                                // a thread's 4 pixels: LDS offsets of their 4 taps, weights
  int t00[4], t01[4], t10[4], t11[4];
  float lx[4], ly;
};

// The taps of the 4 pixels at (y, x .. x + 3).  Pixels beyond the image clamp to its last row / column
// (their results are not stored); the offsets are clamped into the patch from above, which the host sizes
// to hold every tap of the tile.  No clamp from below (the single-view form; the multi-view kernel had
// one): lin_idx is non-decreasing in the output index and every (mirrored) column of the tile lies in the
// range whose first tap is xa, so x0 - xa >= 0.
template <int TCP>
DEV void pt_taps(const PtPatch& g, int y, int x, int H, int W, PtTaps& t) {
  const float sy = (float)g.ch / (float)H, sx = (float)g.cw / (float)W;
  int y0, y1;
  lin_idx(min(y, H - 1), g.ch, sy, y0, y1, t.ly);
  const int ro0 = min(y0 - g.ya, g.pr - 1) * g.pc, ro1 = min(y1 - g.ya, g.pr - 1) * g.pc;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xo = min(x + k, W - 1), xs = g.flip ? W - 1 - xo : xo;
    int x0, x1;
    lin_idx(xs, g.cw, sx, x0, x1, t.lx[k]);
    const int o0 = min(x0 - g.xa, g.pc - 1), o1 = min(x1 - g.xa, g.pc - 1);
    t.t00[k] = (ro0 + o0) * TCP;
    t.t01[k] = (ro0 + o1) * TCP;
    t.t10[k] = (ro1 + o0) * TCP;
    t.t11[k] = (ro1 + o1) * TCP;
  }
}

// This thread's patch elements (one per pass): source offset inside a class plane of row stride w.
// Elements past the patch repeat its last one (loaded, never written to LDS).
template <int NPP>
DEV void pt_offsets(const PtPatch& g, int tid, int w, int (&off)[NPP]) {
  const int pp = g.pr * g.pc;
#pragma unroll
  for (int j = 0; j < NPP; ++j) {
    const int rc = min(tid + 256 * j, pp - 1), r = rc / g.pc, c = rc - r * g.pc;
    off[j] = min(g.ya + r, g.ch - 1) * w + min(g.xa + c, g.cw - 1);
  }
}

// A thread's staged floats of one chunk, [class][pass]: TC * NPP <= PT_SLOTS of them
template <int TC, int NPP>
struct PtStage {
  float v[TC * NPP];
  DEV void load(const float* src, int64_t plane, const int (&off)[NPP], int t0, int T) {
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      const float* s = src + (int64_t)min(t0 + tt, T - 1) * plane;
#pragma unroll
      for (int j = 0; j < NPP; ++j) v[tt * NPP + j] = s[off[j]];
    }
  }
  template <bool SIG>
  DEV void write(float* buf, int tid, int pp) const {
#pragma unroll
    for (int j = 0; j < NPP; ++j)
      if (tid + 256 * j < pp) {
#pragma unroll
        for (int tt = 0; tt < TC; ++tt) {
          const float x = v[tt * NPP + j];
          buf[(tid + 256 * j) * pt_tcp(TC) + tt] = SIG ? 1.f / (1.f + __expf(-x)) : x;
        }
      }
  }
};

// One pixel's value for VW consecutive classes of a staged chunk: the 4 tap reads at `buf` + the tap
// offsets, then the three fmas.  At VW >= 2 two classes go through one packed fp32 instruction (the pairs
// are register pairs of the reads); each lane of v_pk_fma_f32 is the same IEEE fma as the scalar form.
template <int VW>
DEV void pt_lerp(const float* p00, const float* p01, const float* p10, const float* p11, float lx, float ly,
                    float (&v)[VW]) {
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const vec_t a = *reinterpret_cast<const vec_t*>(p00);
  const vec_t bb = *reinterpret_cast<const vec_t*>(p01);
  const vec_t c = *reinterpret_cast<const vec_t*>(p10);
  const vec_t d = *reinterpret_cast<const vec_t*>(p11);
  if constexpr (VW >= 2) {
    const f32x2 lx2 = {lx, lx}, ly2 = {ly, ly};
    auto lerp2 = [&](f32x2 a2, f32x2 b2, f32x2 c2, f32x2 d2, float* out) {
      const f32x2 top = __builtin_elementwise_fma(lx2, b2 - a2, a2);
      const f32x2 bot = __builtin_elementwise_fma(lx2, d2 - c2, c2);
      const f32x2 vv = __builtin_elementwise_fma(ly2, bot - top, top);
      out[0] = vv[0];
      out[1] = vv[1];
    };
    if constexpr (VW == 4) {
      lerp2(__builtin_shufflevector(a, a, 0, 1), __builtin_shufflevector(bb, bb, 0, 1),
            __builtin_shufflevector(c, c, 0, 1), __builtin_shufflevector(d, d, 0, 1), v);
      lerp2(__builtin_shufflevector(a, a, 2, 3), __builtin_shufflevector(bb, bb, 2, 3),
            __builtin_shufflevector(c, c, 2, 3), __builtin_shufflevector(d, d, 2, 3), v + 2);
    } else {
      lerp2(a, bb, c, d, v);
    }
  } else {
    const float top = fmaf(lx, bb[0] - a[0], a[0]);
    const float bot = fmaf(lx, d[0] - c[0], c[0]);
    v[0] = fmaf(ly, bot - top, top);
  }
}

// 16-byte stores of a thread's 4 pixels at element o of a row of width W, x its first column: possible
// when all 4 are inside, the pointers are 16-byte aligned (out_vec, from the host) and o is a multiple of 4
DEV bool pt_vec_ok(int x, int W, int out_vec, int64_t o) { return x + 3 < W && out_vec && (o & 3) == 0; }

DEV void pt_store_labels(int32_t* labels, float* score, int64_t o, int x, int W, bool vec_ok, const int (&arg)[4],
                         const float (&best)[4]) {
  if (vec_ok) {
    *reinterpret_cast<int4*>(labels + o) = make_int4(arg[0], arg[1], arg[2], arg[3]);
    if (score) *reinterpret_cast<float4*>(score + o) = make_float4(best[0], best[1], best[2], best[3]);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x + k < W) {
        labels[o + k] = arg[k];
        if (score) score[o + k] = best[k];
      }
  }
}

// ---------------------------------------------------------------- host
// Source patch of a tile along one axis: n consecutive outputs span at most floor(scale * (n - 1)) + 2
// source indices beyond the first (i0 spread + the i1 tap); one more for the rounding of the fp32 taps.
// A mirrored tile is n consecutive outputs too.
inline int64_t pt_patch_bound(int tile, int crop, int out) {
  return std::min<int64_t>(crop, (int64_t)(tile - 1) * crop / out + 4);
}

// The LDS stage holds PT_CAP floats of one class; beyond that (pp > PT_CAP) not even one class per chunk
// fits.  The entry's name goes in front of the message and its own words (which view) in the middle.
#define PT_PATCH_MSG(entry, where)                                                                     \
  entry ": the source patch of one 16 x 64 output tile exceeds the LDS stage (4096 floats per class)" \
  where ": downsampling factor too large"

// 256-element passes over a patch of pp floats, and the kernel instantiation for it: f is called with
// std::integral_constant<int, NPP>
inline int pt_npp(int64_t pp) { return pp <= 256 ? 1 : pp <= 512 ? 2 : pp <= 1024 ? 4 : pp <= 2048 ? 8 : 16; }

template <class F>
void pt_dispatch(int npp, F&& f) {
  switch (npp) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 8: return f(std::integral_constant<int, 8>{});
    default: return f(std::integral_constant<int, 16>{});
  }
}
