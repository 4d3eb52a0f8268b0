// Merge of the test-time-augmentation views on the device: for K augmented views of one image,
// sigmoid + bilinear resize of each view's low-resolution logits, the flip back of the mirrored
// views, the sum over the views and the 1 / K scale in one kernel (reference
// cat_seg/test_time_augmentation.py:81-108 after cat_seg_model.py:222-227), and for the label form
// also the evaluator's argmax over the classes (plain_train_net.py:107-116).  The K full-size
// (T, H, W) volumes of the torch merge are never formed; the label form forms none at all.
//
//   p_k(t, y, x) = the value catseg_postprocess forms on its banded path for (h, w, crop_h_k, crop_w_k,
//                  H, W): lin_idx taps, 1 / (1 + __expf(-logit)) on the SOURCE logit, the three fmas,
//                  restated here exactly as post_argmax.hip restates them
//   v_k(t, y, x) = p_k(t, y, flip_k ? W - 1 - x : x)
//   s = v_0; s = s + v_k (k = 1 .. K-1, fp32, in view order);  m = s * rK, rK = 1.0f / (float)K (host)
//   probs[t][y][x] = m;  labels[y][x] = first maximum of m over t;  score[y][x] = that maximum
//
// No atomics and one fixed order per element: the result is deterministic.  The label form and the
// probability form are one template and share every arithmetic statement, so labels / score equal the
// argmax / max of what the probability form writes, bit for bit.
//
// What was chosen and why:
//  * post_argmax_kernel's shape: one workgroup per 16 x 64 output tile, a thread owns 4 consecutive
//    pixels of a row.  A thread keeps 4 x TC fp32 sums in registers for a chunk of TC classes and walks
//    the K views for that chunk; after the last view the chunk is scaled and stored (probs) or compared
//    into the thread's running (best, arg) (labels).  Views are the inner loop because the sums of a
//    chunk are the only state that has to survive a view; the other order would need T sums per pixel.
//  * One step = (chunk, view).  The view's source patch of the tile (pr x pc floats per class, 6 x 12 at
//    96 x 96 -> 512 x 684) is staged in LDS for the chunk's classes with the sigmoid applied once per
//    source logit as it is written.  Two buffers: the global loads of step s + 1 are issued before step
//    s is accumulated and written to the other buffer after it (one barrier per step), as there.
//    LDS keeps the chunk's classes innermost ([patch element][TCP]) so the 4 taps of a pixel are read
//    for 4 classes at a time.
//  * Every view has its own crop, so its own patch origin, patch size and tap offsets.  They are
//    recomputed per step from the view table in the kernel arguments (6 lin_idx and 16 offsets, about
//    a hundred scalar / vector instructions against 4 * TC interpolations of ~10 instructions each); a
//    table of them in LDS would save little and cost a second LDS region per workgroup.
//  * A flipped view reads the mirrored tile: output columns [x0, x1] of the tile map to source-side
//    columns [W - 1 - x1, W - 1 - x0], still contiguous, so its patch obeys the same bound.
//  * TC follows from the largest view's patch (NPP passes of 256 elements, TC = min(8, 16 / NPP)), which is
//    also the bound of the LDS stage (4096 floats per class, the rule of catseg_postprocess_argmax).
//  * The probability form has no reduction over the classes, so its grid also splits the class chunks
//    over blockIdx.z until there are a few workgroups per compute unit (a 512 x 684 output has only 352
//    tiles).  The label form keeps all classes in one workgroup.
//
// Built with NaNs honoured and without SLP re-packing, as post_argmax.o (Makefile): NaN ranks above
// every number and the first NaN wins.
#include <type_traits>
#include "common.h"
#include "capi.h"
#include "resize_idx.h"

namespace {

constexpr int PT_ROWS = 16, PT_COLS = 64;      // output tile: 256 threads x 4 pixels of a row
constexpr int PT_SLOTS = 16;                   // staged floats per thread and step
constexpr int PT_CAP = PT_SLOTS * 256;         // largest source patch of one class, floats
constexpr int PT_MAXK = 32;

// classes per chunk: 16 staged floats per thread over NPP passes, but at most 8 (16 classes = 64 sums per
// thread compiled to 256 VGPRs, one wave per SIMD; 8 leave room for two or more)
constexpr int pt_tc(int npp) { return npp == 1 ? 8 : PT_SLOTS / npp; }
constexpr int pt_tcp(int tc) { return tc == 16 ? 20 : tc == 8 ? 12 : tc; }   // 4 * odd at TC >= 4

DEV bool pt_is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// the view table, passed by value in the kernel arguments (388 bytes)
struct TtaViews {
  int ch[PT_MAXK], cw[PT_MAXK];                // crop of view k
  unsigned short pr[PT_MAXK], pc[PT_MAXK];     // host bound of its tile source patch
  unsigned flip;                               // bit k: view k is mirrored
};

struct TtaGeo {                                // one view's source patch of this tile
  int ya, xa, pr, pc, ch, cw, flip;
};

template <bool LABELS, int NPP>
__global__ __launch_bounds__(256) void post_tta_kernel(const float* __restrict__ lg, int K, int T, int h, int w,
                                                       const TtaViews vw, float rK, float* __restrict__ probs,
                                                       int32_t* __restrict__ labels, float* __restrict__ score,
                                                       int H, int W, int cap, int chunks_per_z, int out_vec) {
  constexpr int TC = pt_tc(NPP);                 // classes per chunk
  constexpr int TCP = pt_tcp(TC);                // their padded LDS stride
  constexpr int VW = TC >= 4 ? 4 : TC;           // classes per LDS read
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  extern __shared__ float smem[];                // [2][cap][TCP], pr * pc elements of each used
  const int tid = threadIdx.x;
  const int ty0 = blockIdx.y * PT_ROWS, tx0 = blockIdx.x * PT_COLS;
  const int tx1 = min(tx0 + PT_COLS, W) - 1;     // last column of the tile inside the image
  const int y = ty0 + (tid >> 4), x = tx0 + ((tid & 15) << 2);
  const int64_t plane = (int64_t)h * w;
  // the class range of this workgroup (all of it for the label form)
  const int tbeg = blockIdx.z * chunks_per_z * TC;
  const int tend = min(T, tbeg + chunks_per_z * TC);
  if (tbeg >= tend) return;

  // the tile's source patch in view k: first and last tap row / column of the (mirrored) tile
  auto geo = [&](int k) {
    TtaGeo g;
    g.ch = vw.ch[k];
    g.cw = vw.cw[k];
    g.flip = (vw.flip >> k) & 1;
    const float sy = (float)g.ch / (float)H, sx = (float)g.cw / (float)W;
    const int xlo = g.flip ? W - 1 - tx1 : tx0, xhi = g.flip ? W - 1 - tx0 : tx1;
    int yb, xb, tmp;
    float lt;
    lin_idx(ty0, g.ch, sy, g.ya, tmp, lt);
    lin_idx(xlo, g.cw, sx, g.xa, tmp, lt);
    lin_idx(min(ty0 + PT_ROWS, H) - 1, g.ch, sy, tmp, yb, lt);
    lin_idx(xhi, g.cw, sx, tmp, xb, lt);
    g.pr = min(yb - g.ya + 1, (int)vw.pr[k]);
    g.pc = min(xb - g.xa + 1, (int)vw.pc[k]);
    return g;
  };

  float stage[PT_SLOTS];
  // the loads of one step: patch elements tid + 256 j of the chunk's classes in view k.  Elements past
  // the patch repeat its last one (loaded, never written to LDS); classes past T repeat class T - 1.
  auto load_step = [&](const TtaGeo& g, int k, int t0) {
    const int pp = g.pr * g.pc;
    int off[NPP];
#pragma unroll
    for (int j = 0; j < NPP; ++j) {
      const int rc = min(tid + 256 * j, pp - 1), r = rc / g.pc, c = rc - r * g.pc;
      off[j] = min(g.ya + r, g.ch - 1) * w + min(g.xa + c, g.cw - 1);
    }
    const float* src = lg + (int64_t)k * T * plane;
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      const float* s = src + (int64_t)min(t0 + tt, T - 1) * plane;
#pragma unroll
      for (int j = 0; j < NPP; ++j) stage[tt * NPP + j] = s[off[j]];
    }
  };
  auto write_step = [&](float* buf, int pp) {
#pragma unroll
    for (int j = 0; j < NPP; ++j)
      if (tid + 256 * j < pp) {
#pragma unroll
        for (int tt = 0; tt < TC; ++tt) {
          const float v = stage[tt * NPP + j];
          buf[(tid + 256 * j) * TCP + tt] = 1.f / (1.f + __expf(-v));
        }
      }
  };

  float acc[TC * 4];                             // [class of the chunk][pixel]: the sum over the views
  // one view of one chunk: v_k of this thread's 4 pixels for the TC classes of `buf`, into acc.  Pixels
  // beyond the image clamp to its last row / column (their results are not stored); the tap offsets
  // are clamped into the patch, which the host sizes to hold every tap of the tile.
  auto accumulate = [&](const float* buf, const TtaGeo& g, auto first) {
    const float sy = (float)g.ch / (float)H, sx = (float)g.cw / (float)W;
    int y0, y1, t00[4], t01[4], t10[4], t11[4];
    float ly, lx[4];
    lin_idx(min(y, H - 1), g.ch, sy, y0, y1, ly);
    const int ro0 = min(y0 - g.ya, g.pr - 1) * g.pc, ro1 = min(y1 - g.ya, g.pr - 1) * g.pc;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int xo = min(x + k, W - 1), xs = g.flip ? W - 1 - xo : xo;
      int x0, x1;
      lin_idx(xs, g.cw, sx, x0, x1, lx[k]);
      const int o0 = max(min(x0 - g.xa, g.pc - 1), 0), o1 = max(min(x1 - g.xa, g.pc - 1), 0);
      t00[k] = (ro0 + o0) * TCP;
      t01[k] = (ro0 + o1) * TCP;
      t10[k] = (ro1 + o0) * TCP;
      t11[k] = (ro1 + o1) * TCP;
    }
#pragma unroll
    for (int gI = 0; gI < TC; gI += VW) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const vec_t a = *reinterpret_cast<const vec_t*>(buf + t00[k] + gI);
        const vec_t bb = *reinterpret_cast<const vec_t*>(buf + t01[k] + gI);
        const vec_t c = *reinterpret_cast<const vec_t*>(buf + t10[k] + gI);
        const vec_t d = *reinterpret_cast<const vec_t*>(buf + t11[k] + gI);
        float v[VW];
        if constexpr (VW >= 2) {
          // two classes per packed fp32 instruction; each lane of v_pk_fma_f32 is the same IEEE fma
          // as the scalar form (post_argmax.hip)
          const f32x2 lx2 = {lx[k], lx[k]}, ly2 = {ly, ly};
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
          const float top = fmaf(lx[k], bb[0] - a[0], a[0]);
          const float bot = fmaf(lx[k], d[0] - c[0], c[0]);
          v[0] = fmaf(ly, bot - top, top);
        }
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          float& s = acc[(gI + e) * 4 + k];
          if constexpr (decltype(first)::value) s = v[e];     // s = v_0
          else s = s + v[e];                                    // s = s + v_k, in view order
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
  const bool inside = y < H && x < W;
  const int64_t o = (int64_t)y * W + x;
  const bool vec_ok = x + 3 < W && out_vec && (o & 3) == 0;
  // after the last view of a chunk: scale, then store or compare.  A last chunk that runs past T holds
  // copies of class T - 1 in the slots beyond it: never stored, and a copy never beats the original
  // under the strict compare, nor a NaN of it (the first NaN already won).
  auto finish = [&](int t0) {
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      float m[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) m[k] = acc[tt * 4 + k] * rK;
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

  TtaGeo gc = geo(0);
  load_step(gc, 0, tbeg);
  write_step(smem, gc.pr * gc.pc);
  __syncthreads();
  int cur = 0;
  for (int t0 = tbeg; t0 < tend; t0 += TC) {
    for (int k = 0; k < K; ++k) {
      const int kn = k + 1 < K ? k + 1 : 0;
      const int tn = k + 1 < K ? t0 : t0 + TC;
      const bool more = tn < tend;
      TtaGeo gn = gc;
      if (more) {                                // in flight while this step is accumulated
        gn = geo(kn);
        load_step(gn, kn, tn);
      }
      const float* buf = smem + cur * cap * TCP;
      if (k == 0) accumulate(buf, gc, std::true_type{});
      else accumulate(buf, gc, std::false_type{});
      if (k == K - 1) finish(t0);
      cur ^= 1;
      if (more) write_step(smem + cur * cap * TCP, gn.pr * gn.pc);
      __syncthreads();
      gc = gn;
    }
  }

  if constexpr (LABELS) {
    if (!inside) return;
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
}

template <bool LABELS, int NPP>
void launch_post_tta(dim3 grid, hipStream_t st, const float* logits, int K, int T, int h, int w, const TtaViews& vw,
                     float rK, float* probs, int32_t* labels, float* score, int H, int W, int cap, int chunks_per_z,
                     int out_vec) {
  const size_t lds = (size_t)2 * cap * pt_tcp(pt_tc(NPP)) * 4;
  hipLaunchKernelGGL((post_tta_kernel<LABELS, NPP>), grid, dim3(256), lds, st, logits, K, T, h, w, vw, rK, probs,
                     labels, score, H, W, cap, chunks_per_z, out_vec);
}

}  // namespace

extern "C" int catseg_postprocess_tta(const float* logits, int K, int T, int h, int w, const int32_t* views,
                                      float* probs, int32_t* labels, float* score, int H, int W, void* stream) {
  char msg[192];
  CATSEG_CHECK(logits && views, "postprocess_tta: null pointer (logits, views)");
  CATSEG_CHECK(probs || labels, "postprocess_tta: no output (probs and labels are both NULL)");
  CATSEG_CHECK(labels || !score, "postprocess_tta: score needs labels");
  CATSEG_CHECK(K >= 1 && K <= PT_MAXK, "postprocess_tta: K must be in [1, 32]");
  CATSEG_CHECK(T > 0 && H > 0 && W > 0, "postprocess_tta: T, H, W must be positive");
  CATSEG_CHECK(h > 0 && w > 0, "postprocess_tta: h, w must be positive");
  TtaViews vw = {};
  for (int k = 0; k < K; ++k) {
    const int ch = views[3 * k], cw = views[3 * k + 1], fl = views[3 * k + 2];
    if (!(ch > 0 && ch <= h && cw > 0 && cw <= w)) {
      snprintf(msg, sizeof msg, "postprocess_tta: bad crop (%d, %d) of view %d (need 0 < crop <= (h, w) = (%d, %d))",
               ch, cw, k, h, w);
      CATSEG_FAIL(msg);
    }
    if (fl != 0 && fl != 1) {
      snprintf(msg, sizeof msg, "postprocess_tta: flip of view %d is %d (need 0 or 1)", k, fl);
      CATSEG_FAIL(msg);
    }
    vw.ch[k] = ch;
    vw.cw[k] = cw;
    vw.flip |= (unsigned)fl << k;
  }
  CATSEG_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)probs % 4) == 0 && ((uintptr_t)labels % 4) == 0 &&
                   ((uintptr_t)score % 4) == 0,
               "postprocess_tta: misaligned pointer");
  const int64_t gx = ((int64_t)W + PT_COLS - 1) / PT_COLS, gy = ((int64_t)H + PT_ROWS - 1) / PT_ROWS;
  CATSEG_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535,
               "postprocess_tta: grid out of range (need ceil(H / 16) <= 65535)");
  CATSEG_CHECK((int64_t)h * w < ((int64_t)1 << 31), "postprocess_tta: source plane too large");
  // source patch of a tile, per view: the rule of catseg_postprocess_argmax (a mirrored tile is 64
  // consecutive outputs too)
  int64_t cap = 0;
  for (int k = 0; k < K; ++k) {
    const int64_t PR = std::min<int64_t>(vw.ch[k], (int64_t)(PT_ROWS - 1) * vw.ch[k] / H + 4);
    const int64_t PC = std::min<int64_t>(vw.cw[k], (int64_t)(PT_COLS - 1) * vw.cw[k] / W + 4);
    if (PR * PC > PT_CAP) {
      snprintf(msg, sizeof msg,
               "postprocess_tta: the source patch of one 16 x 64 output tile exceeds the LDS stage "
               "(4096 floats per class) in view %d: downsampling factor too large",
               k);
      CATSEG_FAIL(msg);
    }
    vw.pr[k] = (unsigned short)PR;
    vw.pc[k] = (unsigned short)PC;
    cap = std::max(cap, PR * PC);
  }
  const int npp = cap <= 256 ? 1 : cap <= 512 ? 2 : cap <= 1024 ? 4 : cap <= 2048 ? 8 : 16;
  const int tc = pt_tc(npp);
  const int chunks = (T + tc - 1) / tc;
  const float rK = 1.0f / (float)K;
  // 16-byte stores: a probability row starts at t * H * W + y * W, so W % 4 == 0 is needed there
  const int probs_vec = ((uintptr_t)probs % 16) == 0 && W % 4 == 0;
  const int labels_vec = ((uintptr_t)labels % 16) == 0 && ((uintptr_t)score % 16) == 0;
  hipStream_t st = (hipStream_t)stream;
#define PT_LAUNCH(LAB, NPP, grid, cpz)                                                                             \
  launch_post_tta<LAB, NPP>(grid, st, logits, K, T, h, w, vw, rK, probs, labels, score, H, W, (int)cap, cpz, \
                            LAB ? labels_vec : probs_vec)
#define PT_DISPATCH(LAB, grid, cpz)            \
  do {                                         \
    if (npp == 1) PT_LAUNCH(LAB, 1, grid, cpz);        \
    else if (npp == 2) PT_LAUNCH(LAB, 2, grid, cpz);   \
    else if (npp == 4) PT_LAUNCH(LAB, 4, grid, cpz);   \
    else if (npp == 8) PT_LAUNCH(LAB, 8, grid, cpz);   \
    else PT_LAUNCH(LAB, 16, grid, cpz);                \
  } while (0)
  if (probs) {
    // split the class chunks over grid z until there are about 4 workgroups per compute unit
    const int64_t tiles = gx * gy;
    const int64_t want = std::max<int64_t>(1, ((int64_t)4 * catseg_device_cus() + tiles - 1) / tiles);
    const int nz = (int)std::min<int64_t>(std::min<int64_t>(want, chunks), 65535);
    const int cpz = (chunks + nz - 1) / nz;
    const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)((chunks + cpz - 1) / cpz));
    PT_DISPATCH(false, grid, cpz);
    const int rc = catseg_launch_status("postprocess_tta");
    if (rc != CATSEG_OK) return rc;
  }
  if (labels) {
    const dim3 grid((unsigned)gx, (unsigned)gy, 1);
    PT_DISPATCH(true, grid, chunks);
    return catseg_launch_status("postprocess_tta");
  }
#undef PT_DISPATCH
#undef PT_LAUNCH
  return CATSEG_OK;
}
