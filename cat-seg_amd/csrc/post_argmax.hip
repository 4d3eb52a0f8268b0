// Label-map output of the eval forward: sigmoid + bilinear resize + argmax over the classes in
// one kernel (cat_seg_model.py:222-227 followed by the evaluator's argmax,
// plain_train_net.py:107-116), without the (T, H, W) probability volume in between.
//
//   labels[b][y][x] = argmax_t v(b, t, y, x),  score[b][y][x] = max_t v(b, t, y, x)
//
// v is formed exactly as post_sep_kernel / post_band_kernel (misc.hip) form it -- lin_idx taps,
// sigmoid = 1 / (1 + __expf(-logit)) on the SOURCE logit, top = fma(lx, r0[x1] - r0[x0], r0[x0]),
// bot likewise, fma(ly, bot - top, top) -- for every shape, W % 4 != 0 included, so labels and
// scores equal the argmax / max of catseg_postprocess wherever that runs banded.
//
// One workgroup owns one PA_ROWS x PA_COLS output tile of one image; a thread owns 4 consecutive
// pixels of a row and keeps their running (best, arg) in registers while the workgroup walks the
// T class planes.  The tile's source patch (pr x pc floats per class; about 7 x 21 at the 96 -> 336
// headline) is staged in LDS for a chunk of TC classes at a time, sigmoid applied once per source
// logit as it is written.  Two buffers: the global loads of chunk k+1 are issued before chunk k is
// reduced and written to the other buffer after it (one barrier per chunk).
//
// A thread stages PA_SLOTS = NPP * TC floats per chunk: patch elements tid + 256 j (j < NPP, NPP
// the compile-time number of 256-element passes over the patch) of TC classes, so every slot's
// class and LDS offset are compile-time and no index is divided in the loop.  LDS keeps the
// chunk's classes innermost, [patch element][TCP], so the 4 taps of a pixel are read for 4
// classes at a time (ds_read_b128 at TC >= 4: twice the LDS bytes per clock of scalar reads) at
// immediate offsets; TCP pads TC to 4 * odd floats, which spreads neighbouring patch elements over
// the 16-byte LDS slots.
//
// Built with NaNs honoured (Makefile): NaN ranks above every number and the first NaN wins, as
// torch.argmax and confusion_kernel (evaluate.hip); NaN is tested on the bits as there.
#include "common.h"
#include "capi.h"
#include "resize_idx.h"

namespace {

constexpr int PA_ROWS = 16, PA_COLS = 64;      // output tile: 256 threads x 4 pixels of a row
constexpr int PA_SLOTS = 16;                   // staged floats per thread and chunk
constexpr int PA_CAP = PA_SLOTS * 256;         // largest source patch of one class, floats

constexpr int pa_tcp(int tc) { return tc == 16 ? 20 : tc == 8 ? 12 : tc; }   // 4 * odd at TC >= 4

DEV bool is_nan_bits(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

template <bool SIG, int NPP>
__global__ __launch_bounds__(256) void post_argmax_kernel(const float* __restrict__ lg, int T, int h, int w, int ch,
                                                          int cw, int32_t* __restrict__ labels,
                                                          float* __restrict__ score, int H, int W, int PR, int PC,
                                                          int out_vec) {
  constexpr int TC = PA_SLOTS / NPP;             // classes per chunk
  constexpr int TCP = pa_tcp(TC);                // their padded LDS stride
  constexpr int VW = TC >= 4 ? 4 : TC;           // classes per LDS read
  typedef float vec_t __attribute__((ext_vector_type(VW)));
  extern __shared__ float smem[];                // [2][PR * PC][TCP], pr * pc elements of each used
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * PA_ROWS, tx0 = blockIdx.x * PA_COLS;
  const float sy = (float)ch / (float)H, sx = (float)cw / (float)W;
  // the tile's source patch: first and last tap row / column (the taps are non-decreasing in the
  // output index).  pr x pc is what is staged; the host's PR x PC bounds it and sizes the buffers.
  int ya, xa, yb, xb, tmp;
  float lt;
  lin_idx(ty0, ch, sy, ya, tmp, lt);
  lin_idx(tx0, cw, sx, xa, tmp, lt);
  lin_idx(min(ty0 + PA_ROWS, H) - 1, ch, sy, tmp, yb, lt);
  lin_idx(min(tx0 + PA_COLS, W) - 1, cw, sx, tmp, xb, lt);
  const int pr = min(yb - ya + 1, PR), pc = min(xb - xa + 1, PC);
  const int pp = pr * pc;

  // this thread's 4 pixels: LDS offsets of their 4 taps, computed once.  Pixels beyond the image
  // clamp to its last row / column (their results are not stored); the offsets are clamped into
  // the patch, which the host sizes to hold every tap of the tile.
  const int y = ty0 + (tid >> 4), x = tx0 + ((tid & 15) << 2);
  int y0, y1, t00[4], t01[4], t10[4], t11[4];
  float ly, lx[4];
  lin_idx(min(y, H - 1), ch, sy, y0, y1, ly);
  const int ro0 = min(y0 - ya, pr - 1) * pc, ro1 = min(y1 - ya, pr - 1) * pc;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    int x0, x1;
    lin_idx(min(x + k, W - 1), cw, sx, x0, x1, lx[k]);
    const int o0 = min(x0 - xa, pc - 1), o1 = min(x1 - xa, pc - 1);
    t00[k] = (ro0 + o0) * TCP;
    t01[k] = (ro0 + o1) * TCP;
    t10[k] = (ro1 + o0) * TCP;
    t11[k] = (ro1 + o1) * TCP;
  }

  // this thread's patch elements (one per pass): source offset inside a class plane.  Elements past
  // the patch repeat its last one (loaded, never written to LDS).
  int off[NPP];
#pragma unroll
  for (int j = 0; j < NPP; ++j) {
    const int rc = min(tid + 256 * j, pp - 1), r = rc / pc, c = rc - r * pc;
    off[j] = min(ya + r, ch - 1) * w + min(xa + c, cw - 1);
  }
  const int64_t plane = (int64_t)h * w;
  const float* src = lg + (int64_t)b * T * plane;

  float stage[PA_SLOTS];
  auto load_chunk = [&](int t0) {                // classes past T repeat class T - 1
#pragma unroll
    for (int tt = 0; tt < TC; ++tt) {
      const float* s = src + (int64_t)min(t0 + tt, T - 1) * plane;
#pragma unroll
      for (int j = 0; j < NPP; ++j) stage[tt * NPP + j] = s[off[j]];
    }
  };
  auto write_chunk = [&](float* buf) {
#pragma unroll
    for (int j = 0; j < NPP; ++j)
      if (tid + 256 * j < pp) {
#pragma unroll
        for (int tt = 0; tt < TC; ++tt) {
          const float v = stage[tt * NPP + j];
          buf[(tid + 256 * j) * TCP + tt] = SIG ? 1.f / (1.f + __expf(-v)) : v;
        }
      }
  };

  float best[4];
  int arg[4];
  // "this pixel's best is a NaN" as one wave mask per pixel slot (a lane's bit), so the rule costs
  // scalar mask operations, not vector ones
  uint64_t bnan[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    best[k] = -INFINITY;
    arg[k] = 0;
    bnan[k] = 0;
  }
  // the TC classes of one buffer.  A last chunk that runs past T holds copies of class T - 1 in the
  // slots beyond it (load_chunk): a copy never beats the original under the strict compare, nor a
  // NaN of it (the first NaN already won), so the tail needs no guard.
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  auto reduce = [&](const float* buf, int t0) {
#pragma unroll 1
    for (int g = 0; g < TC; g += VW) {           // VW classes per tap read; one group in flight per trip
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const vec_t a = *reinterpret_cast<const vec_t*>(buf + t00[k] + g);
        const vec_t bb = *reinterpret_cast<const vec_t*>(buf + t01[k] + g);
        const vec_t c = *reinterpret_cast<const vec_t*>(buf + t10[k] + g);
        const vec_t d = *reinterpret_cast<const vec_t*>(buf + t11[k] + g);
        float v[VW];
        if constexpr (VW >= 2) {
          // two classes per packed fp32 instruction (the pairs are register pairs of the reads);
          // each lane of v_pk_fma_f32 is the same IEEE fma as the scalar form
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
          // strict >: the first maximum wins; NaN above every number, the first NaN wins
          const uint64_t vn = __builtin_amdgcn_ballot_w64(is_nan_bits(v[e]));
          const uint64_t gt = __builtin_amdgcn_ballot_w64(v[e] > best[k]);
          const uint64_t take_m = (vn | gt) & ~bnan[k];
          bnan[k] |= take_m & vn;
          const bool take = __builtin_amdgcn_inverse_ballot_w64(take_m);
          best[k] = take ? v[e] : best[k];
          arg[k] = take ? t0 + g + e : arg[k];
        }
      }
    }
  };

  const int cap = PR * PC * TCP;
  load_chunk(0);
  write_chunk(smem);
  __syncthreads();
  int cur = 0;
  for (int t0 = 0; t0 < T; t0 += TC) {
    const bool more = t0 + TC < T;
    if (more) load_chunk(t0 + TC);               // in flight while this chunk is reduced
    const float* buf = smem + cur * cap;
    reduce(buf, t0);
    cur ^= 1;
    if (more) write_chunk(smem + cur * cap);
    __syncthreads();
  }

  if (y >= H || x >= W) return;
  const int64_t o = ((int64_t)b * H + y) * W + x;
  if (x + 3 < W && out_vec && (o & 3) == 0) {
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

template <bool SIG, int NPP>
void launch_post_argmax(dim3 grid, hipStream_t st, const float* logits, int T, int h, int w, int ch, int cw,
                        int32_t* labels, float* score, int H, int W, int PR, int PC, int out_vec) {
  const size_t lds = (size_t)2 * PR * PC * pa_tcp(PA_SLOTS / NPP) * 4;
  hipLaunchKernelGGL((post_argmax_kernel<SIG, NPP>), grid, dim3(256), lds, st, logits, T, h, w, ch, cw, labels, score,
                     H, W, PR, PC, out_vec);
}

}  // namespace

extern "C" int catseg_postprocess_argmax(const float* logits, int64_t B, int T, int h, int w, int crop_h, int crop_w,
                                         int sigmoid, int32_t* labels, float* score, int H, int W, void* stream) {
  CATSEG_CHECK(logits && labels, "postprocess_argmax: null pointer");
  CATSEG_CHECK(B > 0 && T > 0 && H > 0 && W > 0, "postprocess_argmax: B, T, H, W must be positive");
  CATSEG_CHECK(h > 0 && w > 0 && crop_h > 0 && crop_h <= h && crop_w > 0 && crop_w <= w,
               "postprocess_argmax: bad crop (need 0 < crop <= (h, w))");
  CATSEG_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)labels % 4) == 0 && ((uintptr_t)score % 4) == 0,
               "postprocess_argmax: misaligned pointer");
  const int64_t gx = ((int64_t)W + PA_COLS - 1) / PA_COLS, gy = ((int64_t)H + PA_ROWS - 1) / PA_ROWS;
  CATSEG_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535 && B <= 65535,
               "postprocess_argmax: grid out of range (need ceil(H / 16) <= 65535 and B <= 65535)");
  CATSEG_CHECK((int64_t)h * w < ((int64_t)1 << 31), "postprocess_argmax: source plane too large");
  // source patch of a tile: n consecutive outputs span at most floor(scale * (n - 1)) + 2 source
  // indices beyond the first (i0 spread + the i1 tap); one more for the rounding of the fp32 taps
  const int PR = (int)std::min<int64_t>(crop_h, (int64_t)(PA_ROWS - 1) * crop_h / H + 4);
  const int PC = (int)std::min<int64_t>(crop_w, (int64_t)(PA_COLS - 1) * crop_w / W + 4);
  const int64_t pp = (int64_t)PR * PC;
  // the classes per chunk follow from the LDS stage that one class leaves: 16 at <= 256 patch
  // elements, down to 1 at 4096; beyond that not even one class fits
  CATSEG_CHECK(pp <= PA_CAP,
               "postprocess_argmax: the source patch of one 16 x 64 output tile exceeds the LDS stage "
               "(4096 floats per class): downsampling factor too large");
  const int out_vec = ((uintptr_t)labels % 16) == 0 && ((uintptr_t)score % 16) == 0;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
#define PA_LAUNCH(NPP)                                                                                              \
  (sigmoid ? launch_post_argmax<true, NPP>(grid, st, logits, T, h, w, crop_h, crop_w, labels, score, H, W, PR, PC,  \
                                           out_vec)                                                                 \
           : launch_post_argmax<false, NPP>(grid, st, logits, T, h, w, crop_h, crop_w, labels, score, H, W, PR, PC, \
                                            out_vec))
  if (pp <= 256) PA_LAUNCH(1);
  else if (pp <= 512) PA_LAUNCH(2);
  else if (pp <= 1024) PA_LAUNCH(4);
  else if (pp <= 2048) PA_LAUNCH(8);
  else PA_LAUNCH(16);
#undef PA_LAUNCH
  return catseg_launch_status("postprocess_argmax");
}
