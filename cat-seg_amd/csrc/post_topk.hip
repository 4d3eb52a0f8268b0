// Top-k label maps of the eval forward: sigmoid + bilinear resize + the K best classes of every pixel in
// one kernel, with the sum over the classes and an optional reject rule, without the (T, H, W)
// probability volume in between (include/catseg_hip_confidence.h; DESIGN.md section 4, "Confidence
// outputs").
//
//   topk_labels[b][k][y][x], topk_score[b][k][y][x] = class and value of rank k of v(b, ., y, x)
//   mass[b][y][x] = 0 + v(b, 0, y, x) + v(b, 1, y, x) + ... (fp32, class order, one add per class)
//
// v is the value of post_tile.h, so plane 0 equals catseg_postprocess_argmax's labels / score and every
// plane equals the stable descending sort of catseg_postprocess's banded output, bit for bit.
//
// The rank is a total order: a NaN above every number, a larger value first, the lower class first among
// equal values and among NaNs.  The classes arrive in class order, so a value is inserted BEHIND the
// entries it does not beat: "beats" is strict (v > s, or v a NaN and s not), and nothing beats a NaN.
//
// One workgroup owns one 16 x 64 output tile of one image and walks the T class planes in chunks through
// the double-buffered LDS stage of post_tile.h, exactly as post_argmax_kernel; a thread keeps the KK
// (value, class) pairs of its 4 pixels, sorted, and their 4 running sums in registers.  KK (1, 2 or 4)
// is the compile-time length of the list; K = 3 runs the list of 4 and stores 3 planes.  Entry j of the
// list is empty while fewer than j + 1 classes have been seen, which is the same for every thread (a
// scalar compare), so no sentinel value takes part in the order and -inf is a value like any other.
//
// A last chunk that runs past T holds copies of class T - 1 in the slots beyond it (PtStage::load).  An
// argmax can ignore them; here a copy would enter the list as the next rank and be added to the sum once
// more, so slots with t0 + g + e >= T are skipped (uniform: a scalar branch).
//
// Built with NaNs honoured and without SLP re-packing, as post_argmax.o (Makefile).  The value's last fma
// and the add into the sum are two operations: there is no product for the compiler to contract.
#include "common.h"
#include "capi.h"
#include "post_tile.h"

namespace {

constexpr int TOPK_MAX = 4;

template <bool SIG, int NPP, int KK>
__global__ __launch_bounds__(256) void post_topk_kernel(const float* __restrict__ lg, int T, int h, int w, int ch,
                                                        int cw, int K, int32_t* __restrict__ topk_labels,
                                                        float* __restrict__ topk_score, float* __restrict__ mass,
                                                        int32_t* __restrict__ labels, float min_score,
                                                        float min_margin, int reject_label, int H, int W, int PR,
                                                        int PC, int out_vec) {
  constexpr int TC = PT_SLOTS / NPP;             // classes per chunk
  constexpr int TCP = pt_tcp(TC);                // their padded LDS stride
  constexpr int VW = pt_vw(TC);                  // classes per LDS read
  extern __shared__ float smem[];                // [2][PR * PC][TCP], pr * pc elements of each used
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * PT_ROWS, tx0 = blockIdx.x * PT_COLS;
  const PtPatch gp = pt_patch(ty0, tx0, ch, cw, 0, H, W, PR, PC);
  const int pp = gp.pr * gp.pc;
  const int y = ty0 + (tid >> 4), x = tx0 + ((tid & 15) << 2);
  PtTaps tp;
  pt_taps<TCP>(gp, y, x, H, W, tp);
  int off[NPP];
  pt_offsets<NPP>(gp, tid, w, off);
  const int64_t plane = (int64_t)h * w;
  const float* src = lg + (int64_t)b * T * plane;

  PtStage<TC, NPP> stage;
  float s[4][KK], acc[4];
  int c[4][KK];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < KK; ++j) {
      s[k][j] = -INFINITY;
      c[k][j] = 0;
    }
  }

  auto reduce = [&](const float* buf, int t0) {
#pragma unroll 1
    for (int g = 0; g < TC; g += VW) {           // VW classes per tap read; one group in flight per trip
      if (t0 + g >= T) break;                    // the chunk tail: nothing but copies of class T - 1
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v[VW];
        pt_lerp<VW>(buf + tp.t00[k] + g, buf + tp.t01[k] + g, buf + tp.t10[k] + g, buf + tp.t11[k] + g, tp.lx[k],
                    tp.ly, v);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          const int t = t0 + g + e;
          if (t < T) {                           // the chunk tail inside a group
            acc[k] = acc[k] + v[e];
            const bool vn = pt_is_nan_bits(v[e]);
            bool beats[KK];
#pragma unroll
            for (int j = 0; j < KK; ++j)
              beats[j] = j >= t || (!pt_is_nan_bits(s[k][j]) && (vn || v[e] > s[k][j]));
            // beats is monotone in j (the list is sorted): entry j takes its left neighbour where v beats
            // that one too, v where it beats only entry j
#pragma unroll
            for (int j = KK - 1; j > 0; --j) {
              s[k][j] = beats[j - 1] ? s[k][j - 1] : beats[j] ? v[e] : s[k][j];
              c[k][j] = beats[j - 1] ? c[k][j - 1] : beats[j] ? t : c[k][j];
            }
            s[k][0] = beats[0] ? v[e] : s[k][0];
            c[k][0] = beats[0] ? t : c[k][0];
          }
        }
      }
    }
  };

  const int cap = PR * PC * TCP;
  stage.load(src, plane, off, 0, T);
  stage.template write<SIG>(smem, tid, pp);
  __syncthreads();
  int cur = 0;
  for (int t0 = 0; t0 < T; t0 += TC) {
    const bool more = t0 + TC < T;
    if (more) stage.load(src, plane, off, t0 + TC, T);               // in flight while this chunk is reduced
    const float* buf = smem + cur * cap;
    reduce(buf, t0);
    cur ^= 1;
    if (more) stage.template write<SIG>(smem + cur * cap, tid, pp);
    __syncthreads();
  }

  if (y >= H || x >= W) return;
  const int64_t hw = (int64_t)H * W, px = (int64_t)y * W + x;
#pragma unroll
  for (int j = 0; j < KK; ++j) {
    if (j < K) {
      const int64_t o = ((int64_t)b * K + j) * hw + px;
      const int cj[4] = {c[0][j], c[1][j], c[2][j], c[3][j]};
      const float sj[4] = {s[0][j], s[1][j], s[2][j], s[3][j]};
      pt_store_labels(topk_labels, topk_score, o, x, W, pt_vec_ok(x, W, out_vec, o), cj, sj);
    }
  }
  const int64_t o = (int64_t)b * hw + px;
  const bool vec_ok = pt_vec_ok(x, W, out_vec, o);
  if (mass) {
    if (vec_ok) {
      *reinterpret_cast<float4*>(mass + o) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) mass[o + k] = acc[k];
    }
  }
  if (labels) {
    int out[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      // both comparisons are false for a NaN: a NaN winner is kept
      bool rej = s[k][0] < min_score;
      if constexpr (KK >= 2) rej = rej || (K >= 2 && s[k][0] - s[k][1] < min_margin);
      out[k] = rej ? reject_label : c[k][0];
    }
    if (vec_ok) {
      *reinterpret_cast<int4*>(labels + o) = make_int4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (x + k < W) labels[o + k] = out[k];
    }
  }
}

template <bool SIG, int NPP>
auto topk_kernel_for(int K) {
  return K == 1 ? post_topk_kernel<SIG, NPP, 1> : K == 2 ? post_topk_kernel<SIG, NPP, 2> : post_topk_kernel<SIG, NPP, 4>;
}

}  // namespace

extern "C" int catseg_postprocess_topk(const float* logits, int64_t B, int T, int h, int w, int crop_h, int crop_w,
                                       int sigmoid, int K, int32_t* topk_labels, float* topk_score, float* mass,
                                       int32_t* labels, float min_score, float min_margin, int reject_label, int H,
                                       int W, void* stream) {
  CATSEG_CHECK(logits && topk_labels && topk_score, "postprocess_topk: null pointer");
  CATSEG_CHECK(B > 0 && T > 0 && H > 0 && W > 0, "postprocess_topk: B, T, H, W must be positive");
  CATSEG_CHECK(K >= 1 && K <= TOPK_MAX && K <= T, "postprocess_topk: K out of range (need 1 <= K <= min(4, T))");
  CATSEG_CHECK(h > 0 && w > 0 && crop_h > 0 && crop_h <= h && crop_w > 0 && crop_w <= w,
               "postprocess_topk: bad crop (need 0 < crop <= (h, w))");
  CATSEG_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)topk_labels % 4) == 0 && ((uintptr_t)topk_score % 4) == 0 &&
                   ((uintptr_t)mass % 4) == 0 && ((uintptr_t)labels % 4) == 0,
               "postprocess_topk: misaligned pointer");
  CATSEG_CHECK(!labels || reject_label >= 0, "postprocess_topk: labels needs a reject_label >= 0");
  const int64_t gx = ((int64_t)W + PT_COLS - 1) / PT_COLS, gy = ((int64_t)H + PT_ROWS - 1) / PT_ROWS;
  CATSEG_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535 && B <= 65535,
               "postprocess_topk: grid out of range (need ceil(H / 16) <= 65535 and B <= 65535)");
  CATSEG_CHECK((int64_t)h * w < ((int64_t)1 << 31), "postprocess_topk: source plane too large");
  const int PR = (int)pt_patch_bound(PT_ROWS, crop_h, H), PC = (int)pt_patch_bound(PT_COLS, crop_w, W);
  const int64_t pp = (int64_t)PR * PC;
  CATSEG_CHECK(pp <= PT_CAP, PT_PATCH_MSG("postprocess_topk", ""));
  const int out_vec = ((uintptr_t)topk_labels % 16) == 0 && ((uintptr_t)topk_score % 16) == 0 &&
                      ((uintptr_t)mass % 16) == 0 && ((uintptr_t)labels % 16) == 0;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  pt_dispatch(pt_npp(pp), [&](auto npp) {
    constexpr int NPP = decltype(npp)::value;
    const size_t lds = (size_t)2 * PR * PC * pt_tcp(PT_SLOTS / NPP) * 4;
    auto* kern = sigmoid ? topk_kernel_for<true, NPP>(K) : topk_kernel_for<false, NPP>(K);
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, logits, T, h, w, crop_h, crop_w, K, topk_labels, topk_score,
                       mass, labels, min_score, min_margin, reject_label, H, W, PR, PC, out_vec);
  });
  return catseg_launch_status("postprocess_topk");
}
