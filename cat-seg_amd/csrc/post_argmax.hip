// Label-map output of the eval forward: sigmoid + bilinear resize + argmax over the classes in
// one kernel (cat_seg_model.py:222-227 followed by the evaluator's argmax,
// plain_train_net.py:107-116), without the (T, H, W) probability volume in between.
//
//   labels[b][y][x] = argmax_t v(b, t, y, x),  score[b][y][x] = max_t v(b, t, y, x)
//
// v is the value of post_tile.h, which is that of post_sep_kernel / post_band_kernel (misc.hip) for every
// shape, W % 4 != 0 included, so labels and scores equal the argmax / max of catseg_postprocess wherever
// that runs banded.
//
// One workgroup owns one output tile of one image (post_tile.h: the tile, the staging of its source patch
// in LDS and the interpolation); a thread keeps the running (best, arg) of its 4 pixels in registers while
// the workgroup walks the T class planes in chunks of TC = 16 / NPP classes (the patch is about 7 x 21
// floats per class at the 96 -> 336 headline).  Two buffers: the global loads of chunk k+1 are issued
// before chunk k is reduced and written to the other buffer after it (one barrier per chunk).
//
// The patch geometry, the tap offsets, the patch-element offsets and the final store are post_tile.h's
// pt_patch / pt_taps / pt_offsets / pt_store_labels with flip = 0, written out here: called as functions
// they leave the values alone but reschedule every instantiation (the 8 x 150 x 96^2 -> 336^2 call took 0.9 %
// longer), while this text compiles to the instructions it compiled to before the header existed.  A
// change to either copy goes into the other; tests/test_gpu_postprocess_tta.py compares the two kernels
// bit for bit at one unflipped view.
//
// NaN ranks above every number and the first NaN wins, as torch.argmax and confusion_kernel
// (evaluate.hip).
#include "common.h"
#include "capi.h"
#include "post_tile.h"

namespace {

template <bool SIG, int NPP>
__global__ __launch_bounds__(256) void post_argmax_kernel(const float* __restrict__ lg, int T, int h, int w, int ch,
                                                          int cw, int32_t* __restrict__ labels,
                                                          float* __restrict__ score, int H, int W, int PR, int PC,
                                                          int out_vec) {
  constexpr int TC = PT_SLOTS / NPP;             // classes per chunk
  constexpr int TCP = pt_tcp(TC);                // their padded LDS stride
  constexpr int VW = pt_vw(TC);                  // classes per LDS read
  extern __shared__ float smem[];                // [2][PR * PC][TCP], pr * pc elements of each used
  const int tid = threadIdx.x;
  const int b = blockIdx.z;
  const int ty0 = blockIdx.y * PT_ROWS, tx0 = blockIdx.x * PT_COLS;
  const float sy = (float)ch / (float)H, sx = (float)cw / (float)W;
  // the tile's source patch (pt_patch, flip = 0)
  int ya, xa, yb, xb, tmp;
  float lt;
  lin_idx(ty0, ch, sy, ya, tmp, lt);
  lin_idx(tx0, cw, sx, xa, tmp, lt);
  lin_idx(min(ty0 + PT_ROWS, H) - 1, ch, sy, tmp, yb, lt);
  lin_idx(min(tx0 + PT_COLS, W) - 1, cw, sx, tmp, xb, lt);
  const int pr = min(yb - ya + 1, PR), pc = min(xb - xa + 1, PC);
  const int pp = pr * pc;

  // this thread's 4 pixels: LDS offsets of their 4 taps, computed once (pt_taps, flip = 0)
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

  // this thread's patch elements, one per pass (pt_offsets)
  int off[NPP];
#pragma unroll
  for (int j = 0; j < NPP; ++j) {
    const int rc = min(tid + 256 * j, pp - 1), r = rc / pc, c = rc - r * pc;
    off[j] = min(ya + r, ch - 1) * w + min(xa + c, cw - 1);
  }
  const int64_t plane = (int64_t)h * w;
  const float* src = lg + (int64_t)b * T * plane;

  PtStage<TC, NPP> stage;
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
  auto reduce = [&](const float* buf, int t0) {
#pragma unroll 1
    for (int g = 0; g < TC; g += VW) {           // VW classes per tap read; one group in flight per trip
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float v[VW];
        pt_lerp<VW>(buf + t00[k] + g, buf + t01[k] + g, buf + t10[k] + g, buf + t11[k] + g, lx[k], ly, v);
#pragma unroll
        for (int e = 0; e < VW; ++e) {
          // strict >: the first maximum wins; NaN above every number, the first NaN wins
          const uint64_t vn = __builtin_amdgcn_ballot_w64(pt_is_nan_bits(v[e]));
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

}  // namespace

extern "C" int catseg_postprocess_argmax(const float* logits, int64_t B, int T, int h, int w, int crop_h, int crop_w,
                                         int sigmoid, int32_t* labels, float* score, int H, int W, void* stream) {
  CATSEG_CHECK(logits && labels, "postprocess_argmax: null pointer");
  CATSEG_CHECK(B > 0 && T > 0 && H > 0 && W > 0, "postprocess_argmax: B, T, H, W must be positive");
  CATSEG_CHECK(h > 0 && w > 0 && crop_h > 0 && crop_h <= h && crop_w > 0 && crop_w <= w,
               "postprocess_argmax: bad crop (need 0 < crop <= (h, w))");
  CATSEG_CHECK(((uintptr_t)logits % 4) == 0 && ((uintptr_t)labels % 4) == 0 && ((uintptr_t)score % 4) == 0,
               "postprocess_argmax: misaligned pointer");
  const int64_t gx = ((int64_t)W + PT_COLS - 1) / PT_COLS, gy = ((int64_t)H + PT_ROWS - 1) / PT_ROWS;
  CATSEG_CHECK(gx < ((int64_t)1 << 31) && gy <= 65535 && B <= 65535,
               "postprocess_argmax: grid out of range (need ceil(H / 16) <= 65535 and B <= 65535)");
  CATSEG_CHECK((int64_t)h * w < ((int64_t)1 << 31), "postprocess_argmax: source plane too large");
  const int PR = (int)pt_patch_bound(PT_ROWS, crop_h, H), PC = (int)pt_patch_bound(PT_COLS, crop_w, W);
  const int64_t pp = (int64_t)PR * PC;
  // the classes per chunk follow from the LDS stage that one class leaves: 16 at <= 256 patch
  // elements, down to 1 at 4096
  CATSEG_CHECK(pp <= PT_CAP, PT_PATCH_MSG("postprocess_argmax", ""));
  const int out_vec = ((uintptr_t)labels % 16) == 0 && ((uintptr_t)score % 16) == 0;
  const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  pt_dispatch(pt_npp(pp), [&](auto npp) {
    constexpr int NPP = decltype(npp)::value;
    const size_t lds = (size_t)2 * PR * PC * pt_tcp(PT_SLOTS / NPP) * 4;
    auto* kern = sigmoid ? post_argmax_kernel<true, NPP> : post_argmax_kernel<false, NPP>;
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, logits, T, h, w, crop_h, crop_w, labels, score, H, W, PR, PC,
                       out_vec);
  });
  return catseg_launch_status("postprocess_argmax");
}
