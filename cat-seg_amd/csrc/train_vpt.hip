// Visual prompt tuning in the training step (CLIP_FINETUNE "prompt", model_vpt.py:243-266): the
// prompt rows of the vision residual stream and their gradient.  fp32, 16-byte accesses, no atomics.
//
// The stream keeps each image's P prompt rows at the END of its sequence (CatSegEngine.vision_seq_len):
// image b holds rows b*Ls .. b*Ls + L0 - 1 = CLS + patch tokens ("body", L0 = 1 + grid^2) and rows
// b*Ls + L0 .. b*Ls + Ls - 1 = the prompts (Ls = L0 + P).  The reference inserts prompt_tokens[i] after
// CLS before block i (model_vpt.py:258-259) and every block drops them again (:215-216, :238-239);
// attention is order-free over keys, so the tail position changes no result beyond summation order.
//
//   catseg_vpt_rows_forward    expand body -> stream + write one layer's prompts into the tails,
//                              rewrite the tails in place (the per-block writer), or strip stream -> body
//   catseg_vpt_rows_backward   dprompt[p] (+)= sum_b dx[b*Ls + L0 + p] in the fixed order b = 0..B-1,
//                              then those rows of dx zeroed (the previous block's tail outputs were
//                              overwritten: they receive no gradient)
#include "common.h"
#include "capi.h"
#include "catseg_hip_train.h"

namespace {

unsigned blocks(int64_t n) { return (unsigned)((n + 255) / 256); }

// one thread per float4 of the destination.  strip: dst is the body (B*L0 rows), src the stream.
// else dst is the stream (B*Ls rows): body rows from src (skipped when src == nullptr), tail rows from
// prompt (zero when prompt == nullptr: the strip's backward).
__global__ __launch_bounds__(256) void vpt_rows_fwd_kernel(const float* __restrict__ src, int64_t ld_src,
                                                           const float* __restrict__ prompt, int64_t ld_p,
                                                           float* __restrict__ dst, int64_t ld_dst, int64_t B, int L0,
                                                           int P, int W4, int strip, int tails_only) {
  const int Ls = L0 + P;
  const int rows = strip ? L0 : (tails_only ? P : Ls);       // destination rows handled per image
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= B * rows * W4) return;
  const int c = (int)(i % W4) * 4;
  const int64_t br = i / W4, b = br / rows;
  const int r = (int)(br % rows);
  if (strip) {
    *reinterpret_cast<float4*>(dst + (b * L0 + r) * ld_dst + c) =
        *reinterpret_cast<const float4*>(src + (b * Ls + r) * ld_src + c);
    return;
  }
  const int l = tails_only ? L0 + r : r;
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (l < L0) v = *reinterpret_cast<const float4*>(src + (b * L0 + l) * ld_src + c);
  else if (prompt) v = *reinterpret_cast<const float4*>(prompt + (int64_t)(l - L0) * ld_p + c);
  *reinterpret_cast<float4*>(dst + (b * Ls + l) * ld_dst + c) = v;
}

// one thread per float4 of dprompt: the batch sum in the order b = 0..B-1, then the rows zeroed.
// Every (p, c) of dx's tails is read and written by one thread only.  dprompt == nullptr: zero only.
__global__ __launch_bounds__(256) void vpt_rows_bwd_kernel(float* __restrict__ dx, int64_t ld_dx,
                                                           float* __restrict__ dprompt, int64_t ld_dp, int64_t B,
                                                           int L0, int P, int W4, int beta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)P * W4) return;
  const int c = (int)(i % W4) * 4, p = (int)(i / W4);
  const int Ls = L0 + P;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t b = 0; b < B; ++b) {
    float4* t = reinterpret_cast<float4*>(dx + (b * Ls + L0 + p) * ld_dx + c);
    if (dprompt) { const float4 v = *t; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    *t = z;
  }
  if (!dprompt) return;
  float4* o = reinterpret_cast<float4*>(dprompt + (int64_t)p * ld_dp + c);
  if (beta) { const float4 v = *o; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
  *o = s;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// [a, a + na) and [b, b + nb) in floats
bool overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

}  // namespace

extern "C" int catseg_vpt_rows_forward(const float* src, int64_t ld_src, const float* prompt, int64_t ld_prompt,
                                       float* dst, int64_t ld_dst, int64_t B, int L0, int P, int W, int strip,
                                       void* stream) {
  CATSEG_CHECK(dst && B > 0 && L0 > 0 && P > 0 && W > 0 && W % 4 == 0, "vpt_rows_forward: bad args");
  CATSEG_CHECK(ld_dst >= W && ld_dst % 4 == 0 && aligned16(dst), "vpt_rows_forward: dst stride / alignment");
  const int64_t Ls = (int64_t)L0 + P;
  CATSEG_CHECK(B * Ls < (1LL << 30) && B * Ls * (W / 4) < (1LL << 38), "vpt_rows_forward: too many rows");
  if (strip) CATSEG_CHECK(src && !prompt, "vpt_rows_forward: strip takes src and no prompt");
  else CATSEG_CHECK(src || prompt, "vpt_rows_forward: nothing to write");
  const int64_t dst_rows = B * (strip ? L0 : Ls), src_rows = B * (strip ? Ls : L0);
  const int64_t dst_span = (dst_rows - 1) * ld_dst + W;
  if (src) {
    CATSEG_CHECK(ld_src >= W && ld_src % 4 == 0 && aligned16(src), "vpt_rows_forward: src stride / alignment");
    CATSEG_CHECK(!overlap(src, (src_rows - 1) * ld_src + W, dst, dst_span), "vpt_rows_forward: src overlaps dst");
  }
  if (prompt) {
    CATSEG_CHECK(ld_prompt >= W && ld_prompt % 4 == 0 && aligned16(prompt),
                 "vpt_rows_forward: prompt stride / alignment");
    CATSEG_CHECK(!overlap(prompt, (int64_t)(P - 1) * ld_prompt + W, dst, dst_span),
                 "vpt_rows_forward: prompt overlaps dst");
  }
  const int tails_only = !strip && !src;
  const int64_t rows = strip ? L0 : (tails_only ? P : Ls);
  hipLaunchKernelGGL(vpt_rows_fwd_kernel, dim3(blocks(B * rows * (W / 4))), dim3(256), 0, (hipStream_t)stream, src,
                     ld_src, prompt, ld_prompt, dst, ld_dst, B, L0, P, W / 4, strip, tails_only);
  return catseg_launch_status("vpt_rows_forward");
}

extern "C" int catseg_vpt_rows_backward(float* dx, int64_t ld_dx, float* dprompt, int64_t ld_dprompt, int64_t B,
                                        int L0, int P, int W, int beta, void* stream) {
  CATSEG_CHECK(dx && B > 0 && L0 > 0 && P > 0 && W > 0 && W % 4 == 0, "vpt_rows_backward: bad args");
  CATSEG_CHECK(ld_dx >= W && ld_dx % 4 == 0 && aligned16(dx), "vpt_rows_backward: dx stride / alignment");
  const int64_t Ls = (int64_t)L0 + P;
  CATSEG_CHECK(B * Ls < (1LL << 30) && (int64_t)P * (W / 4) < (1LL << 38), "vpt_rows_backward: too many rows");
  if (dprompt) {
    CATSEG_CHECK(ld_dprompt >= W && ld_dprompt % 4 == 0 && aligned16(dprompt),
                 "vpt_rows_backward: dprompt stride / alignment");
    CATSEG_CHECK(!overlap(dprompt, (int64_t)(P - 1) * ld_dprompt + W, dx, (B * Ls - 1) * ld_dx + W),
                 "vpt_rows_backward: dprompt overlaps dx");
  }
  hipLaunchKernelGGL(vpt_rows_bwd_kernel, dim3(blocks((int64_t)P * (W / 4))), dim3(256), 0, (hipStream_t)stream, dx,
                     ld_dx, dprompt, ld_dprompt, B, L0, P, W / 4, beta);
  return catseg_launch_status("vpt_rows_backward");
}
