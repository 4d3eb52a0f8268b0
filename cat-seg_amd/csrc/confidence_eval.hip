// Calibration counters on the device (include/catseg_hip_confidence.h; DESIGN.md section 4, "Confidence
// outputs"): per confidence bin the pixels, the correct pixels and the summed confidence in Q24, the top-k hits,
// and the valid / NaN totals of one image's top-k label maps against its ground truth.  The per-pixel logic is
// confidence_eval_logic.h.
//
// One thread per pixel over a bounded grid.  The 3 n_bins + K + 2 <= 774 counters are summed per workgroup in
// LDS (64-bit: a Q24 sum passes 2^32 after 256 pixels) and only the nonzero ones reach memory, one 64-bit atomic
// each, as be_counters_kernel (boundary_eval.hip).  Integer sums: exact and independent of the order.  No
// workgroup waits for another; all pixel indexing is 64-bit.
#include "common.h"
#include "capi.h"
#include "confidence_eval_logic.h"

namespace {

constexpr int CE_LDS_COUNTERS = 3 * CE_MAX_BINS + CE_MAX_K + 2;

__global__ __launch_bounds__(256) void ce_bins_kernel(const int32_t* __restrict__ topk_labels, int K,
                                                      const float* __restrict__ conf, const int32_t* __restrict__ gt,
                                                      int64_t HW, int N, int ignore_label, int clamp_pred, int n_bins,
                                                      unsigned long long* __restrict__ counters) {
  __shared__ unsigned long long hist[CE_LDS_COUNTERS];
  const int total = (int)ce_counters(n_bins, K);
  for (int i = threadIdx.x; i < total; i += 256) hist[i] = 0ull;
  __syncthreads();
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    int ranks[CE_MAX_K];
#pragma unroll
    for (int k = 0; k < CE_MAX_K; ++k) ranks[k] = k < K ? topk_labels[(int64_t)k * HW + p] : 0;
    ce_count_pixel(ranks, K, conf[p], gt[p], N, ignore_label, clamp_pred, n_bins,
                   [&](int i, int64_t n) { atomicAdd(hist + i, (unsigned long long)n); });
  }
  __syncthreads();
  for (int i = threadIdx.x; i < total; i += 256) {
    const unsigned long long v = hist[i];
    if (v) atomicAdd(counters + i, v);
  }
}

}  // namespace

extern "C" int catseg_confidence_bins(const int32_t* topk_labels, int K, const float* conf, const int32_t* gt,
                                      int64_t H, int64_t W, int num_classes, int ignore_label, int clamp_pred,
                                      int n_bins, int64_t* counters, void* stream) {
  CATSEG_CHECK(topk_labels && conf && gt && counters, "confidence_bins: null pointer");
  CATSEG_CHECK(H >= 1 && W >= 1 && H <= 65536 && W <= 65536, "confidence_bins: H and W must lie in 1 .. 65536");
  CATSEG_CHECK(K >= 1 && K <= CE_MAX_K, "confidence_bins: K must lie in 1 .. 4");
  CATSEG_CHECK(num_classes >= 1, "confidence_bins: num_classes must be positive");
  CATSEG_CHECK(n_bins >= 1 && n_bins <= CE_MAX_BINS, "confidence_bins: n_bins must lie in 1 .. 256");
  CATSEG_CHECK(((uintptr_t)topk_labels % 4) == 0 && ((uintptr_t)conf % 4) == 0 && ((uintptr_t)gt % 4) == 0 &&
                   ((uintptr_t)counters % 8) == 0,
               "confidence_bins: misaligned pointer");
  const int64_t HW = H * W;
  // a bounded grid: a workgroup flushes once, after many pixels
  const int64_t blocks = std::min<int64_t>((HW + 255) / 256, (int64_t)std::max(1, catseg_device_cus()) * 8);
  hipLaunchKernelGGL(ce_bins_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, topk_labels, K, conf, gt,
                     HW, num_classes, ignore_label, clamp_pred, n_bins, (unsigned long long*)counters);
  return catseg_launch_status("confidence_bins");
}
