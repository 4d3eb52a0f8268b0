// Boundary-aware evaluation on the device (include/catseg_hip_boundary.h; DESIGN.md section 4, "Boundary-aware
// evaluation"): the capped Chebyshev distance of every pixel of a label map to the nearest pixel of another label
// (the outside of the map counting as one), and the counters of Boundary IoU, trimap and eroded-boundary metrics
// binned from the distance maps of a prediction and its ground truth.
//
//   distance   two passes, the logic in boundary_eval_logic.h:
//     rows     one workgroup per row: the "starts a run" bit line of the row by __ballot into LDS, then per pixel
//              the previous and the next set bit a 64-bit word at a time -> h = min(distance inside the row, cap),
//              int16, into the workspace ([H][W], dense);
//     columns  a wave per 64 columns of a row, four rows per workgroup: |dy| = 1, 2, ... reading the label and h of
//              the rows above and below until |dy| reaches the best value so far.  A pixel reads 2 (D - 1) row
//              segments (256 B of labels, 128 B of h per wave, the neighbouring waves reading the same rows), never a
//              halo sized by cap: the cost follows the distances in the map, and no cap needs another path.
//   counters   one thread per pixel over a bounded grid; when all K ((N+1)^2 + 3N) counters fit 32 KB of LDS they
//              are summed per workgroup in LDS (32-bit, H W <= 2^28 cannot overflow them) and only the nonzero ones
//              reach memory, one 64-bit atomic each; otherwise every hit is a 64-bit atomic in memory, as in
//              confusion_labels_kernel.  Integer sums: exact and independent of the order.
// No workgroup waits for another; all pixel indexing is 64-bit.
#include "common.h"
#include "capi.h"
#include "boundary_eval_logic.h"

namespace {

constexpr int BE_LDS_COUNTERS = 8192;              // 32 KB of 32-bit counters per workgroup

__global__ __launch_bounds__(256) void be_rows_kernel(const int32_t* __restrict__ labels, int W, int64_t ld,
                                                      int clamp_pred, int cap, int16_t* __restrict__ hrow) {
  __shared__ unsigned long long line[BE_ROW_WORDS];
  const int64_t y = blockIdx.x;
  const int32_t* row = labels + y * ld;
  const int words = (W + RO_WORD - 1) / RO_WORD;
  // base is a multiple of 256, so a wave covers the 64 pixels of one word; pixels >= W give 0 bits
  for (int base = 0; base < words * RO_WORD; base += 256) {
    const int x = base + (int)threadIdx.x;
    bool start = false;
    if (x < W) start = x == 0 || be_fold(row[x], clamp_pred) != be_fold(row[x - 1], clamp_pred);
    const unsigned long long m = __ballot(start);
    if ((threadIdx.x & 63) == 0 && (x >> 6) < words) line[x >> 6] = m;
  }
  __syncthreads();
  int16_t* out = hrow + y * W;
  for (int x = threadIdx.x; x < W; x += 256) out[x] = (int16_t)be_row_distance(line, W, x, cap);
}

__global__ __launch_bounds__(256) void be_columns_kernel(const int32_t* __restrict__ labels, int H, int W, int64_t ld,
                                                         int clamp_pred, const int16_t* __restrict__ hrow,
                                                         int16_t* __restrict__ dist, int64_t ld_dist) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const int32_t* lcol = labels + x;
  const int16_t* hcol = hrow + x;
  const int mine = be_fold(lcol[(int64_t)y * ld], clamp_pred);
  const int h0 = hcol[(int64_t)y * W];
  const int d = be_column_distance(y, H, h0, [&](int yy) {
    return be_fold(lcol[(int64_t)yy * ld], clamp_pred) == mine ? (int)hcol[(int64_t)yy * W] : 0;
  });
  dist[(int64_t)y * ld_dist + x] = (int16_t)d;
}

template <bool LDS>
__global__ __launch_bounds__(256) void be_counters_kernel(const int32_t* __restrict__ pred,
                                                          const int32_t* __restrict__ gt,
                                                          const int16_t* __restrict__ dist_pred,
                                                          const int16_t* __restrict__ dist_gt, int64_t HW, int N,
                                                          int ignore_label, int clamp_pred, BeWidths widths, int K,
                                                          unsigned long long* __restrict__ counters) {
  extern __shared__ unsigned int hist[];
  const int total = K * (int)be_counters_per_width(N);
  if (LDS) {
    for (int i = threadIdx.x; i < total; i += 256) hist[i] = 0u;
    __syncthreads();
  }
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
    be_count_pixel(pred[p], gt[p], dist_pred[p], dist_gt[p], N, ignore_label, clamp_pred, widths, K, [&](int i) {
      if (LDS)
        atomicAdd(hist + i, 1u);
      else
        atomicAdd(counters + i, 1ull);
    });
  }
  if (LDS) {
    __syncthreads();
    for (int i = threadIdx.x; i < total; i += 256) {
      const unsigned int v = hist[i];
      if (v) atomicAdd(counters + i, (unsigned long long)v);
    }
  }
}

bool be_side(int64_t v) { return v >= 1 && v <= BE_MAX_SIDE; }

}  // namespace

extern "C" int64_t catseg_boundary_distance_workspace(int64_t H, int64_t W, int64_t cap) {
  if (!be_side(H) || !be_side(W) || !be_side(cap)) return 0;
  return (H * W * 2 + 15) / 16 * 16;                // the row distances h, int16 [H][W]
}

extern "C" int catseg_boundary_distance(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                        int64_t cap, int16_t* dist, int64_t ld_dist, void* workspace,
                                        int64_t workspace_bytes, void* stream) {
  CATSEG_CHECK(labels && dist && workspace, "boundary_distance: null pointer");
  CATSEG_CHECK(be_side(H) && be_side(W), "boundary_distance: H and W must lie in 1 .. 16384");
  CATSEG_CHECK(be_side(cap), "boundary_distance: cap must lie in 1 .. 16384");
  CATSEG_CHECK(ld >= W && ld_dist >= W, "boundary_distance: a row stride is smaller than W");
  CATSEG_CHECK(((uintptr_t)labels % 4) == 0 && ((uintptr_t)dist % 2) == 0 && ((uintptr_t)workspace % 2) == 0,
               "boundary_distance: misaligned pointer");
  CATSEG_CHECK(workspace_bytes >= catseg_boundary_distance_workspace(H, W, cap),
               "boundary_distance: workspace smaller than catseg_boundary_distance_workspace(H, W, cap)");
  hipStream_t st = (hipStream_t)stream;
  int16_t* hrow = (int16_t*)workspace;
  hipLaunchKernelGGL(be_rows_kernel, dim3((unsigned)H), dim3(256), 0, st, labels, (int)W, ld, clamp_pred, (int)cap,
                     hrow);
  hipLaunchKernelGGL(be_columns_kernel, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), dim3(64, 4), 0, st,
                     labels, (int)H, (int)W, ld, clamp_pred, hrow, dist, ld_dist);
  return catseg_launch_status("boundary_distance");
}

extern "C" int catseg_boundary_confusion(const int32_t* pred, const int32_t* gt, const int16_t* dist_pred,
                                         const int16_t* dist_gt, int64_t H, int64_t W, int num_classes,
                                         int ignore_label, int clamp_pred, const int32_t* widths, int K,
                                         int64_t* counters, void* stream) {
  CATSEG_CHECK(pred && gt && dist_pred && dist_gt && widths && counters, "boundary_confusion: null pointer");
  CATSEG_CHECK(be_side(H) && be_side(W), "boundary_confusion: H and W must lie in 1 .. 16384");
  CATSEG_CHECK(num_classes >= 1 && num_classes <= 8192, "boundary_confusion: num_classes must lie in 1 .. 8192");
  CATSEG_CHECK(K >= 1 && K <= BE_MAX_WIDTHS, "boundary_confusion: K must lie in 1 .. 8");
  CATSEG_CHECK(((uintptr_t)counters % 8) == 0, "boundary_confusion: misaligned counters");
  BeWidths w = {};
  for (int k = 0; k < K; ++k) {
    CATSEG_CHECK(widths[k] >= 1 && widths[k] < BE_MAX_SIDE, "boundary_confusion: a width must lie in 1 .. 16383");
    w.w[k] = widths[k];
  }
  const int64_t HW = H * W, total = K * be_counters_per_width(num_classes);
  // a bounded grid: with the LDS sums a workgroup flushes once, after many pixels
  const int64_t blocks = std::min<int64_t>((HW + 255) / 256, (int64_t)std::max(1, catseg_device_cus()) * 8);
  hipStream_t st = (hipStream_t)stream;
  if (total <= BE_LDS_COUNTERS)
    hipLaunchKernelGGL(be_counters_kernel<true>, dim3((unsigned)blocks), dim3(256), (size_t)total * 4, st, pred, gt,
                       dist_pred, dist_gt, HW, num_classes, ignore_label, clamp_pred, w, K,
                       (unsigned long long*)counters);
  else
    hipLaunchKernelGGL(be_counters_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, pred, gt, dist_pred,
                       dist_gt, HW, num_classes, ignore_label, clamp_pred, w, K, (unsigned long long*)counters);
  return catseg_launch_status("boundary_confusion");
}
