// Deterministic exclusive scan of int32 counts in device memory, shared by the kernels that compact by
// "count, scan, write" (label_runs.hip: run starts per column segment; label_regions.hip: region roots per
// 64 pixels): block sums, one block over the block sums, block scans.  Three launches on the stream, no
// atomics and no inter-block waiting, so the offsets follow the index order of the counts.
#pragma once
#include "common.h"

namespace {

constexpr int LR_PER_THREAD = 8;
constexpr int LR_SCAN = 256 * LR_PER_THREAD;      // counts per block of the scan passes

// exclusive scan of one value per thread over the 256 threads of a block; total = the block's sum
DEV int lr_block_exscan(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) sh[wv] = inc;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = sh[i];
    base += i < wv ? s : 0;
    total += s;
  }
  __syncthreads();                                 // sh may be written again
  return base + inc - v;
}

// bsum[b] = the sum of counts [b * LR_SCAN, (b + 1) * LR_SCAN)
__global__ __launch_bounds__(256) void lr_block_sums_kernel(const int32_t* __restrict__ counts, int64_t n,
                                                            int32_t* __restrict__ bsum) {
  __shared__ int sh[4];
  const int64_t base = (int64_t)blockIdx.x * LR_SCAN;
  int v = 0;
#pragma unroll
  for (int j = 0; j < LR_PER_THREAD; ++j) {
    const int64_t i = base + j * 256 + threadIdx.x;
    v += i < n ? counts[i] : 0;
  }
  int total;
  lr_block_exscan(v, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one block: bsum -> its exclusive scan, in strips of 256 with a carry; *total = the sum of all of it
__global__ __launch_bounds__(256) void lr_scan_top_kernel(int32_t* __restrict__ bsum, int64_t nb,
                                                          int32_t* __restrict__ total_out) {
  __shared__ int sh[4];
  int carry = 0;
  for (int64_t base = 0; base < nb; base += 256) {
    const int64_t i = base + threadIdx.x;
    const int v = i < nb ? bsum[i] : 0;
    int total;
    const int ex = lr_block_exscan(v, sh, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) total_out[0] = carry;
}

// counts -> offsets in place: a thread owns LR_PER_THREAD consecutive counts of its block's range
__global__ __launch_bounds__(256) void lr_scan_apply_kernel(int32_t* __restrict__ counts, int64_t n,
                                                            const int32_t* __restrict__ bsum) {
  __shared__ int sh[4];
  const int64_t first = (int64_t)blockIdx.x * LR_SCAN + (int64_t)threadIdx.x * LR_PER_THREAD;
  int c[LR_PER_THREAD];
  int v = 0;
#pragma unroll
  for (int j = 0; j < LR_PER_THREAD; ++j) {
    c[j] = first + j < n ? counts[first + j] : 0;
    v += c[j];
  }
  int total;
  int run = bsum[blockIdx.x] + lr_block_exscan(v, sh, total);
#pragma unroll
  for (int j = 0; j < LR_PER_THREAD; ++j) {
    if (first + j < n) counts[first + j] = run;
    run += c[j];
  }
}

// counts[0, n) -> their exclusive scan in place, *total = their sum; bsum: ceil(n / LR_SCAN) ints
inline void lr_scan_launch(int32_t* counts, int64_t n, int32_t* bsum, int32_t* total, hipStream_t st) {
  const int64_t nb = (n + LR_SCAN - 1) / LR_SCAN;
  hipLaunchKernelGGL(lr_block_sums_kernel, dim3((unsigned)nb), dim3(256), 0, st, counts, n, bsum);
  hipLaunchKernelGGL(lr_scan_top_kernel, dim3(1), dim3(256), 0, st, bsum, nb, total);
  hipLaunchKernelGGL(lr_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, st, counts, n, bsum);
}

}  // namespace
