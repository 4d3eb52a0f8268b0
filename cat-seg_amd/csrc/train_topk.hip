// Training with more classes than pad_len: the per-image top-k class selection of Aggregator.forward
// (model.py:691-725) around the training head.  The selection itself is catseg_topk_classes (misc.hip);
// here are the index and data movers it needs on both sides of the head.  fp32, memory-bound, 16-byte
// accesses where the lengths, strides and bases allow (a scalar path otherwise), no atomics: every output
// element is written by one thread, every sum runs in a fixed order (bit-reproducible).
//
//   catseg_class_inverse        classes [B][k] -> inv [B][T0]: the position of class t in image b's
//                               selection or -1 (one workgroup per image builds the row in LDS and writes
//                               all T0 entries itself: no memset + scatter, no order between two kernels)
//   catseg_class_rows_reduce    the backward of "gather rows per image" (model.py:698, :712-715 on the
//                               gathered text): out[t] (+)= sum_b d[b*k + inv[b][t]] in ascending b,
//                               read back through the inverted index; rows no image selected are 0
//   catseg_class_planes_gather  out[b][j] = in[b][classes[b][j]]: the k selected cost planes
//                               (model.py:702), and the backward of the final scatter
//   catseg_class_planes_scatter out[b][t] = inv[b][t] >= 0 ? in[b][inv[b][t]] : fill: the -100 fill and
//                               the scatter of model.py:722-723 in one pass over the output
#include "common.h"
#include "capi.h"
#include "catseg_hip_train.h"

namespace {

constexpr int TOPK_MAX_T = 2048;        // the limit of catseg_topk_classes
constexpr int PLANE_CHUNK = 4096;       // floats of one plane per workgroup step: 256 lanes x 4 x float4

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

unsigned grid_of(int64_t items, int64_t cap = 1 << 20) { return (unsigned)(items < cap ? items : cap); }

// One workgroup per image.  A class id outside [0, T0) is skipped; of a duplicated id one position stays.
__global__ __launch_bounds__(256) void class_inverse_kernel(const int32_t* __restrict__ classes, int64_t B, int k,
                                                            int T0, int32_t* __restrict__ inv) {
  __shared__ int32_t row[TOPK_MAX_T];
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    for (int t = threadIdx.x; t < T0; t += 256) row[t] = -1;
    __syncthreads();
    for (int j = threadIdx.x; j < k; j += 256) {
      const int32_t c = classes[b * k + j];
      if (c >= 0 && c < T0) row[c] = j;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T0; t += 256) inv[b * T0 + t] = row[t];
    __syncthreads();
  }
}

// One thread per V floats of a destination row: the images' contributions in ascending b.  A position
// outside [0, k) counts as "not selected".  beta with no contribution leaves the element as it is.
template <int V>
__global__ __launch_bounds__(256) void class_rows_reduce_kernel(const float* __restrict__ d, int64_t ld_d,
                                                                const int32_t* __restrict__ inv, int64_t B, int k,
                                                                int T0, int64_t colsV, float* __restrict__ out,
                                                                int64_t ld_out, int beta) {
  const int64_t total = (int64_t)T0 * colsV;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t t = i / colsV, c = (i % colsV) * V;
    float s[V];
#pragma unroll
    for (int v = 0; v < V; ++v) s[v] = 0.f;
    int n = 0;
    for (int64_t b = 0; b < B; ++b) {
      const int32_t j = inv[b * T0 + t];
      if (j < 0 || j >= k) continue;
      const float* src = d + (b * k + j) * ld_d + c;
      if (V == 4) {
        const float4 x = *reinterpret_cast<const float4*>(src);
        s[0] += x.x; s[1] += x.y; s[2] += x.z; s[3] += x.w;
      } else {
        s[0] += src[0];
      }
      ++n;
    }
    if (beta && !n) continue;
    float* o = out + t * ld_out + c;
    if (V == 4) {
      float4 r = make_float4(s[0], s[1], s[2], s[3]);
      if (beta) { const float4 x = *reinterpret_cast<const float4*>(o); r.x = x.x + r.x; r.y = x.y + r.y; r.z = x.z + r.z; r.w = x.w + r.w; }
      *reinterpret_cast<float4*>(o) = r;
    } else {
      o[0] = beta ? o[0] + s[0] : s[0];
    }
  }
}

// out[b][t][p] = in[b][idx[b*n_out + t]][p] for an index in [0, n_in), else fill.  One workgroup step =
// PLANE_CHUNK floats of one output plane; the four loads of a lane are issued before its stores.
template <bool VEC>
__global__ __launch_bounds__(256) void class_planes_kernel(const float* __restrict__ in, int64_t in_t_stride,
                                                           int64_t in_b_stride, const int32_t* __restrict__ idx,
                                                           int64_t B, int n_out, int n_in, int64_t P,
                                                           float* __restrict__ out, int64_t out_t_stride,
                                                           int64_t out_b_stride, float fill) {
  const int64_t chunks = (P + PLANE_CHUNK - 1) / PLANE_CHUNK;
  const int64_t work = B * n_out * chunks;
  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int64_t plane = w / chunks, p0 = (w % chunks) * PLANE_CHUNK;
    const int64_t b = plane / n_out, t = plane % n_out;
    const int32_t s = idx[plane];
    const bool have = s >= 0 && s < n_in;
    const float* src = in + b * in_b_stride + (have ? s : 0) * in_t_stride;
    float* dst = out + b * out_b_stride + t * out_t_stride;
    if (VEC) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t p = p0 + (u * 256 + threadIdx.x) * 4;
        v[u] = make_float4(fill, fill, fill, fill);
        if (have && p < P) v[u] = *reinterpret_cast<const float4*>(src + p);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int64_t p = p0 + (u * 256 + threadIdx.x) * 4;
        if (p < P) *reinterpret_cast<float4*>(dst + p) = v[u];
      }
    } else {
      const int64_t p1 = p0 + PLANE_CHUNK < P ? p0 + PLANE_CHUNK : P;
      for (int64_t p = p0 + threadIdx.x; p < p1; p += 256) dst[p] = have ? src[p] : fill;
    }
  }
}

// [a, a + na) and [b, b + nb) in floats
bool overlap(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

int planes_launch(const char* what, const float* in, int64_t in_t_stride, int64_t in_b_stride, const int32_t* idx,
                  int64_t B, int n_out, int n_in, int64_t P, float* out, int64_t out_t_stride, int64_t out_b_stride,
                  float fill, void* stream) {
  CATSEG_CHECK(in_t_stride >= P && out_t_stride >= P, "class_planes: a plane stride is below the plane length");
  CATSEG_CHECK(in_b_stride >= (int64_t)(n_in - 1) * in_t_stride + P &&
                   out_b_stride >= (int64_t)(n_out - 1) * out_t_stride + P,
               "class_planes: an image stride is below the image's planes");
  CATSEG_CHECK(B * n_out < (1LL << 40) && P < (1LL << 40), "class_planes: too many planes");
  CATSEG_CHECK(!overlap(in, (B - 1) * in_b_stride + (int64_t)(n_in - 1) * in_t_stride + P, out,
                        (B - 1) * out_b_stride + (int64_t)(n_out - 1) * out_t_stride + P),
               "class_planes: in overlaps out");
  const bool vec = P % 4 == 0 && in_t_stride % 4 == 0 && in_b_stride % 4 == 0 && out_t_stride % 4 == 0 &&
                   out_b_stride % 4 == 0 && aligned16(in) && aligned16(out);
  const int64_t work = B * n_out * ((P + PLANE_CHUNK - 1) / PLANE_CHUNK);
  if (vec)
    hipLaunchKernelGGL(class_planes_kernel<true>, dim3(grid_of(work)), dim3(256), 0, (hipStream_t)stream, in,
                       in_t_stride, in_b_stride, idx, B, n_out, n_in, P, out, out_t_stride, out_b_stride, fill);
  else
    hipLaunchKernelGGL(class_planes_kernel<false>, dim3(grid_of(work)), dim3(256), 0, (hipStream_t)stream, in,
                       in_t_stride, in_b_stride, idx, B, n_out, n_in, P, out, out_t_stride, out_b_stride, fill);
  return catseg_launch_status(what);
}

}  // namespace

#define TOPK_SIZES_CHECK(what)                                                                  \
  CATSEG_CHECK(B > 0 && k > 0 && T0 > 0, what ": non-positive size");                           \
  CATSEG_CHECK(k <= T0 && T0 <= TOPK_MAX_T, what ": need k <= T0 <= 2048")

extern "C" int catseg_class_inverse(const int32_t* classes, int64_t B, int k, int T0, int32_t* inv, void* stream) {
  CATSEG_CHECK(classes && inv, "class_inverse: null pointer");
  TOPK_SIZES_CHECK("class_inverse");
  hipLaunchKernelGGL(class_inverse_kernel, dim3(grid_of(B, 65535)), dim3(256), 0, (hipStream_t)stream, classes, B, k,
                     T0, inv);
  return catseg_launch_status("class_inverse");
}

extern "C" int catseg_class_rows_reduce(const float* d, int64_t ld_d, const int32_t* inv, int64_t B, int k, int T0,
                                        int64_t cols, float* out, int64_t ld_out, int beta, void* stream) {
  CATSEG_CHECK(d && inv && out, "class_rows_reduce: null pointer");
  TOPK_SIZES_CHECK("class_rows_reduce");
  CATSEG_CHECK(cols > 0 && ld_d >= cols && ld_out >= cols, "class_rows_reduce: bad cols / row strides");
  CATSEG_CHECK(B * k < (1LL << 40) && cols < (1LL << 31), "class_rows_reduce: too many rows");
  CATSEG_CHECK(!overlap(d, (B * k - 1) * ld_d + cols, out, (int64_t)(T0 - 1) * ld_out + cols),
               "class_rows_reduce: d overlaps out");
  const bool vec = cols % 4 == 0 && ld_d % 4 == 0 && ld_out % 4 == 0 && aligned16(d) && aligned16(out);
  if (vec)
    hipLaunchKernelGGL(class_rows_reduce_kernel<4>, dim3(grid_of((T0 * (cols / 4) + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d, ld_d, inv, B, k, T0, cols / 4, out, ld_out, beta);
  else
    hipLaunchKernelGGL(class_rows_reduce_kernel<1>, dim3(grid_of((T0 * cols + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, d, ld_d, inv, B, k, T0, cols, out, ld_out, beta);
  return catseg_launch_status("class_rows_reduce");
}

extern "C" int catseg_class_planes_gather(const float* in, int64_t in_t_stride, int64_t in_b_stride,
                                          const int32_t* classes, int64_t B, int k, int T0, int64_t P, float* out,
                                          int64_t out_t_stride, int64_t out_b_stride, void* stream) {
  CATSEG_CHECK(in && classes && out, "class_planes_gather: null pointer");
  TOPK_SIZES_CHECK("class_planes_gather");
  CATSEG_CHECK(P > 0, "class_planes_gather: non-positive size");
  return planes_launch("class_planes_gather", in, in_t_stride, in_b_stride, classes, B, k, T0, P, out, out_t_stride,
                       out_b_stride, 0.f, stream);
}

extern "C" int catseg_class_planes_scatter(const float* in, int64_t in_t_stride, int64_t in_b_stride,
                                           const int32_t* inv, int64_t B, int k, int T0, int64_t P, float fill,
                                           float* out, int64_t out_t_stride, int64_t out_b_stride, void* stream) {
  CATSEG_CHECK(in && inv && out, "class_planes_scatter: null pointer");
  TOPK_SIZES_CHECK("class_planes_scatter");
  CATSEG_CHECK(P > 0, "class_planes_scatter: non-positive size");
  return planes_launch("class_planes_scatter", in, in_t_stride, in_b_stride, inv, B, T0, k, P, out, out_t_stride,
                       out_b_stride, fill, stream);
}
