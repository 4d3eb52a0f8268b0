// Training input on the device: the reference's training mapper
// (cat_seg/data/dataset_mappers/mask_former_semantic_dataset_mapper.py:62-147) for a whole batch of decoded
// uint8 images, byte for byte what the host composition computes (cat_seg/data/train_input.py
// reference_apply = transforms.py with the random draws pinned).
//
//   catseg_train_crop_select  RandomCrop_CategoryAreaConstraint's candidate rule: one workgroup per
//                             (image, candidate) counts the window's labels of the nearest-resized label map
//                             (read through the index tables from the source labels) into an LDS histogram
//                             with integer atomics; the last workgroup of an image to finish (a counter)
//                             takes the first passing candidate, else the last one
//   catseg_train_augment      grid (output tiles, B): per 64 x 16 tile of the padded canvas the horizontal
//                             resampling pass of the source rows the tile needs goes into LDS as uint8, in
//                             chunks of 32 source rows (any downscale factor: the tap counts are loop bounds
//                             read from the tables); each lane owns 4 neighbouring output pixels, accumulates
//                             their vertical pass from LDS, applies the colour record and stores 4 pixels
//                             per 32-bit store (scalar when S % 4 != 0).  No atomics, one writer per byte.
//
// The resampling is PIL's (Resample.c, 8 bits per channel): int32 coefficients with 22 fraction bits,
// clip8((sum + 2^21) >> 22) per pass, the horizontal pass first and rounded to uint8.  The colour math is
// float32 in numpy's operation order (train_color.h); this file is built with -ffp-contract=off (Makefile)
// and says so again below, so no a * b + c here becomes an fma.
#pragma clang fp contract(off)
#include "common.h"
#include "capi.h"
#include "catseg_hip_train.h"
#include "train_color.h"

static_assert(sizeof(CatsegTrainImageDesc) == 128, "CatsegTrainImageDesc is mirrored as a 128-byte numpy record");

namespace {

constexpr int TW = 64, TH = 16;       // output tile: 16 lanes x 4 pixels wide, 16 rows (256 lanes)
constexpr int ROWS = 32;              // source rows of the horizontal pass held in LDS at a time
constexpr int MAX_LABELS = 4096;      // LDS histogram bins of the crop selection
constexpr int PREC = 22;              // PIL's PRECISION_BITS

__device__ inline int clip8(int v) {
  v >>= PREC;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__device__ inline int load_label(const uint8_t* lab, int lab_bytes, int64_t i) {
  return lab_bytes == 1 ? (int)lab[i] : reinterpret_cast<const int32_t*>(lab)[i];
}

// ---------------------------------------------------------------------------------------------------------
// crop selection
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crop_select_kernel(const uint8_t* __restrict__ src,
                                                          const int32_t* __restrict__ tab,
                                                          const CatsegTrainImageDesc* __restrict__ descs,
                                                          const int32_t* __restrict__ cands, int n_cand, int n_labels,
                                                          int ignore_label, double max_area, int32_t* flags,
                                                          int32_t* counters, int32_t* __restrict__ crops) {
  __shared__ unsigned hist[MAX_LABELS];
  __shared__ unsigned red[3][4];
  const int c = blockIdx.x, b = blockIdx.y;
  const CatsegTrainImageDesc& d = descs[b];
  const int32_t* cand = cands + ((int64_t)b * n_cand + c) * 4;
  const int y0 = cand[0], x0 = cand[1], ch = cand[2], cw = cand[3];
  const int w = d.w, lab_bytes = d.lab_bytes;
  const uint8_t* lab = src + d.lab_off;
  const int32_t* nx = tab + d.nx_off;
  const int32_t* ny = tab + d.ny_off;
  for (int i = threadIdx.x; i < n_labels; i += 256) hist[i] = 0;
  __syncthreads();
  // 4 window rows per pass of the workgroup, a 64-lane wave along x
  for (int y = threadIdx.x >> 6; y < ch; y += 4) {
    const int64_t row = (int64_t)ny[y0 + y] * w;
    for (int x = threadIdx.x & 63; x < cw; x += 64) {
      const int v = load_label(lab, lab_bytes, row + nx[x0 + x]);
      if (v != ignore_label && v >= 0 && v < n_labels) atomicAdd(&hist[v], 1u);
    }
  }
  __syncthreads();
  unsigned nz = 0, mx = 0, sum = 0;
  for (int i = threadIdx.x; i < n_labels; i += 256) {
    const unsigned h = hist[i];
    nz += h != 0;
    mx = h > mx ? h : mx;
    sum += h;
  }
  for (int o = 32; o > 0; o >>= 1) {
    nz += __shfl_down(nz, o);
    const unsigned m2 = __shfl_down(mx, o);
    mx = m2 > mx ? m2 : mx;
    sum += __shfl_down(sum, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = nz;
    red[1][threadIdx.x >> 6] = mx;
    red[2][threadIdx.x >> 6] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    nz = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    sum = red[2][0] + red[2][1] + red[2][2] + red[2][3];
    mx = red[1][0];
    for (int k = 1; k < 4; ++k) mx = red[1][k] > mx ? red[1][k] : mx;
    // the host's float64 comparison: len(cnt) > 1 and max(cnt) < sum(cnt) * max_area
    const int pass = nz > 1 && (double)mx < (double)sum * max_area;
    __hip_atomic_store(&flags[(int64_t)b * n_cand + c], pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __threadfence();
    const int done = atomicAdd(&counters[b], 1);
    if (done == n_cand - 1) {
      // the last workgroup of this image: every flag is visible (fence before each increment)
      __threadfence();
      int pick = n_cand - 1;
      for (int k = n_cand - 1; k >= 0; --k)
        if (__hip_atomic_load(&flags[(int64_t)b * n_cand + k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) pick = k;
      const int32_t* win = cands + ((int64_t)b * n_cand + pick) * 4;
      for (int k = 0; k < 4; ++k) crops[b * 4 + k] = win[k];
      __hip_atomic_store(&counters[b], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// resize + crop + colour + flip + pad
// ---------------------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void augment_kernel(const uint8_t* __restrict__ src, const int32_t* __restrict__ tab,
                                                      const CatsegTrainImageDesc* __restrict__ descs,
                                                      const int32_t* __restrict__ crops, int S, int tiles_x,
                                                      int64_t ignore_label, uint8_t* __restrict__ images,
                                                      int64_t* __restrict__ targets) {
  __shared__ uint8_t hbuf[ROWS][3][TW];
  const int b = blockIdx.y;
  const CatsegTrainImageDesc& d = descs[b];
  const int32_t* crop = d.crop_sel >= 0 ? crops + (int64_t)d.crop_sel * 4 : d.crop;
  const int y0 = crop[0], x0 = crop[1], ch = crop[2], cw = crop[3];
  const int flip = d.flip, w = d.w;
  const int ty0 = (blockIdx.x / tiles_x) * TH, tx0 = (blockIdx.x % tiles_x) * TW;
  const int oy = ty0 + (threadIdx.x >> 4), ox = tx0 + (threadIdx.x & 15) * 4;
  const bool row_in = oy < ch;

  int acc[4][3];
  bool pin[4];          // this lane's pixel lies inside the crop
  int rxs[4];           // its column in the resized image
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    pin[u] = row_in && ox + u < cw;
    rxs[u] = pin[u] ? x0 + (flip ? cw - 1 - (ox + u) : ox + u) : x0;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[u][k] = 1 << (PREC - 1);
  }

  if (ty0 < ch && tx0 < cw) {           // workgroup-uniform: the tile holds crop pixels
    const int th = min(TH, ch - ty0), tw = min(TW, cw - tx0);
    const int rxa = flip ? x0 + cw - (tx0 + tw) : x0 + tx0;      // first resized column of the tile
    const int rya = y0 + ty0, ryb = rya + th;                    // its resized rows [rya, ryb)
    const int32_t* xb = tab + d.xb_off;
    const int32_t* xk = tab + d.xk_off;
    const int32_t* yb = tab + d.yb_off;
    const int32_t* yk = tab + d.yk_off;
    const int kx = d.kx, ky = d.ky;
    // source rows of the tile: the bounds rise with the row
    const int sya = yb[2 * rya], syb = yb[2 * (ryb - 1)] + yb[2 * (ryb - 1) + 1];
    int ymin = 0, ycnt = 0;
    const int32_t* ykr = yk;
    if (row_in) {
      ymin = yb[2 * (y0 + oy)];
      ycnt = yb[2 * (y0 + oy) + 1];
      ykr = yk + (int64_t)(y0 + oy) * ky;
    }
    const uint8_t* simg = src + d.img_off;
    // the horizontal pass: lane -> (column lc of the tile, rows lr, lr + 4, ...)
    const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
    int hxmin = 0, hcnt = 0;
    const int32_t* hk = xk;
    if (lc < tw) {
      hxmin = xb[2 * (rxa + lc)];
      hcnt = xb[2 * (rxa + lc) + 1];
      hk = xk + (int64_t)(rxa + lc) * kx;
    }
    for (int c0 = sya; c0 < syb; c0 += ROWS) {
      const int nr = min(ROWS, syb - c0);
      __syncthreads();                  // the previous chunk has been consumed
      if (lc < tw) {
        for (int r = lr; r < nr; r += 4) {
          const uint8_t* p = simg + ((int64_t)(c0 + r) * w + hxmin) * 3;
          int s0 = 1 << (PREC - 1), s1 = s0, s2 = s0;
          for (int t = 0; t < hcnt; ++t) {
            const int k = hk[t];
            s0 += (int)p[3 * t] * k;
            s1 += (int)p[3 * t + 1] * k;
            s2 += (int)p[3 * t + 2] * k;
          }
          hbuf[r][0][lc] = (uint8_t)clip8(s0);
          hbuf[r][1][lc] = (uint8_t)clip8(s1);
          hbuf[r][2][lc] = (uint8_t)clip8(s2);
        }
      }
      __syncthreads();
      // the vertical taps of this lane's row that lie in the chunk
      const int ta = max(ymin, c0), tb = min(ymin + ycnt, c0 + nr);
      for (int y = ta; y < tb; ++y) {
        const int k = ykr[y - ymin];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int cidx = rxs[u] - rxa;           // a pixel outside the crop reads column x0 - rxa or any: unused
          const int ci = pin[u] ? cidx : 0;
#pragma unroll
          for (int q = 0; q < 3; ++q) acc[u][q] += (int)hbuf[y - c0][q][ci] * k;
        }
      }
    }
  }

  train_color::Record rec;
  rec.bright = d.bright; rec.order = d.order; rec.contrast = d.contrast; rec.sat = d.sat; rec.hue = d.hue;
  rec.hue_delta = d.hue_delta; rec.beta = d.beta; rec.c_alpha = d.c_alpha; rec.s_alpha = d.s_alpha;
  const bool colour = rec.bright | rec.contrast | rec.sat | rec.hue;

  int px[4][3];
  int64_t lab[4];
  const uint8_t* slab = src + d.lab_off;
  const int32_t* nx = tab + d.nx_off;
  const int64_t lrow = row_in ? (int64_t)tab[d.ny_off + y0 + oy] * w : 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    px[u][0] = px[u][1] = px[u][2] = 128;
    lab[u] = ignore_label;
    if (pin[u]) {
      int r = clip8(acc[u][0]), g = clip8(acc[u][1]), bl = clip8(acc[u][2]);
      if (colour) train_color::apply(rec, r, g, bl);
      px[u][0] = r; px[u][1] = g; px[u][2] = bl;
      lab[u] = load_label(slab, d.lab_bytes, lrow + nx[rxs[u]]);
    }
  }

  if (oy >= S) return;
  uint8_t* img = images + (int64_t)b * 3 * S * S + (int64_t)oy * S + ox;
  int64_t* tgt = targets + ((int64_t)b * S + oy) * S + ox;
  if (VEC) {                            // S % 4 == 0: a group of 4 pixels is inside the canvas or outside
    if (ox >= S) return;
#pragma unroll
    for (int q = 0; q < 3; ++q)
      *reinterpret_cast<uint32_t*>(img + (int64_t)q * S * S) =
          (uint32_t)px[0][q] | (uint32_t)px[1][q] << 8 | (uint32_t)px[2][q] << 16 | (uint32_t)px[3][q] << 24;
    longlong2 a, c;
    a.x = lab[0]; a.y = lab[1]; c.x = lab[2]; c.y = lab[3];
    reinterpret_cast<longlong2*>(tgt)[0] = a;
    reinterpret_cast<longlong2*>(tgt)[1] = c;
  } else {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (ox + u >= S) break;
#pragma unroll
      for (int q = 0; q < 3; ++q) img[(int64_t)q * S * S + u] = (uint8_t)px[u][q];
      tgt[u] = lab[u];
    }
  }
}

}  // namespace

extern "C" int catseg_train_crop_select(const uint8_t* src, const int32_t* tables, const CatsegTrainImageDesc* descs,
                                        const int32_t* cands, int B, int n_cand, int n_labels, int ignore_label,
                                        double max_area, int32_t* workspace, int32_t* crops, void* stream) {
  CATSEG_CHECK(src && tables && descs && cands && workspace && crops, "train_crop_select: null pointer");
  CATSEG_CHECK(B > 0 && B <= 65535 && n_cand > 0 && n_cand <= 65535, "train_crop_select: bad batch / candidate count");
  CATSEG_CHECK(n_labels > 0 && n_labels <= MAX_LABELS, "train_crop_select: need 0 < n_labels <= 4096");
  CATSEG_CHECK(max_area > 0.0, "train_crop_select: max_area must be positive");
  hipLaunchKernelGGL(crop_select_kernel, dim3(n_cand, B), dim3(256), 0, (hipStream_t)stream, src, tables, descs, cands,
                     n_cand, n_labels, ignore_label, max_area, workspace, workspace + (int64_t)B * n_cand, crops);
  return catseg_launch_status("train_crop_select");
}

extern "C" int catseg_train_augment(const uint8_t* src, const int32_t* tables, const CatsegTrainImageDesc* descs,
                                    const int32_t* crops, int B, int S, int64_t ignore_label, uint8_t* images,
                                    int64_t* targets, void* stream) {
  CATSEG_CHECK(src && tables && descs && images && targets, "train_augment: null pointer");
  CATSEG_CHECK(B > 0 && B <= 65535, "train_augment: bad batch");
  CATSEG_CHECK(S > 0 && S <= 16384, "train_augment: need 0 < S <= 16384");
  CATSEG_CHECK(((uintptr_t)targets & 7) == 0 && ((uintptr_t)descs & 7) == 0 && ((uintptr_t)tables & 3) == 0,
               "train_augment: misaligned targets / descriptors / tables");
  const int tiles_x = (S + TW - 1) / TW, tiles_y = (S + TH - 1) / TH;
  const bool vec = S % 4 == 0 && ((uintptr_t)images & 3) == 0 && ((uintptr_t)targets & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(augment_kernel<true>, dim3(tiles_x * tiles_y, B), dim3(256), 0, (hipStream_t)stream, src, tables,
                       descs, crops, S, tiles_x, ignore_label, images, targets);
  else
    hipLaunchKernelGGL(augment_kernel<false>, dim3(tiles_x * tiles_y, B), dim3(256), 0, (hipStream_t)stream, src,
                       tables, descs, crops, S, tiles_x, ignore_label, images, targets);
  return catseg_launch_status("train_augment");
}
