// MFMA GEMM with fused epilogue:  out[m, n] = act(alpha-free) ...
//
//   v = sum_k A[amap(m), k] * W[n, k]            (fp32 accumulate)
//   v += bias[n]                                 (optional, fp32)
//   v += add[addmap(m), n]   for n < add_ncols   (optional: per-image / per-class
//                                                 guidance terms, CLS broadcast)
//   v = act(v) * alpha
//   v += res[m, n] + res2[m, n]                  (optional residual streams)
//   out[store(m, n)] = v                          (row-major or ConvTranspose scatter)
//
// W is in nn.Linear layout [N, K] (K contiguous), as are A's rows, so both MFMA
// operands are K-contiguous 16-byte fragments.  The product is computed as
// D = W_tile . A_tile^T, so each lane ends with 4 CONSECUTIVE output columns of one
// row (C/D layout row = 4*(lane>>4)+r -> n, col = lane&15 -> m): one 8/16-byte
// vector store per fragment, and bias/residual loads are vectors too.
//
// This serves every GEMM-shaped op on the path: ViT QKV / out-proj / MLP,
// ln_post@proj, patch-embed (im2col), Swin and class-attention projections and
// MLPs, the cost volume, ConvTranspose2d (store mode 1) and the guidance terms.
#include "common.h"
#include "capi.h"

namespace {

constexpr int BK = 32;
constexpr int NT = 256;   // 4 waves

template <typename TA> struct Lds;
template <> struct Lds<bf16> { static constexpr int PAD = 8; };   // row = 40 bf16 = 80 B
template <> struct Lds<float> { static constexpr int PAD = 4; };  // row = 36 f32 = 144 B

struct EpiArgs {
  const float* bias;
  const void* add; int64_t ld_add; RowMap addmap; int64_t add_ncols;
  int act; float alpha;
  const void* res; int64_t ld_res;
  const void* res2; int64_t ld_res2;
  void* out; int64_t ldo;
  int store_mode; int cvt_k, cvt_hin, cvt_win, cvt_cout;
  const float* sa; const float* sw;   // fp8 path: per-row scales of A and W (dequant in the epilogue)
  int pf;                             // epilogue / store forms of the gemm3 and gemm6 kernels: EpiForm bits (epi_forms)
};
// EpiArgs::pf.  The two write-through forms carry a 31-bit byte offset: epi_forms clears them for larger outputs.
enum EpiForm : int {
  EF_PREFETCH = 1,   // gemm3 lean epilogue: next round's residual in flight, bias loaded once (knob epi_prefetch)
  EF_WIDE_REG = 2,   // gemm6 bf16 outputs: register-side epilogue wide_epilogue_bf16 (wide_epi)
  EF_WIDE_NT = 4,    // wide_epilogue_bf16 stores: nt (wide_store 1)
  EF_WIDE_WT = 8,    //                            sc1 write-through (wide_store 2)
  EF_G3_NT = 16,     // gemm3 lean fp32 stores: nt (gemm3_store 1)
  EF_G3_WT = 32,     //                         sc1 write-through (gemm3_store 2)
};

template <typename TO>
DEV void epilogue4(const EpiArgs& e, int64_t m, int64_t n, f32x4 acc) {
  float v[4] = {acc[0], acc[1], acc[2], acc[3]};
  if (e.bias) {
    float4 b = *reinterpret_cast<const float4*>(e.bias + n);
    v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
  }
  if (e.add && n < e.add_ncols) {
    float a[4];
    load4<TO>(reinterpret_cast<const TO*>(e.add) + rowmap(e.addmap, m) * e.ld_add + n, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += a[r];
  }
  if (e.act != ACT_NONE || e.alpha != 1.f) {
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = apply_act(v[r], e.act) * e.alpha;
  }
  if (e.res) {
    float a[4];
    load4<TO>(reinterpret_cast<const TO*>(e.res) + m * e.ld_res + n, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += a[r];
  }
  if (e.res2) {
    float a[4];
    load4<TO>(reinterpret_cast<const TO*>(e.res2) + m * e.ld_res2 + n, a);
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] += a[r];
  }
  int64_t off;
  if (e.store_mode == 0) {
    off = m * e.ldo + n;
  } else {   // ConvTranspose2d(k, stride k) scatter: m = (s, y, x), n = (ky, kx, co)
    off = convt_offset(m, n, e.cvt_k, e.cvt_hin, e.cvt_win, e.cvt_cout);
  }
  store4<TO>(reinterpret_cast<TO*>(e.out) + off, v);
}

// 8 consecutive output columns of one row (row-major store only): 16-byte bf16 stores,
// the form the LDS-staged epilogues use (an 8-byte store per lane halves the per-CU
// store rate, MI355X_MICROARCH.md "attention epilogue store tail").
DEV void load8f(const float* p, float v[8]) { load4<float>(p, v); load4<float>(p + 4, v + 4); }
DEV void load8f(const bf16* p, float v[8]) {
  const uint4 u = ld16(p);
  const unsigned w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) { v[2 * i] = __uint_as_float(w[i] << 16); v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u); }
}
DEV void store8f(float* p, const float v[8]) { store4<float>(p, v); store4<float>(p + 4, v + 4); }
DEV void store8f(bf16* p, const float v[8]) {
  st16(p, make_uint4(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]), f2bf2(v[4], v[5]), f2bf2(v[6], v[7])));
}

// EPI selects a compile-time epilogue: 0 = general (every runtime option), 1 = bias (+ res),
// 2 = bias + QuickGELU.  The lean forms drop the unused paths' code and registers, which the
// epilogue-heavy ViT GEMMs measurably feel (a dead scatter branch alone cost QKV 2.5 us).
template <typename TO, bool SC = false, int EPI = 0>
DEV void epilogue8(const EpiArgs& e, int64_t m, int64_t n, f32x4 lo, f32x4 hi) {
  float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  if constexpr (EPI != 0) {
    if (e.bias) {
      float b[8];
      load8f(e.bias + n, b);
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] += b[r];
    }
    if constexpr (EPI == 2) {
#pragma unroll
      for (int r = 0; r < 8; ++r) v[r] = apply_act(v[r], ACT_QUICKGELU);
    }
    if constexpr (EPI == 1) {
      if (e.res) {
        float a[8];
        load8f(reinterpret_cast<const TO*>(e.res) + m * e.ld_res + n, a);
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] += a[r];
      }
    }
    store8f(reinterpret_cast<TO*>(e.out) + m * e.ldo + n, v);
    return;
  }
  if (e.bias) {
    float b[8];
    load8f(e.bias + n, b);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += b[r];
  }
  if (e.add && n < e.add_ncols) {     // add_ncols is a multiple of 8 on the 8-wide path
    float a[8];
    load8f(reinterpret_cast<const TO*>(e.add) + rowmap(e.addmap, m) * e.ld_add + n, a);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += a[r];
  }
  if (e.act != ACT_NONE || e.alpha != 1.f) {
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] = apply_act(v[r], e.act) * e.alpha;
  }
  if (e.res) {
    float a[8];
    load8f(reinterpret_cast<const TO*>(e.res) + m * e.ld_res + n, a);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += a[r];
  }
  if (e.res2) {
    float a[8];
    load8f(reinterpret_cast<const TO*>(e.res2) + m * e.ld_res2 + n, a);
#pragma unroll
    for (int r = 0; r < 8; ++r) v[r] += a[r];
  }
  int64_t off = m * e.ldo + n;
  if constexpr (SC) {   // ConvTranspose2d scatter (as epilogue4); cout % 8 == 0 keeps the 8 columns together
    off = convt_offset(m, n, e.cvt_k, e.cvt_hin, e.cvt_win, e.cvt_cout);
  }
  store8f(reinterpret_cast<TO*>(e.out) + off, v);
}

template <typename TA, typename TO, int BM, int BN>
__global__ __launch_bounds__(NT) void gemm_kernel(const TA* __restrict__ A, int64_t lda, RowMap amap,
                                                  const TA* __restrict__ W, int64_t ldw,
                                                  int64_t M, int64_t N, int64_t K, EpiArgs e) {
  constexpr int VN = Vec16<TA>::N;           // elements per 16-byte chunk
  // fp32 K-tile 16 (bf16: 32): 37 KB of LDS per 128 x 128 workgroup, four workgroups per CU
  constexpr int BKT = sizeof(TA) == 4 ? 16 : BK;
  constexpr int CPR = BKT / VN;              // chunks per tile row
  constexpr int LDR = BKT + Lds<TA>::PAD;    // LDS row stride (elements)
  constexpr int A_CH = BM * CPR / NT;        // chunks per thread
  constexpr int W_CH = BN * CPR / NT;
  static_assert(A_CH >= 1 && W_CH >= 1, "tile too small");
  constexpr int WM = BM / 2, WN = BN / 2;    // wave tile (2x2 waves)
  constexpr int FM = WM / 16, FN = WN / 16;

  __shared__ __attribute__((aligned(16))) TA sA[2][BM * LDR];
  __shared__ __attribute__((aligned(16))) TA sW[2][BN * LDR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t m0 = (int64_t)blockIdx.x * BM, n0 = (int64_t)blockIdx.y * BN;
  const int wm = (wave & 1) * WM, wn = (wave >> 1) * WN;

  // per-thread staging rows (fixed over the K loop)
  const TA* a_ptr[A_CH]; int a_lrow[A_CH], a_col[A_CH]; bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    int c = tid + i * NT;
    a_lrow[i] = c / CPR; a_col[i] = (c % CPR) * VN;
    int64_t m = m0 + a_lrow[i];
    a_ok[i] = m < M;
    a_ptr[i] = A + (a_ok[i] ? rowmap(amap, m) : 0) * lda;
  }
  const TA* w_ptr[W_CH]; int w_lrow[W_CH], w_col[W_CH]; bool w_ok[W_CH];
#pragma unroll
  for (int i = 0; i < W_CH; ++i) {
    int c = tid + i * NT;
    w_lrow[i] = c / CPR; w_col[i] = (c % CPR) * VN;
    int64_t n = n0 + w_lrow[i];
    w_ok[i] = n < N;
    w_ptr[i] = W + (w_ok[i] ? n : 0) * ldw;
  }

  uint4 ra[A_CH], rw[W_CH];
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      int64_t k = k0 + a_col[i];
      ra[i] = (a_ok[i] && k < K) ? ld16(a_ptr[i] + k) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      int64_t k = k0 + w_col[i];
      rw[i] = (w_ok[i] && k < K) ? ld16(w_ptr[i] + k) : make_uint4(0, 0, 0, 0);
    }
  };
  // fp32: rows 8..15 of every 16-row group hold each 4-float chunk rotated by two (halves swapped),
  // so the 16 rows x 2 k of a ds_read_b32 lane group (bank = (36 row + k) mod 32) fall on 32
  // distinct banks instead of two rows per bank; the read index is k ^ 2 on those rows
  auto rot = [](uint4 u, int row) {
    if constexpr (sizeof(TA) == 4) return ((row >> 3) & 1) ? make_uint4(u.z, u.w, u.x, u.y) : u;
    else return u;
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) st16(&sA[buf][a_lrow[i] * LDR + a_col[i]], rot(ra[i], a_lrow[i]));
#pragma unroll
    for (int i = 0; i < W_CH; ++i) st16(&sW[buf][w_lrow[i] * LDR + w_col[i]], rot(rw[i], w_lrow[i]));
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int ktiles = (int)((K + BKT - 1) / BKT);
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ktiles) gload((int64_t)(kt + 1) * BKT);
    const TA* As = sA[buf];
    const TA* Ws = sW[buf];
    if constexpr (sizeof(TA) == 2) {
      const int r = lane & 15, kc = (lane >> 4) * 8;
      s16x8 bfrag[FM];
#pragma unroll
      for (int j = 0; j < FM; ++j)
        bfrag[j] = *reinterpret_cast<const s16x8*>(&As[(wm + 16 * j + r) * LDR + kc]);
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        s16x8 afrag = *reinterpret_cast<const s16x8*>(&Ws[(wn + 16 * i + r) * LDR + kc]);
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = mfma_bf16(afrag, bfrag[j], acc[i][j]);
      }
    } else {
      const int r = lane & 15, kq = (lane >> 4) ^ (((lane >> 3) & 1) << 1);   // rot() above
#pragma unroll
      for (int s = 0; s < BKT / 4; ++s) {
        float bv[FM];
#pragma unroll
        for (int j = 0; j < FM; ++j) bv[j] = As[(wm + 16 * j + r) * LDR + 4 * s + kq];
#pragma unroll
        for (int i = 0; i < FN; ++i) {
          float av = Ws[(wn + 16 * i + r) * LDR + 4 * s + kq];
#pragma unroll
          for (int j = 0; j < FM; ++j) acc[i][j] = mfma_f32(av, bv[j], acc[i][j]);
        }
      }
    }
    if (kt + 1 < ktiles) {
      sstore(buf ^ 1);
    }
    __syncthreads();
  }

  // epilogue
  const int col = lane & 15, rq = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    const int64_t n = n0 + wn + 16 * i + rq;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int64_t m = m0 + wm + 16 * j + col;
      if (m < M) epilogue4<TO>(e, m, n, acc[i][j]);
    }
  }
}

// ------------------------------------------------------------------------------------
// bf16 main GEMM: BK = 64, 16-byte chunks XOR-swizzled in LDS (chunk' = chunk ^ (row & 7))
// so the 16 rows a fragment read touches spread over the bank row; register-staged
// double buffer (next tile's global loads issued before the MFMAs of this one);
// 1-D grid remapped so consecutive tiles (same A row panel) land on one XCD's L2.
// ------------------------------------------------------------------------------------
constexpr int BK2 = 64;

template <typename TO, int BM, int BN>
__global__ __launch_bounds__(NT) void gemm2_kernel(const bf16* __restrict__ A, int64_t lda, RowMap amap,
                                                   const bf16* __restrict__ W, int64_t ldw, int64_t M, int64_t N,
                                                   int64_t K, int tiles_n, EpiArgs e) {
  constexpr int CPR = BK2 / 8;               // 8 chunks of 16 B per tile row
  constexpr int A_CH = BM * CPR / NT, W_CH = BN * CPR / NT;
  constexpr int WM = BM / 2, WN = BN / 2, FM = WM / 16, FN = WN / 16;
  __shared__ __attribute__((aligned(16))) bf16 sA[2][BM * BK2];
  __shared__ __attribute__((aligned(16))) bf16 sW[2][BN * BK2];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwg = gridDim.x;
  const int wg = xcd_remap(blockIdx.x, nwg);
  const int64_t m0 = (int64_t)(wg / tiles_n) * BM, n0 = (int64_t)(wg % tiles_n) * BN;
  const int wm = (wave & 1) * WM, wn = (wave >> 1) * WN;

  const bf16* a_ptr[A_CH]; int a_off[A_CH], a_col[A_CH]; bool a_ok[A_CH];
#pragma unroll
  for (int i = 0; i < A_CH; ++i) {
    const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
    a_col[i] = ch * 8;
    a_off[i] = (row * CPR + (ch ^ (row & 7))) * 8;
    const int64_t m = m0 + row;
    a_ok[i] = m < M;
    a_ptr[i] = A + (a_ok[i] ? rowmap(amap, m) : 0) * lda;
  }
  const bf16* w_ptr[W_CH]; int w_off[W_CH], w_col[W_CH]; bool w_ok[W_CH];
#pragma unroll
  for (int i = 0; i < W_CH; ++i) {
    const int c = tid + i * NT, row = c / CPR, ch = c % CPR;
    w_col[i] = ch * 8;
    w_off[i] = (row * CPR + (ch ^ (row & 7))) * 8;
    const int64_t n = n0 + row;
    w_ok[i] = n < N;
    w_ptr[i] = W + (w_ok[i] ? n : 0) * ldw;
  }
  uint4 ra[A_CH], rw[W_CH];
  auto gload = [&](int64_t k0) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) {
      const int64_t k = k0 + a_col[i];
      ra[i] = (a_ok[i] && k < K) ? ld16(a_ptr[i] + k) : make_uint4(0, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < W_CH; ++i) {
      const int64_t k = k0 + w_col[i];
      rw[i] = (w_ok[i] && k < K) ? ld16(w_ptr[i] + k) : make_uint4(0, 0, 0, 0);
    }
  };
  auto sstore = [&](int buf) {
#pragma unroll
    for (int i = 0; i < A_CH; ++i) st16(&sA[buf][a_off[i]], ra[i]);
#pragma unroll
    for (int i = 0; i < W_CH; ++i) st16(&sW[buf][w_off[i]], rw[i]);
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int r = lane & 15, q = lane >> 4;
  const int ktiles = (int)((K + BK2 - 1) / BK2);
  gload(0);
  sstore(0);
  __syncthreads();
  for (int kt = 0; kt < ktiles; ++kt) {
    const int buf = kt & 1;
    if (kt + 1 < ktiles) gload((int64_t)(kt + 1) * BK2);
    const bf16* As = sA[buf];
    const bf16* Ws = sW[buf];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int ch = ks * 4 + q;
      s16x8 bfrag[FM];
#pragma unroll
      for (int j = 0; j < FM; ++j) {
        const int row = wm + 16 * j + r;
        bfrag[j] = *reinterpret_cast<const s16x8*>(&As[(row * CPR + (ch ^ (row & 7))) * 8]);
      }
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        const int row = wn + 16 * i + r;
        const s16x8 afrag = *reinterpret_cast<const s16x8*>(&Ws[(row * CPR + (ch ^ (row & 7))) * 8]);
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = mfma_bf16(afrag, bfrag[j], acc[i][j]);
      }
    }
    if (kt + 1 < ktiles) sstore(buf ^ 1);
    __syncthreads();
  }
  const int col = lane & 15, rq = (lane >> 4) * 4;
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    const int64_t n = n0 + wn + 16 * i + rq;
    if (n >= N) continue;
#pragma unroll
    for (int j = 0; j < FM; ++j) {
      const int64_t m = m0 + wm + 16 * j + col;
      if (m < M) epilogue4<TO>(e, m, n, acc[i][j]);
    }
  }
}

// ------------------------------------------------------------------------------------
// bf16 large GEMM (ViT QKV / out-proj / MLP): LDS-DMA staging (global_load_lds 16 B,
// no VGPR round trip) into an S-stage ring of BK-deep K-tiles, with a counted `vmcnt` so
// S-2 tiles stay in flight across the single raw barrier of each K-step.  The LDS image
// of a tile is lane-linear per wave-instruction (64 x 16 B); the XOR swizzle
// slot = chunk ^ ((row / RPB) % BKC) (RPB = rows per 256-byte bank row) is applied on the
// per-lane GLOBAL source address and again on the fragment reads (the same involution
// on both sides), which makes the 16 rows of a ds_read_b128 fragment read hit 16
// distinct 16-byte bank slots.  WGM x WGN waves, each owning a (BM/WGM) x (BN/WGN)
// sub-tile of D = W . A^T (4 consecutive output columns per lane).  Needs K % BK == 0 and
// N % BN == 0 (host-checked); rows >= M read row M-1 and are masked in the epilogue.
// ------------------------------------------------------------------------------------

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
DEV i32x8 cat8(i32x4 a, i32x4 b) { return i32x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]}; }
// 16x16x128 e4m3 x e4m3 MFMA, unit block scales (E8M0 127 = 2^0)
DEV f32x4 mfma_fp8x128(i32x8 a, i32x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 127, 0, 127);
}

template <int BK>
struct Swz {
  static constexpr int BKC = BK / 8;            // 16-byte chunks per tile row
  static constexpr int RPB = 256 / (BK * 2);    // tile rows per 256-byte bank row
  static DEV int slot(int row, int ch) { return ch ^ ((row / RPB) % BKC); }
};

// F8: A and W hold OCP e4m3 bytes, addressed here in 2-byte units (K, lda, ldw, BK halved),
// so staging, swizzle and LDS-DMA are byte-identical to bf16.  One K=128 block-scaled MFMA
// (unit scales; fp8 rate = 2x bf16) consumes two 16-byte chunks per lane; A and W fragments
// read the same chunks, so the k order inside the instruction does not matter.  The
// epilogue multiplies by sa[m] * sw[n] (per-row dequant scales) before bias / act / residual.
// 1 (default) = the lean one-item-per-thread epilogue with the next round's residual in flight and the
// bias loaded once (same box, M = 4616: out-proj 20.8 -> 19.9 us, fc1 55.1 -> 52.7, fc2 48.3 -> 47.1;
// bit-identical); 0 = one residual round trip per epilogue round
int g_epi_prefetch = 1;
int g_gemm3_store = 0;  // gemm3 lean fp32 epilogue stores: 0 = plain, 1 = nt (A/B knob)
// gemm6 bf16 epilogue stores: 0 = plain, 1 = nt, 2 = sc1 write-through (default: the output leaves the
// XCD's L2 as it is written instead of as dirty lines at the kernel boundary; same box, whole step,
// tools/ab_knob.py: 9.309 / 9.286 / 9.234 ms)
int g_wide_store = 2;
int g_wide_epi = 1;   // gemm6 bf16 outputs: 1 = register-side epilogue (wide_epilogue_bf16), 0 = fp32 LDS staging
// read-only diagnostics (tests): the kernel of the last launch -- the variant number of a gemm3 / gemm6
// tile, 2 = gemm2_kernel, 3 = the generic gemm_kernel -- and whether it took a write-through store form
int g_gemm_last = 0;
int g_gemm_last_wt = 0;
// gemm3's lean one-or-two-items-per-thread epilogue (the only gemm3 path with the gemm3_store forms):
// the kernel's own condition, shared with launch3 so that gemm_last_wt reports what the kernel does
template <int BM, int BN, int WGM, int WGN, int EPI, bool SC>
struct Gemm3Lean {
  static constexpr int NT3 = 64 * WGM * WGN, FM = BM / WGM / 16;
  static constexpr int JR0 = 4 / WGM, JR = FM % JR0 == 0 ? JR0 : (JR0 >= 2 && FM % 2 == 0 ? 2 : 1);
  static constexpr int ROWS = WGM * JR * 16;
  static constexpr int IPT = ROWS * (BN / 8) / NT3;   // output items per thread per round
  static constexpr bool ONE = IPT >= 1 && IPT <= 2 && ROWS * (BN / 8) == IPT * NT3 && NT3 % (BN / 8) == 0 && EPI != 0 &&
                              !SC;
};
template <typename TO, int BM, int BN, int WGM, int WGN, int S, int BK, bool F8 = false, bool SC = false,
          int EPI = 0>
__global__ __launch_bounds__(64 * WGM * WGN) void gemm3_kernel(const bf16* __restrict__ A, int64_t lda, RowMap amap,
                                                            const bf16* __restrict__ W, int64_t ldw, int64_t M,
                                                            int64_t K, int tiles_n, EpiArgs e, int group_m) {
  constexpr int NT3 = 64 * WGM * WGN;
  using SW = Swz<BK>;
  constexpr int BKC = SW::BKC;
  // A chunks may leave a partial last group (160 / 224-row tiles at 8 waves): every wave still
  // issues it (uniform counted vmcnt), the waves past AREM re-loading the chunks of wave
  // (wave mod AREM/64) into the same LDS slots -- identical bytes, a benign duplicate write
  constexpr int AG = (BM * BKC + NT3 - 1) / NT3, WG = BN * BKC / NT3, G = AG + WG;
  constexpr int AREM = BM * BKC - (AG - 1) * NT3;      // chunks of the last A group
  static_assert(WG * NT3 == BN * BKC, "tile / thread mismatch");
  static_assert(AREM % 64 == 0, "partial A group must be whole waves");
  constexpr int WM = BM / WGM, WN = BN / WGN, FM = WM / 16, FN = WN / 16;
  constexpr int STAGE = (BM + BN) * BK;           // elements per stage
  __shared__ __attribute__((aligned(16))) bf16 smem[S * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  // tile order: row-major, or grouped (group_m m-tiles swept across all n-tiles) so that each
  // XCD's contiguous range of tiles covers a 2-D block: fewer A / W bytes per XCD L2
  int tm_i, tn_i;
  if (group_m > 0) {
    const int tiles_m = (int)((M + BM - 1) / BM);
    const int per = group_m * tiles_n, g = wg / per, r = wg - g * per;
    const int gs = min(group_m, tiles_m - g * group_m);
    tm_i = g * group_m + r % gs;
    tn_i = r / gs;
  } else {
    tm_i = wg / tiles_n;
    tn_i = wg % tiles_n;
  }
  const int64_t m0 = (int64_t)tm_i * BM, n0 = (int64_t)tn_i * BN;
  const int wm = (wave % WGM) * WM, wn = (wave / WGM) * WN;
  const bool ident = amap.d1 == 1 && amap.m1 >= M && amap.s1 == 1 && amap.m2 == 1 && amap.off == 0;

  // per-instruction source pointers: chunk c = g*NT3 + tid -> LDS row c/BKC, slot c%BKC,
  // which holds the global chunk slot(row, c%BKC)
  const bf16* asrc[AG];
#pragma unroll
  for (int g = 0; g < AG; ++g) {
    const int c = g * NT3 + (g == AG - 1 ? tid % AREM : tid), row = c / BKC, ch = SW::slot(row, c % BKC);
    int64_t m = m0 + row;
    if (m >= M) m = M - 1;
    asrc[g] = A + (ident ? m : rowmap(amap, m)) * lda + ch * 8;
  }
  const bf16* wsrc[WG];
#pragma unroll
  for (int g = 0; g < WG; ++g) {
    const int c = g * NT3 + tid, row = c / BKC, ch = SW::slot(row, c % BKC);
    wsrc[g] = W + (n0 + row) * ldw + ch * 8;
  }
  auto issue = [&](int kt) {
    bf16* sa = smem + (kt % S) * STAGE;
    bf16* sw = sa + BM * BK;
    const int64_t k0 = (int64_t)kt * BK;
#pragma unroll
    for (int g = 0; g < AG; ++g) {
      const int wv = g == AG - 1 ? wave % (AREM / 64) : wave;
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(asrc[g] + k0), (lds_void_t*)(sa + (g * NT3 + wv * 64) * 8), 16, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < WG; ++g)
      __builtin_amdgcn_global_load_lds((gbl_void_t*)(wsrc[g] + k0), (lds_void_t*)(sw + (g * NT3 + wave * 64) * 8), 16, 0, 0);
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int r = lane & 15, q = lane >> 4;
  const int ktiles = (int)(K / BK);
#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < ktiles) issue(t);
  for (int kt = 0; kt < ktiles; ++kt) {
    // tiles kt .. min(kt+S-2, ktiles-1) are in flight; retire tile kt
    if (kt + S - 2 < ktiles) wait_vmcnt<(S - 2) * G>();
    else wait_vmcnt<0>();
    __builtin_amdgcn_s_barrier();                 // tile kt visible; stage (kt-1)%S free
    __builtin_amdgcn_sched_barrier(0);
    if (kt + S - 1 < ktiles) issue(kt + S - 1);
    const bf16* As = smem + (kt % S) * STAGE;
    const bf16* Ws = As + BM * BK;
    if constexpr (F8) {
      static_assert(BK % 64 == 0, "fp8 K-step is 128 bytes");
#pragma unroll
      for (int ks = 0; ks < BK / 64; ++ks) {
        const int ch = ks * 8 + 2 * q;
        i32x8 bfrag[FM], afrag[FN];
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int row = wm + 16 * j + r;
          bfrag[j] = cat8(*reinterpret_cast<const i32x4*>(&As[(row * BKC + SW::slot(row, ch)) * 8]),
                          *reinterpret_cast<const i32x4*>(&As[(row * BKC + SW::slot(row, ch + 1)) * 8]));
        }
#pragma unroll
        for (int i = 0; i < FN; ++i) {
          const int row = wn + 16 * i + r;
          afrag[i] = cat8(*reinterpret_cast<const i32x4*>(&Ws[(row * BKC + SW::slot(row, ch)) * 8]),
                          *reinterpret_cast<const i32x4*>(&Ws[(row * BKC + SW::slot(row, ch + 1)) * 8]));
        }
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FM; ++j) acc[i][j] = mfma_fp8x128(afrag[i], bfrag[j], acc[i][j]);
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < BK / 32; ++ks) {
        const int ch = ks * 4 + q;
        s16x8 bfrag[FM], afrag[FN];
#pragma unroll
        for (int j = 0; j < FM; ++j) {
          const int row = wm + 16 * j + r;
          bfrag[j] = *reinterpret_cast<const s16x8*>(&As[(row * BKC + SW::slot(row, ch)) * 8]);
        }
#pragma unroll
        for (int i = 0; i < FN; ++i) {
          const int row = wn + 16 * i + r;
          afrag[i] = *reinterpret_cast<const s16x8*>(&Ws[(row * BKC + SW::slot(row, ch)) * 8]);
        }
#pragma unroll
        for (int i = 0; i < FN; ++i)
#pragma unroll
          for (int j = 0; j < FM; ++j) acc[i][j] = mfma_bf16(afrag[i], bfrag[j], acc[i][j]);
      }
    }
  }
  // ---- epilogue through LDS: rounds of 64 tile rows (JR m-fragments per wave row) are
  // staged as fp32, then every thread walks whole output rows (coalesced stores); the
  // accumulator indices stay compile-time constants (no scratch) ----
  // JR = the largest divisor of FM that keeps a round <= 64 rows (FM = 5 for 160-row tiles)
  constexpr int JR0 = 4 / WGM, JR = FM % JR0 == 0 ? JR0 : (JR0 >= 2 && FM % 2 == 0 ? 2 : 1);
  constexpr int ROWS = WGM * JR * 16, SLD = BN + 4;
  static_assert(JR >= 1 && FM % JR == 0, "epilogue rounds");
  static_assert(ROWS * SLD * 4 <= S * STAGE * 2, "epilogue stage exceeds LDS");
  float* stg = reinterpret_cast<float*>(smem);
  const int col = lane & 15, rq = (lane >> 4) * 4;
  const int wmi = wave % WGM;
  // lean epilogues with one or two output items per thread per round (160 x 128, 96 x 128, 224 x 256): the
  // bias of the thread's 8 columns is loaded once, and the residual rows of round h + 1 are
  // requested before round h's barrier, so no round waits for its own global loads (the loop
  // below issues them inside each round: one HBM round trip per round, ~5 rounds per tile)
  // IPT = output items per thread per round; every item of a thread has the same 8 columns
  using Lean = Gemm3Lean<BM, BN, WGM, WGN, EPI, SC>;
  static_assert(Lean::ROWS == ROWS, "Gemm3Lean mirrors the epilogue rounds");
  constexpr int IPT = Lean::IPT;
  constexpr bool ONE = Lean::ONE;
  if constexpr (ONE) {
    if (e.pf & EF_PREFETCH) {
      const int c8 = (tid % (BN / 8)) * 8;
      const int64_t n = n0 + c8;
      float b[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (e.bias) load8f(e.bias + n, b);
      auto lrow_of = [&](int k) { return (tid + k * NT3) / (BN / 8); };
      auto mrow = [&](int h, int k) {
        const int lrow = lrow_of(k);
        const int wi = lrow / (JR * 16), jj = (lrow / 16) % JR, rr = lrow % 16;
        return m0 + wi * WM + (h * JR + jj) * 16 + rr;
      };
      const bool res = EPI == 1 && e.res;
      float rc[IPT][8], rn[IPT][8];
      // F8: the per-column dequant scales once, the per-row scale of each item with its residual
      float wsc[8];
      float sc[IPT], sn[IPT];
      if constexpr (F8) load8f(e.sw + n, wsc);
      auto ldres = [&](int h, float (&r)[IPT][8], float (&sr)[IPT]) {
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const int64_t m = std::min<int64_t>(mrow(h, k), M - 1);
          if (res) load8f(reinterpret_cast<const TO*>(e.res) + m * e.ld_res + n, r[k]);
          if constexpr (F8) sr[k] = e.sa[ident ? m : rowmap(amap, m)];
        }
      };
      ldres(0, rc, sc);
#pragma unroll
      for (int h = 0; h < FM / JR; ++h) {
        if (h + 1 < FM / JR) ldres(h + 1, rn, sn);
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int j2 = 0; j2 < JR; ++j2)
#pragma unroll
          for (int i = 0; i < FN; ++i)
            *reinterpret_cast<f32x4*>(&stg[((wmi * JR + j2) * 16 + col) * SLD + wn + 16 * i + rq]) = acc[i][h * JR + j2];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
          const int lrow = lrow_of(k);
          const int64_t m = mrow(h, k);
          if (m < M) {
            const f32x4 lo = *reinterpret_cast<const f32x4*>(&stg[lrow * SLD + c8]);
            const f32x4 hi = *reinterpret_cast<const f32x4*>(&stg[lrow * SLD + c8 + 4]);
            float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            if constexpr (F8) {
#pragma unroll
              for (int r = 0; r < 8; ++r) v[r] = v[r] * (wsc[r] * sc[k]);
            }
            if (e.bias) {
#pragma unroll
              for (int r = 0; r < 8; ++r) v[r] += b[r];
            }
            if constexpr (EPI == 2) {
#pragma unroll
              for (int r = 0; r < 8; ++r) v[r] = apply_act(v[r], ACT_QUICKGELU);
            }
            if (res) {
#pragma unroll
              for (int r = 0; r < 8; ++r) v[r] += rc[k][r];
            }
            if constexpr (sizeof(TO) == 4) {
              if (e.pf & EF_G3_NT) {    // A/B knob gemm3_store 1: nt stores of the fp32 rows
                float* p = reinterpret_cast<float*>(e.out) + m * e.ldo + n;
                __builtin_nontemporal_store(f32x4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f32x4*>(p));
                __builtin_nontemporal_store(f32x4{v[4], v[5], v[6], v[7]}, reinterpret_cast<f32x4*>(p + 4));
                continue;
              }
              if (e.pf & EF_G3_WT) {    // gemm3_store 2: sc1 write-through
                const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(e.out, (short)0, 0x7fffffff, 0x00020000);
                const int off = (int)((m * e.ldo + n) * 4);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, f32x4{v[0], v[1], v[2], v[3]}), r, off, 0, 16);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, f32x4{v[4], v[5], v[6], v[7]}), r, off + 16, 0, 16);
                continue;
              }
            }
            store8f(reinterpret_cast<TO*>(e.out) + m * e.ldo + n, v);
          }
        }
#pragma unroll
        for (int k = 0; k < IPT; ++k) {
#pragma unroll
          for (int r = 0; r < 8; ++r) rc[k][r] = rn[k][r];
          sc[k] = sn[k];
        }
      }
      return;
    }
  }
#pragma unroll
  for (int h = 0; h < FM / JR; ++h) {
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int jj = 0; jj < JR; ++jj)
#pragma unroll
      for (int i = 0; i < FN; ++i)
        *reinterpret_cast<f32x4*>(&stg[((wmi * JR + jj) * 16 + col) * SLD + wn + 16 * i + rq]) = acc[i][h * JR + jj];
    __syncthreads();
    for (int idx = tid; idx < ROWS * (BN / 8); idx += NT3) {
      const int lrow = idx / (BN / 8), c8 = (idx % (BN / 8)) * 8;
      const int wi = lrow / (JR * 16), jj = (lrow / 16) % JR, rr = lrow % 16;
      const int64_t m = m0 + wi * WM + (h * JR + jj) * 16 + rr;
      if (m < M) {
        f32x4 lo = *reinterpret_cast<const f32x4*>(&stg[lrow * SLD + c8]);
        f32x4 hi = *reinterpret_cast<const f32x4*>(&stg[lrow * SLD + c8 + 4]);
        if constexpr (F8) {
          const float s = e.sa[ident ? m : rowmap(amap, m)];   // scale of the A row read for m
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(e.sw + n0 + c8);
          const f32x4 w1 = *reinterpret_cast<const f32x4*>(e.sw + n0 + c8 + 4);
          lo = lo * (w0 * s);
          hi = hi * (w1 * s);
        }
        epilogue8<TO, SC, EPI>(e, m, n0 + c8, lo, hi);
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// Wide tiles for the ViT GEMMs (gemm6): BM = 320 rows x BN = 256 / 192 columns, one 8-wave
// workgroup per CU.  At M = 4616 the 320-row tiles make ONE round on 240 CUs for fc1 (15 x 16 at
// BN 256) and QKV (15 x 16 at BN 192), with half of gemm3's L2 -> LDS bytes per FLOP (142 FLOP per
// byte at 320 x 256 vs 71 at 160 x 128): 8 waves as 2 (m) x 4 (n), a 160 x 64 (48) wave tile = 14
// (13) fragment reads per 40 (30) MFMAs per k32, 160 (120) accumulator VGPRs.  Arithmetic per
// output = gemm3's (the same MFMA over the same k order, the same epilogue expression), so the tile
// choice never changes a bit (batch invariance).  Round-6 forms measured and removed (DESIGN.md
// §11): BK = 32 stages (16 rows x 64 B per DMA instruction), in step or ping-pong; a register-
// prefetched 160 x 128 tile for the narrow-N GEMMs.
// ------------------------------------------------------------------------------------
// 16-byte LDS-DMA through a buffer resource (buffer_load_dwordx4 ... lds): base and size are wave-
// uniform, the lane's part is a 32-bit byte offset, `soff` a uniform byte offset (SGPR)
DEV void dma_buf16(const void* base, int bytes, void* lds, int voff, int soff) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), (short)0, bytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_t*)lds, 16, voff, soff, 0, 0);
}

DEV int swz4(int r) { return (0x78 >> (2 * ((r >> 2) & 3))) & 3; }   // g = {0, 2, 3, 1} as 2-bit fields

// Tile origin for the wide kernels: after the XCD remap, groups of `group_m` m-tiles sweep the
// n-tiles, so an XCD's contiguous range of workgroups covers a compact block of A and W panels.
DEV void wide_tile(int wg, int64_t M, int BM, int tiles_n, int group_m, int& tm_i, int& tn_i) {
  const int tiles_m = (int)((M + BM - 1) / BM);
  const int per = group_m * tiles_n, g = wg / per, r = wg - g * per;
  const int gs = min(group_m, tiles_m - g * group_m);
  tm_i = g * group_m + r % gs;
  tn_i = r / gs;
}

// LDS-staged epilogue shared by gemm4 / gemm5: rounds of 64 tile rows (2 m-fragments per wave
// row) staged as fp32, each thread then stores 8 consecutive columns of whole rows; the bias of a
// thread's items is loaded once, a round's residual rows are all requested before the round's
// first barrier.
template <typename TO, int BM, int BN, int EPI, int FM, int FN>
DEV void wide_epilogue(const EpiArgs& e, f32x4 (&acc)[FN][FM], bf16* smem, int64_t M, int64_t m0, int64_t n0) {
  constexpr int NT4 = 512, WGM = 2, WM = BM / WGM, WN = BN / 4;
  constexpr int JR = FM % 2 == 0 ? 2 : 1, ROWS = WGM * JR * 16, SLD = BN + 4;
  static_assert(FM % JR == 0, "epilogue rounds");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wmi = wave / 4, wn = (wave % 4) * WN;
  float* stg = reinterpret_cast<float*>(smem);
  const int col = lane & 15, rq = (lane >> 4) * 4;
  constexpr int CG = BN / 8, ITEMS = ROWS * CG, IPT = (ITEMS + NT4 - 1) / NT4;
  static_assert(ITEMS % 64 == 0, "whole waves per epilogue item slot");
  // when 512 is a multiple of the column groups every item of a thread has the same 8 columns
  constexpr bool SAMEC = NT4 % CG == 0;
  constexpr int NB = SAMEC ? 1 : IPT;
  int lr[IPT], c8[IPT];
  float bias[NB][8];
#pragma unroll
  for (int k = 0; k < IPT; ++k) {
    const int idx = min(tid + k * NT4, ITEMS - 1);
    lr[k] = idx / CG;
    c8[k] = (idx % CG) * 8;
  }
#pragma unroll
  for (int k = 0; k < NB; ++k) {
#pragma unroll
    for (int r = 0; r < 8; ++r) bias[k][r] = 0.f;
    if (e.bias) load8f(e.bias + n0 + c8[k], bias[k]);
  }
  const bool res = EPI == 1 && e.res;
#pragma unroll
  for (int h = 0; h < FM / JR; ++h) {
    int64_t mk[IPT];
    float rv[IPT][8];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int lrow = lr[k], wi = lrow / (JR * 16), jj = (lrow / 16) % JR, rr = lrow % 16;
      mk[k] = m0 + wi * WM + (h * JR + jj) * 16 + rr;
      if (res) load8f(reinterpret_cast<const TO*>(e.res) + min<int64_t>(mk[k], M - 1) * e.ld_res + n0 + c8[k], rv[k]);
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < JR; ++jj)
#pragma unroll
      for (int i = 0; i < FN; ++i)
        *reinterpret_cast<f32x4*>(&stg[((wmi * JR + jj) * 16 + col) * SLD + wn + 16 * i + rq]) = acc[i][h * JR + jj];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      if (tid + k * NT4 < ITEMS && mk[k] < M) {
        const f32x4 lo = *reinterpret_cast<const f32x4*>(&stg[lr[k] * SLD + c8[k]]);
        const f32x4 hi = *reinterpret_cast<const f32x4*>(&stg[lr[k] * SLD + c8[k] + 4]);
        float v[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
#pragma unroll
        for (int r = 0; r < 8; ++r) v[r] += bias[SAMEC ? 0 : k][r];
        if constexpr (EPI == 2) {
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] = apply_act(v[r], ACT_QUICKGELU);
        }
        if (res) {
#pragma unroll
          for (int r = 0; r < 8; ++r) v[r] += rv[k][r];
        }
        store8f(reinterpret_cast<TO*>(e.out) + mk[k] * e.ldo + n0 + c8[k], v);
      }
    }
  }
}

// Register-side epilogue of the wide kernels for bf16 outputs without a residual (QKV: bias; fc1:
// bias + QuickGELU).  The bias (4 columns per n-fragment, fixed per lane) and the activation are
// applied on the accumulators in registers; the bf16 values go through LDS in TWO rounds of half the
// tile's rows (both wave rows' m-fragments 0..FM/2-1, then the rest), 8-byte writes into rows of
// BN + 8 elements (a row stride = 16 B mod 256: the 16 rows of a write group hit 16 distinct 16-B
// slots), and leave as whole-row 16-byte stores.  Against wide_epilogue: 4 instead of 10 barriers and
// half the LDS bytes (bf16 instead of fp32 staging); the arithmetic of an output is the same
// expression (acc + bias, then the activation, then one rounding).
template <int BM, int BN, int EPI, int FM, int FN>
DEV void wide_epilogue_bf16(const EpiArgs& e, f32x4 (&acc)[FN][FM], bf16* smem, int64_t M, int64_t m0, int64_t n0) {
  constexpr int NT4 = 512, WM = BM / 2, WN = BN / 4, SR = BN + 8;
  constexpr int FH = FM / 2, ROWS = 2 * FH * 16;                 // rows staged per round
  static_assert(FM % 2 == 0, "two rounds");
  static_assert(ROWS * SR * 2 <= 160 * 1024, "staging exceeds LDS");
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wmi = wave / 4, wn = (wave % 4) * WN;
  const int col = lane & 15, q = lane >> 4;
  float bias[FN][4];
#pragma unroll
  for (int i = 0; i < FN; ++i) {
    if (e.bias) {
      const float4 b = *reinterpret_cast<const float4*>(e.bias + n0 + wn + 16 * i + 4 * q);
      bias[i][0] = b.x; bias[i][1] = b.y; bias[i][2] = b.z; bias[i][3] = b.w;
    } else {
      bias[i][0] = bias[i][1] = bias[i][2] = bias[i][3] = 0.f;
    }
  }
  constexpr int CG = BN / 8, ITEMS = ROWS * CG, IPT = (ITEMS + NT4 - 1) / NT4;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < FH; ++jj)
#pragma unroll
      for (int i = 0; i < FN; ++i) {
        const f32x4 a = acc[i][h * FH + jj];
        float v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = a[r] + bias[i][r];
          if constexpr (EPI == 2) v[r] = apply_act(v[r], ACT_QUICKGELU);
        }
        const int lrow = (wmi * FH + jj) * 16 + col;
        *reinterpret_cast<uint2*>(&smem[lrow * SR + wn + 16 * i + 4 * q]) = make_uint2(f2bf2(v[0], v[1]), f2bf2(v[2], v[3]));
      }
    __syncthreads();
    uint4 val[IPT];
    int64_t mr[IPT];
    int cc[IPT];
#pragma unroll
    for (int k = 0; k < IPT; ++k) {
      const int idx = min(tid + k * NT4, ITEMS - 1);
      const int lrow = idx / CG, c8 = (idx % CG) * 8;
      const int wi = lrow / (FH * 16), rr = lrow % (FH * 16);
      mr[k] = m0 + wi * WM + h * FH * 16 + rr;
      cc[k] = c8;
      val[k] = *reinterpret_cast<const uint4*>(&smem[lrow * SR + c8]);
    }
#pragma unroll
    for (int k = 0; k < IPT; ++k)
      if (tid + k * NT4 < ITEMS && mr[k] < M) {
        bf16* p = reinterpret_cast<bf16*>(e.out) + mr[k] * e.ldo + n0 + cc[k];
        if (e.pf & EF_WIDE_NT) __builtin_nontemporal_store(__builtin_bit_cast(i32x4, val[k]), reinterpret_cast<i32x4*>(p));
        else if (e.pf & EF_WIDE_WT) {
          const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(e.out, (short)0, 0x7fffffff, 0x00020000);
          __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(i32x4, val[k]), r,
                                                 (int)((mr[k] * e.ldo + n0 + cc[k]) * 2), 0, 16);   // sc1 write-through
        } else st16(p, val[k]);
      }
  }
}

// gemm6's choice of the register-side bf16 epilogue (wide_epilogue_bf16, the only gemm6 path with the
// wide_store forms): the kernel's own condition, shared with launch6 so that gemm_last_wt reports what the
// kernel does.  CAN is the compile-time half (bf16 output, an even count of m-fragments), GEMM6_REG_USE the
// run-time half: a macro, because behind a bool-returning function the same expression compiles to other
// branches, and with them another register allocation, in the EPI 1 kernels.
template <typename TO, int BM>
struct Gemm6Reg {
  static constexpr bool CAN = sizeof(TO) == 2 && (BM / 32) % 2 == 0;
};
#define GEMM6_REG_USE(EPI, e) (((e).pf & EF_WIDE_REG) && !((EPI) == 1 && (e).res))

// gemm6: the wide tile as a PING-PONG loop (cdna_hip_programming.md §5, the staggered 8-wave
// template) with FULL-LINE staging.  Waves w and w + 4 share a SIMD; the waves of the second m-half
// (group 1 = waves 4-7) run one barrier behind group 0, so between any two barriers one group issues
// its fragment reads, LDS-DMA and counted waits (LOAD) while the other issues MFMAs (COMPUTE): each
// SIMD's matrix pipe is fed by one wave while its partner loads.  The stages are BK = 64 (each DMA
// wave-instruction moves 8 rows x 128 B, whole lines; the BK = 32 form's 16 rows x 64 B measured
// 724 vs 683 us of fill alone at 8192^3) in S = 2 slots (2 x (BM + BN) x 128 B of LDS), each K64
// tile run as two k32 phases so the per-wave fragment registers stay those of one k32 step.  The
// DMA is buffer_load ... lds (one 32-bit lane offset, the K offset in soffset: no per-issue VALU).
// Schedule (interval = the span between two barriers; group 1 one interval behind group 0):
//   group 0: L(t,0) @4t, C(t,0) @4t+1, L(t,1) @4t+2, C(t,1) @4t+3;  group 1: each one later.
//   L(t,0) issues the wave's share of tile t + 1's DMA (slot (t + 1) % 2 = (t - 1) % 2, whose last
//   reads -- group 1's L(t - 1, 1) @4t-1 -- retired before the barrier that opened @4t);
//   tile t + 1 is read from @4t+4 (group 0) / @4t+5 (group 1), so every wave waits its own DMA of
//   t + 1 before the barrier closing @4t+3: group 0 at the end of C(t,1), group 1 at the end of L(t,1).
// Swizzle: the 16-byte chunk c of row r sits at slot c ^ ((r / 2) % 8) (Swz<64>, as gemm3).
template <typename TO, int BM, int BN, int EPI>
__global__ __launch_bounds__(512) void gemm6_kernel(const bf16* __restrict__ A, int64_t lda, const bf16* __restrict__ W,
                                                    int64_t ldw, int64_t M, int64_t K, int tiles_n, EpiArgs e,
                                                    int group_m) {
  constexpr int BK = 64, BKC = 8, WM = BM / 2, WN = BN / 4, FM = WM / 16, FN = WN / 16;
  constexpr int STAGE = (BM + BN) * BK, NI = (BM + BN) / 8, JMAX = (NI + 7) / 8;
  static_assert(BM % 16 == 0 && BN % 16 == 0, "rows per fragment");
  using SW = Swz<64>;
  __shared__ __attribute__((aligned(16))) bf16 smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int grp = __builtin_amdgcn_readfirstlane(wave) >> 2;
  int tm_i, tn_i;
  wide_tile(xcd_remap(blockIdx.x, gridDim.x), M, BM, tiles_n, group_m, tm_i, tn_i);
  const int64_t m0 = (int64_t)tm_i * BM, n0 = (int64_t)tn_i * BN;
  const int wm = grp * WM, wn = (wave % 4) * WN;

  // DMA plan: instruction i = wave + 8 j covers stage rows 8 i .. 8 i + 7 (A rows, then W rows);
  // lane -> row 8 i + lane / 8, physical slot lane % 8 = logical chunk SW::slot(row, lane % 8).
  // Buffer loads (buffer_load_dwordx4 ... lds): whether instruction j reads A or W is wave-uniform,
  // the lane's part is one 32-bit byte offset, the K offset goes in soffset (no per-issue VALU).
  const int64_t abytes = M * lda * 2, wbytes = (int64_t)tiles_n * BN * ldw * 2;
  const int anr = abytes < 0x7fffffff ? (int)abytes : 0x7fffffff, wnr = wbytes < 0x7fffffff ? (int)wbytes : 0x7fffffff;
  const int wv = __builtin_amdgcn_readfirstlane(wave);
  const bool full = (wave + 8 * (JMAX - 1)) < NI;
  int voff[JMAX];
#pragma unroll
  for (int j = 0; j < JMAX; ++j) {
    const int i = min(wave + 8 * j, NI - 1);
    const int row = 8 * i + (lane >> 3), ch = SW::slot(row, lane & 7);
    if (row < BM) {
      const int64_t m = min<int64_t>(m0 + row, M - 1);
      voff[j] = (int)((m * lda + ch * 8) * 2);
    } else {
      voff[j] = (int)(((n0 + row - BM) * ldw + ch * 8) * 2);
    }
  }
  auto issue = [&](int kt) {
    bf16* st = smem + (kt & 1) * STAGE;
    const int kb = kt * BK * 2;
#pragma unroll
    for (int j = 0; j < JMAX; ++j) {
      if (j < JMAX - 1 || full) {
        if ((wv + 8 * j) * 8 < BM) dma_buf16(A, anr, st + (wv + 8 * j) * 512, voff[j], kb);   // wave-uniform choice
        else dma_buf16(W, wnr, st + (wv + 8 * j) * 512, voff[j], kb);
      }
    }
  };

  f32x4 acc[FN][FM];
#pragma unroll
  for (int i = 0; i < FN; ++i)
#pragma unroll
    for (int j = 0; j < FM; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int r16 = lane & 15, q = lane >> 4;
  // fragment address of row base rb (a multiple of 16), k32 half h: rows rb + r16, chunk 4 h + q,
  // whose slot (4 h + q) ^ ((r16 / 2) % 8) depends on the lane only
  const int fo0 = r16 * BK + ((q ^ ((r16 >> 1) & 7)) * 8), fo1 = r16 * BK + (((4 + q) ^ ((r16 >> 1) & 7)) * 8);
  auto fptr = [&](const bf16* base, int rb, int h) {
    return reinterpret_cast<const s16x8*>(&base[rb * BK + (h ? fo1 : fo0)]);
  };
  const int ktiles = (int)(K / BK);
  issue(0);
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();                        // tile 0 visible
  if (grp == 1) __builtin_amdgcn_s_barrier();          // the stagger
  __builtin_amdgcn_sched_barrier(0);
  for (int kt = 0; kt < ktiles; ++kt) {
    const bf16* As = smem + (kt & 1) * STAGE;
    const bf16* Ws = As + BM * BK;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // ---- LOAD(kt, h) ----
      s16x8 bfrag[FM], afrag[FN];
#pragma unroll
      for (int i = 0; i < FN; ++i) afrag[i] = *fptr(Ws, wn + 16 * i, h);
#pragma unroll
      for (int j = 0; j < FM; ++j) bfrag[j] = *fptr(As, wm + 16 * j, h);
      if (h == 0 && kt + 1 < ktiles) issue(kt + 1);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (h == 1 && grp == 1) wait_vmcnt<0>();     // group 1: own DMA of kt + 1 landed
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // ---- COMPUTE(kt, h) ----
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int j = 0; j < FM; ++j)
#pragma unroll
        for (int i = 0; i < FN; ++i) acc[i][j] = mfma_bf16(afrag[i], bfrag[j], acc[i][j]);
      __builtin_amdgcn_s_setprio(0);
      if (h == 1 && grp == 0) wait_vmcnt<0>();     // group 0: own DMA of kt + 1 landed
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (grp == 0) __builtin_amdgcn_s_barrier();          // re-align the groups' barrier counts
  static_assert(FM == BM / 32, "Gemm6Reg mirrors the m-fragment count");
  if constexpr (Gemm6Reg<TO, BM>::CAN) {
    if (GEMM6_REG_USE(EPI, e)) {
      wide_epilogue_bf16<BM, BN, EPI, FM, FN>(e, acc, smem, M, m0, n0);
      return;
    }
  }
  wide_epilogue<TO, BM, BN, EPI, FM, FN>(e, acc, smem, M, m0, n0);
}

// ------------------------------------------------------------------------------------
// Host side: argument conversion, the tile table, dispatch.
// ------------------------------------------------------------------------------------
int g_gemm_group = 4;    // gemm3 tile order: 0 = row-major, G > 0 = G m-tiles per group (catseg_set_gemm_group); 4 measured best (fc2 48.6 -> 47.4 us)
int g_gemm4_group = 5;   // gemm6 tile order: G m-tiles per group (catseg_set_gemm4_group)
int g_gemm_wide = 1;     // 1 = the automatic choice includes the wide ping-pong tiles (gemm6); 0 = round-5 candidates
int g_gemm_variant = 0;  // 0 = automatic; >0 forces the bf16 tile of TILES with that id (tests / tuning)
int g_gemm_f8_variant = 0;   // the same for the fp8 tiles

RowMap to_rowmap(const CatsegRowMap& m) { return RowMap{m.d1, m.m1, m.s1, m.d2, m.m2, m.s2, m.off}; }
// the map reads row m for every m < M (the kernels' own test, gemm3_kernel `ident`)
bool is_identity(const CatsegRowMap& m, int64_t M) { return m.d1 == 1 && m.m1 >= M && m.s1 == 1 && m.m2 == 1 && m.off == 0; }

// The kernels' view of the epilogue arguments.  pf: the gemm3 / gemm6 launchers pass epi_forms(); gemm_kernel and
// gemm2_kernel (epilogue4) read no form flag.  The fp8 launcher adds its scales.
EpiArgs make_epi(const CatsegGemmArgs* g, int pf = 0) {
  EpiArgs e;
  e.bias = g->bias;
  e.add = g->add; e.ld_add = g->ld_add; e.addmap = to_rowmap(g->addmap); e.add_ncols = g->add_ncols;
  e.act = g->act; e.alpha = g->alpha;
  e.res = g->res; e.ld_res = g->ld_res; e.res2 = g->res2; e.ld_res2 = g->ld_res2;
  e.out = g->out; e.ldo = g->ldo;
  e.store_mode = g->store_mode; e.cvt_k = g->cvt_k; e.cvt_hin = g->cvt_hin; e.cvt_win = g->cvt_win;
  e.cvt_cout = g->cvt_cout;
  e.sa = nullptr; e.sw = nullptr;
  e.pf = pf;
  return e;
}

// EpiArgs::pf from the knobs.  out_bytes = sizeof(TO): an output whose extent does not fit the write-through
// forms' 31-bit byte offset falls to the kernels' plain-store branch
int epi_forms(const CatsegGemmArgs* g, int out_bytes) {
  int pf = (g_epi_prefetch ? EF_PREFETCH : 0) | (g_wide_epi ? EF_WIDE_REG : 0) |
           (g_wide_store == 1 ? EF_WIDE_NT : g_wide_store == 2 ? EF_WIDE_WT : 0) |
           (g_gemm3_store == 1 ? EF_G3_NT : g_gemm3_store == 2 ? EF_G3_WT : 0);
  const int64_t out_elems = g->store_mode == 0 ? g->M * g->ldo : g->M * g->N;   // scatter: M x k x k x cout, dense
  if (!fits_31bit(out_elems, out_bytes)) pf &= ~(EF_WIDE_WT | EF_G3_WT);
  return pf;
}

// The tiles of gemm3_kernel (bf16 and fp8 operands) and gemm6_kernel: the ONLY place that says which
// exist.  The automatic choice, the forced variants (gemm_variant / gemm_fp8_variant = id), the scatter
// restriction, the instantiations and gemm_last all read it.  To add a tile: add a row, with the mask of
// the epilogues it is to be instantiated for.  Ids are test / tool vocabulary, unique per operand type.
enum Family : int { GEMM3, GEMM3_FP8, GEMM6 };
enum : unsigned { E0 = 1, E1 = 2, E2 = 4 };   // EPI 0 = general, 1 = bias (+ res), 2 = bias + QuickGELU
struct Tile {
  int id; Family fam;
  int bm, bn, wgm, wgn, s, bk;   // tile, waves (m x n), ring depth, K-step in 2-byte units (fp8: 2x the fp8 K depth)
  int slots;                     // workgroups per CU
  float w;                       // measured per-CU efficiency for the automatic score; 0 = not an automatic candidate
  unsigned epi;                  // the EPI forms instantiated (E0 | E1 | E2)
  bool sc;                       // also the ConvTranspose scatter form (EPI 0, SC)
};
// Automatic bf16 weights: tools/micro_gemm.py on one box (MG_M for other M).  M = 4616 (bs 8): QKV 224x256
// 35.1 us (hipBLASLt 32.3), fc1 160x128 two per CU 54.2 (256x256: 71.3), out-proj / fc2 160x128 BK=128
// 19.8 / 47.9; M = 2308 (bs 4, config 4): QKV 128x128 8-wave two per CU 22.9 vs 24.2, fc1 160x128 two per
// CU 31.4 (256x256: 47.6), out-proj / fc2 96x128 BK=128 13.9 / 35.2 vs 18.8 / 50.9.  gemm6 (round 6): fc1
// 41.2 us vs 47.3 for 160x128 two per CU, QKV 31.4 vs 33.3 for 224x256; weights from those ratios.
// (Measured and dropped: bf16 160x128 with ring depth 3 / 4, slower on fc2; a one-round 320x256 gemm3 fc1
// tile, 58.4 us vs 54.5; 288x256, 102 us.)  Equal scores keep the earlier row.
constexpr Tile TILES[] = {
    {20, GEMM3, 224, 256, 2, 4, 2, 64, 1, 1.0f, E0 | E1 | E2, false},
    {1, GEMM3, 256, 256, 2, 4, 2, 64, 1, 0.95f, E0, false},
    {15, GEMM3, 160, 128, 2, 4, 2, 128, 1, 0.95f, E0 | E1 | E2, true},
    {17, GEMM3, 160, 128, 2, 4, 2, 64, 2, 0.9f, E0 | E1 | E2, true},
    {19, GEMM3, 128, 128, 2, 4, 2, 64, 2, 0.85f, E0 | E1 | E2, false},
    {24, GEMM3, 96, 128, 2, 4, 2, 128, 1, 0.85f, E0 | E1 | E2, false},
    // the wide ping-pong tiles: lean epilogues only; gemm6_kernel is 2 x 4 waves, 2 slots of BK 64
    {50, GEMM6, 320, 256, 2, 4, 2, 64, 1, 1.1f, E1 | E2, false},
    {51, GEMM6, 320, 192, 2, 4, 2, 64, 1, 1.1f, E1 | E2, false},
    {52, GEMM6, 256, 256, 2, 4, 2, 64, 1, 0.f, E1 | E2, false},
    // fp8 (catseg_gemm_fp8): chosen by launch_f8's own rule, not by score
    {1, GEMM3_FP8, 256, 256, 2, 4, 2, 64, 1, 0.f, E0, false},
    {15, GEMM3_FP8, 160, 128, 2, 4, 2, 128, 1, 0.f, E0 | E1 | E2, false},
    {17, GEMM3_FP8, 160, 128, 2, 4, 2, 64, 2, 0.f, E0 | E1 | E2, false},
    {19, GEMM3_FP8, 128, 128, 2, 4, 2, 64, 2, 0.f, E0, false},
    {20, GEMM3_FP8, 224, 256, 2, 4, 2, 64, 1, 0.f, E0 | E1 | E2, false},
    {21, GEMM3_FP8, 160, 128, 2, 4, 3, 64, 1, 0.f, E0, false},
    {23, GEMM3_FP8, 160, 256, 2, 4, 3, 64, 1, 0.f, E0, false},
    {24, GEMM3_FP8, 160, 256, 2, 4, 2, 64, 1, 0.f, E0, false},
};
constexpr int NTILES = sizeof(TILES) / sizeof(TILES[0]);

// row of the bf16 (gemm3 / gemm6) or fp8 tile `id`, -1 = none
constexpr int find_tile(bool fp8, int id) {
  for (int i = 0; i < NTILES; ++i)
    if ((TILES[i].fam == GEMM3_FP8) == fp8 && TILES[i].id == id) return i;
  return -1;
}

struct Call { const CatsegGemmArgs* g; const float* sa; const float* sw; hipStream_t st; };   // sa / sw: fp8 scales

// gemm3 tile TILES[I].  fp8: g's K / lda / ldw are in fp8 elements (bytes), the kernel sees 2-byte units;
// gemm_last / gemm_last_wt report the bf16 launches only
template <typename TO, int I, int EPI, bool SC>
bool launch3(const Call& c) {
  constexpr Tile T = TILES[I];
  constexpr bool F8 = T.fam == GEMM3_FP8;
  constexpr int U = F8 ? 2 : 1;
  const CatsegGemmArgs* g = c.g;
  if (g->N % T.bn != 0 || (g->K / U) % T.bk != 0) return false;
  EpiArgs e = make_epi(g, epi_forms(g, sizeof(TO)));
  e.sa = c.sa; e.sw = c.sw;
  const int tm = (int)((g->M + T.bm - 1) / T.bm), tn = (int)(g->N / T.bn);
  if constexpr (!F8) {
    g_gemm_last = T.id;
    g_gemm_last_wt = Gemm3Lean<T.bm, T.bn, T.wgm, T.wgn, EPI, SC>::ONE && (e.pf & EF_PREFETCH) && sizeof(TO) == 4 &&
                     !(e.pf & EF_G3_NT) && (e.pf & EF_G3_WT);
  }
  hipLaunchKernelGGL((gemm3_kernel<TO, T.bm, T.bn, T.wgm, T.wgn, T.s, T.bk, F8, SC, EPI>), dim3((unsigned)(tm * tn)),
                     dim3(64 * T.wgm * T.wgn), 0, c.st, (const bf16*)g->A, g->lda / U, to_rowmap(g->amap), (const bf16*)g->W,
                     g->ldw / U, g->M, g->K / U, tn, e, g_gemm_group);
  return true;
}

// the wide ping-pong tile TILES[I] (gemm6): needs an identity A map (32-bit buffer offsets: try_gemm3's wide_ok)
template <typename TO, int I, int EPI>
bool launch6(const Call& c) {
  constexpr Tile T = TILES[I];
  static_assert(T.wgm == 2 && T.wgn == 4 && T.s == 2 && T.bk == 64, "gemm6_kernel's fixed geometry");
  const CatsegGemmArgs* g = c.g;
  if (g->N % T.bn != 0 || g->K % T.bk != 0) return false;
  if (!is_identity(g->amap, g->M)) return false;
  const EpiArgs e = make_epi(g, epi_forms(g, sizeof(TO)));
  const int tm = (int)((g->M + T.bm - 1) / T.bm), tn = (int)(g->N / T.bn);
  g_gemm_last = T.id;
  g_gemm_last_wt = Gemm6Reg<TO, T.bm>::CAN && GEMM6_REG_USE(EPI, e) && !(e.pf & EF_WIDE_NT) && (e.pf & EF_WIDE_WT);
  hipLaunchKernelGGL((gemm6_kernel<TO, T.bm, T.bn, EPI>), dim3((unsigned)(tm * tn)), dim3(512), 0, c.st, (const bf16*)g->A,
                     g->lda, (const bf16*)g->W, g->ldw, g->M, g->K, tn, e, std::max(1, g_gemm4_group));
  return true;
}

// TILES[I] with epilogue EPI (SC: the scatter form); false where the table has no such instantiation
template <typename TO, int I, int EPI, bool SC = false>
bool launch_form(const Call& c) {
  constexpr Tile T = TILES[I];
  if constexpr (SC ? !T.sc : !(T.epi >> EPI & 1)) return false;
  else if constexpr (T.fam == GEMM6) return launch6<TO, I, EPI>(c);
  else return launch3<TO, I, EPI, SC>(c);
}
// a lean epilogue the tile is not instantiated for runs as the general one
template <typename TO, int I>
bool launch_row(const Call& c, int epi, bool scatter) {
  if (scatter) return launch_form<TO, I, 0, true>(c);
  if (!(TILES[I].epi >> epi & 1)) epi = 0;
  return epi == 1 ? launch_form<TO, I, 1>(c) : epi == 2 ? launch_form<TO, I, 2>(c) : launch_form<TO, I, 0>(c);
}
using Rows = std::make_integer_sequence<int, NTILES>;
template <typename TO, int... I>
bool launch_tile(int row, const Call& c, int epi, bool scatter, std::integer_sequence<int, I...>) {
  bool ok = false;
  (void)((row == I && ((ok = launch_row<TO, I>(c, epi, scatter)), true)) || ...);
  return ok;   // row -1 (no such tile): nothing launched
}

// the lean epilogues: 1 = bias (+ res), 2 = bias + QuickGELU, 0 = everything else
int lean_epi(const CatsegGemmArgs* g) {
  const bool plain = !g->add && !g->res2 && g->alpha == 1.f;
  return plain && g->act == ACT_NONE ? 1 : plain && g->act == ACT_QUICKGELU && !g->res ? 2 : 0;
}

// returns true when a gemm3 / gemm6 tile was launched
template <typename TO>
bool try_gemm3(const CatsegGemmArgs* g, hipStream_t st) {
  if (g->K % 32 != 0 || g->lda % 8 != 0 || g->ldw % 8 != 0) return false;
  // 8-wide epilogue: 16-byte aligned output / residual / add rows
  const int vo = sizeof(TO) == 2 ? 8 : 4;
  if (g->ldo % 8 != 0 || ((uintptr_t)g->out % 16) != 0) return false;
  if (g->res && (g->ld_res % 8 != 0 || ((uintptr_t)g->res % 16) != 0)) return false;
  if (g->res2 && (g->ld_res2 % 8 != 0 || ((uintptr_t)g->res2 % 16) != 0)) return false;
  if (g->add && (g->add_ncols % 8 != 0 || g->ld_add % vo != 0 || ((uintptr_t)g->add % 16) != 0)) return false;
  if (g_gemm_variant < 0) return false;
  const bool scatter = g->store_mode != 0;
  int row = find_tile(false, g_gemm_variant);   // a number that names no tile: gemm2_kernel
  if (g_gemm_variant == 0) {
    if (g->M < 1024 || g->K < 256) return false;
    // Tile choice by wave quantization over the 256 CUs: score = fill x w / (1 + 0.15 (rounds - 1)),
    // fill = tiles / (rounds x slots), slots = 256 x workgroups per CU.  The tile never changes the
    // arithmetic: every variant accumulates the full K of an output in the same k order.
    // The ping-pong wide tiles (gemm6) need an identity A map, a lean epilogue and 32-bit buffer offsets.
    const bool wide_ok = g_gemm_wide && is_identity(g->amap, g->M) && lean_epi(g) != 0 && !scatter &&
                         fits_31bit(g->M * g->lda, 2) && fits_31bit(g->N * g->ldw, 2);
    float best = 0.f;
    for (int i = 0; i < NTILES; ++i) {
      const Tile& t = TILES[i];
      if (t.fam == GEMM3_FP8 || t.w == 0.f) continue;
      if (g->N % t.bn != 0 || g->K % t.bk != 0) continue;
      if (t.fam == GEMM6 && !wide_ok) continue;
      const int64_t tiles = ((g->M + t.bm - 1) / t.bm) * (g->N / t.bn), slots = 256LL * t.slots;
      const int64_t rounds = (tiles + slots - 1) / slots;
      const float score = (float)tiles / (float)(rounds * slots) * t.w / (1.f + 0.15f * (float)(rounds - 1));
      if (score > best) { best = score; row = i; }
    }
    if (row < 0) return false;
    if (scatter && !TILES[row].sc) {   // the first tile with the scatter form whose K-step divides K
      row = -1;
      for (int i = 0; i < NTILES && row < 0; ++i)
        if (TILES[i].sc && g->K % TILES[i].bk == 0) row = i;
    }
  }
  return launch_tile<TO>(row, Call{g, nullptr, nullptr, st}, lean_epi(g), scatter, Rows{});
}

// the generic kernels: no tile table, no epilogue forms
template <typename TA, typename TO, int BM, int BN>
void launch(const CatsegGemmArgs* g, hipStream_t st) {
  dim3 grid((unsigned)((g->M + BM - 1) / BM), (unsigned)((g->N + BN - 1) / BN));
  g_gemm_last = 3;
  g_gemm_last_wt = 0;
  hipLaunchKernelGGL((gemm_kernel<TA, TO, BM, BN>), grid, dim3(NT), 0, st, (const TA*)g->A, g->lda, to_rowmap(g->amap),
                     (const TA*)g->W, g->ldw, g->M, g->N, g->K, make_epi(g));
}

template <typename TO, int BM, int BN>
void launch2(const CatsegGemmArgs* g, hipStream_t st) {
  const int tm = (int)((g->M + BM - 1) / BM), tn = (int)((g->N + BN - 1) / BN);
  g_gemm_last = 2;
  g_gemm_last_wt = 0;
  hipLaunchKernelGGL((gemm2_kernel<TO, BM, BN>), dim3((unsigned)(tm * tn)), dim3(NT), 0, st, (const bf16*)g->A,
                     g->lda, to_rowmap(g->amap), (const bf16*)g->W, g->ldw, g->M, g->N, g->K, tn, make_epi(g));
}

template <typename TA, typename TO>
void launch_tiles(const CatsegGemmArgs* g, hipStream_t st) {
  if constexpr (sizeof(TA) == 2) {
    if ((g->store_mode == 0 || g->cvt_cout % 8 == 0) && try_gemm3<TO>(g, st)) return;
    const int64_t t128 = ((g->M + 127) / 128) * ((g->N + 127) / 128);
    if (g->N <= 64) launch2<TO, 128, 64>(g, st);
    else if (t128 < 512) launch2<TO, 64, 128>(g, st);     // fill 256 CUs x 2 slots
    else launch2<TO, 128, 128>(g, st);
  } else {
    // fp32: 64 x 64 tiles when 128 x 128 would leave most CUs idle (the CLIP GEMMs of the training
    // step at M = 4 x 577 / 171 x 12 rows: 68-114 tiles)
    const int64_t t128 = ((g->M + 127) / 128) * ((g->N + 127) / 128);
    if (t128 < 256) launch<TA, TO, 64, 64>(g, st);
    else if (g->N <= 64) launch<TA, TO, 128, 64>(g, st);
    else launch<TA, TO, 128, 128>(g, st);
  }
}

// fp8: the automatic rule is its own (not the bf16 score): one round of <= 256 tiles of the 224x256 or
// the 160x128 BK-128 tile where that fills most CUs, else 160x128 two per CU, else 128x128
template <typename TO>
bool launch_f8(const CatsegGemmArgs* g, const float* sa, const float* sw, hipStream_t st) {
  int id = g_gemm_f8_variant;
  if (id == 0) {
    auto tile = [](int v) -> const Tile& { return TILES[find_tile(true, v)]; };
    auto fits = [&](int v) { return g->N % tile(v).bn == 0 && g->K % (2 * tile(v).bk) == 0; };   // K in fp8 elements
    auto tiles = [&](int v) { return ((g->M + tile(v).bm - 1) / tile(v).bm) * (g->N / tile(v).bn); };
    if (fits(20) && tiles(20) >= 200 && tiles(20) <= 256) id = 20;
    else if (fits(15) && tiles(15) >= 160 && tiles(15) <= 256) id = 15;
    else if (fits(17) && tiles(17) > 256) id = 17;
    else if (fits(19)) id = 19;
    else return false;
  }
  return launch_tile<TO>(find_tile(true, id), Call{g, sa, sw, st}, lean_epi(g), false, Rows{});
}

// the checks catseg_gemm and catseg_gemm_fp8 share (row-map sanity; their alignment rules differ): the
// message to put after the entry point's prefix, nullptr = fine
const char* shared_arg_error(const CatsegGemmArgs* g) {
  auto ok = [](const CatsegRowMap& m) { return m.d1 > 0 && m.m1 > 0 && m.d2 > 0 && m.m2 > 0; };
  return !ok(g->amap) ? "bad amap" : g->add && !ok(g->addmap) ? "bad addmap" : nullptr;
}

}  // namespace

CATSEG_KNOB(g_gemm_variant, "gemm_variant");
CATSEG_KNOB(g_gemm_wide, "gemm_wide");
CATSEG_KNOB(g_gemm_group, "gemm_group");
CATSEG_KNOB(g_gemm4_group, "gemm4_group");
CATSEG_KNOB(g_epi_prefetch, "epi_prefetch");
CATSEG_KNOB(g_wide_epi, "wide_epi");
CATSEG_KNOB(g_wide_store, "wide_store");
CATSEG_KNOB(g_gemm3_store, "gemm3_store");
CATSEG_KNOB(g_gemm_last, "gemm_last");
CATSEG_KNOB(g_gemm_last_wt, "gemm_last_wt");
CATSEG_KNOB(g_gemm_f8_variant, "gemm_fp8_variant");

extern "C" int catseg_gemm_fp8(const CatsegGemmArgs* g, const float* scale_a, const float* scale_w, void* stream) {
  CATSEG_CHECK(g && g->A && g->W && g->out && scale_a && scale_w, "gemm_fp8: null pointer");
  CATSEG_CHECK(g->dtype_a == CATSEG_FP8, "gemm_fp8: dtype_a must be CATSEG_FP8");
  CATSEG_CHECK(g->M > 0 && g->N > 0 && g->K > 0, "gemm_fp8: empty shape");
  CATSEG_CHECK(g->K % 128 == 0 && g->lda % 16 == 0 && g->ldw % 16 == 0, "gemm_fp8: K must be a multiple of 128, lda/ldw of 16");
  CATSEG_CHECK(g->N % 128 == 0, "gemm_fp8: N must be a multiple of 128");
  CATSEG_CHECK(((uintptr_t)g->A % 16) == 0 && ((uintptr_t)g->W % 16) == 0 && ((uintptr_t)scale_w % 16) == 0,
               "gemm_fp8: A/W/scale_w must be 16B aligned");
  CATSEG_CHECK(g->store_mode == 0, "gemm_fp8: row-major store only");
  CATSEG_CHECK(g->ldo % 8 == 0 && ((uintptr_t)g->out % 16) == 0, "gemm_fp8: out rows must be 16B aligned");
  CATSEG_CHECK(!g->res || (g->ld_res % 8 == 0 && ((uintptr_t)g->res % 16) == 0), "gemm_fp8: res rows must be 16B aligned");
  CATSEG_CHECK(!g->res2 || (g->ld_res2 % 8 == 0 && ((uintptr_t)g->res2 % 16) == 0), "gemm_fp8: res2 rows must be 16B aligned");
  CATSEG_CHECK(!g->add || (g->add_ncols % 8 == 0 && g->ld_add % 8 == 0 && ((uintptr_t)g->add % 16) == 0),
               "gemm_fp8: add rows must be 16B aligned");
  if (const char* m = shared_arg_error(g)) { catseg_set_error("gemm_fp8: %s", m); return CATSEG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  bool ok;
  if (g->dtype_out == CATSEG_BF16) ok = launch_f8<bf16>(g, scale_a, scale_w, st);
  else if (g->dtype_out == CATSEG_F32) ok = launch_f8<float>(g, scale_a, scale_w, st);
  else CATSEG_FAIL("gemm_fp8: dtype_out must be f32 or bf16");
  CATSEG_CHECK(ok, "gemm_fp8: no tile fits this shape / variant");
  return catseg_launch_status("gemm_fp8");
}

extern "C" int catseg_gemm(const CatsegGemmArgs* g, void* stream) {
  CATSEG_CHECK(g && g->A && g->W && g->out, "gemm: null pointer");
  CATSEG_CHECK(g->M > 0 && g->N > 0 && g->K > 0, "gemm: empty shape");
  CATSEG_CHECK(g->N % 4 == 0, "gemm: N must be a multiple of 4");
  const int va = g->dtype_a == CATSEG_BF16 ? 8 : 4;
  CATSEG_CHECK(g->K % va == 0 && g->lda % va == 0 && g->ldw % va == 0,
               "gemm: K/lda/ldw must be multiples of 16 bytes");
  CATSEG_CHECK(((uintptr_t)g->A % 16) == 0 && ((uintptr_t)g->W % 16) == 0, "gemm: A/W must be 16B aligned");
  CATSEG_CHECK(g->ldo % 4 == 0, "gemm: ldo must be a multiple of 4");
  CATSEG_CHECK(!g->add || g->ld_add % 4 == 0, "gemm: ld_add must be a multiple of 4");
  CATSEG_CHECK(g->store_mode == 0 || (g->cvt_cout % 4 == 0 && g->cvt_k > 0 && g->cvt_hin > 0 && g->cvt_win > 0),
               "gemm: bad ConvTranspose scatter geometry");
  CATSEG_CHECK(g->store_mode == 0 || g->N == (int64_t)g->cvt_k * g->cvt_k * g->cvt_cout,
               "gemm: ConvTranspose N must be k*k*cout");
  CATSEG_CHECK(g->store_mode == 0 || g->M < (1LL << 31), "gemm: ConvTranspose row count must fit 31 bits");
  if (const char* m = shared_arg_error(g)) { catseg_set_error("gemm: %s", m); return CATSEG_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  if (g->dtype_a == CATSEG_BF16 && g->dtype_out == CATSEG_BF16) launch_tiles<bf16, bf16>(g, st);
  else if (g->dtype_a == CATSEG_BF16 && g->dtype_out == CATSEG_F32) launch_tiles<bf16, float>(g, st);
  else if (g->dtype_a == CATSEG_F32 && g->dtype_out == CATSEG_F32) launch_tiles<float, float>(g, st);
  else if (g->dtype_a == CATSEG_F32 && g->dtype_out == CATSEG_BF16) launch_tiles<float, bf16>(g, st);
  else CATSEG_FAIL("gemm: unsupported dtype combination");
  return catseg_launch_status("gemm");
}
