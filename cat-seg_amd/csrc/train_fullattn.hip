// Training forward and backward of ATTENTION_TYPE "full" in the class aggregation: FullAttention (reference
// cat_seg/modeling/transformer/model.py:289-320) over every pixel's T classes plus the n_pad learned
// padding tokens (model.py:397-410), in the head's class-major row layout, fp32.
//
// catseg_full_attention_backward — token t of sequence (b, p) is row (b*T + t)*HW + p of q / k / v / dy
//   (no packed sequence-major copy); head h at columns 32 h .. 32 h + 31.  The n_pad padding keys are
//   identical rows (k_pad, v_pad) whose outputs the reference discards (model.py:419-421): one extra
//   key column of multiplicity n_pad in every softmax row, no padding queries.  Nothing is kept from
//   the forward: the softmax statistics are recomputed from q, k, v.
//
//   One workgroup of 4 waves per (pixel, head).  The sequence streams through two LDS tiles in blocks
//   of 64 rows (rows past T staged as zeros and masked, never read); a wave owns up to two 16-row
//   tiles per round of 128 rows:
//     pass Q  waves own QUERY tiles (Q, dY rows in registers), K / V blocks stream:
//       sweep 1  online softmax max m, sum l and D = sum_j P_ij dP_ij (the pad column joins after the
//                sweep); m, 1/l, D and the pad column's n_pad P_i*, n_pad dS_i* go to an LDS table
//       sweep 2  dQ += dS K, then + n_pad dS_i* k_pad, times scale
//     pass K  waves own KEY tiles (K, V rows in registers), Q / dY blocks stream:
//       dV += P^T dY, dK += scale dS^T Q; in the first round every thread also sums its share of
//       sum_i n_pad dS_i* q_i and sum_i n_pad P_i* dy_i, written per (pixel, head) to the workspace
//   and full_pad_reduce_kernel sums the workspace over pixels in a fixed order into dk_pad / dv_pad.
//   Every product is an exact-f32 MFMA (16x16x4), operand conventions of train_attn.hip: an
//   accumulator tile's 4 registers are the next MFMA's A operand for 4 k-steps.  Every dq / dk / dv
//   element is owned by one wave: no atomics, bit-reproducible.
#include "common.h"
#include "capi.h"
#include "catseg_hip_train.h"

namespace {

constexpr int FD = 32;          // head_dim
constexpr int FH = 4;           // heads
constexpr int FP = FD + 4;      // LDS row pitch (floats): 16-byte aligned rows; the [4g + j][16e + r] reads conflict-free
constexpr int FB = 64;          // rows per staged block
constexpr int NQ = 2;           // 16-row tiles a wave owns per round
constexpr int FTMAX = 2048;     // the statistics table (5 floats per row) stays within 64 KB of LDS with the tiles

struct FullP {
  const float* q; const float* k; const float* v; int64_t ld_qkv;
  const float* dy; int64_t ld_dy;
  float* dq; float* dk; float* dv; int64_t ld_dqkv;
  int T, HW, n_pad; float scale;
  const float* k_pad; const float* v_pad;
  float* padpart;                // [B*HW][256]: d k_pad | d v_pad partials per pixel
};

// stage rows t0 .. t0 + 63 (head columns) of `src` into tile[64][FP]; token t is row base + t * HW
DEV void stage_block(float* tile, const float* src, int64_t ld, int64_t base, int HW, int t0, int T, int col) {
  for (int e = threadIdx.x; e < FB * (FD / 4); e += 256) {
    const int i = e / (FD / 4), c = (e % (FD / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + i < T) v = *reinterpret_cast<const float4*>(src + (base + (int64_t)(t0 + i) * HW) * ld + col + c);
    *reinterpret_cast<float4*>(tile + i * FP + c) = v;
  }
}

__global__ __launch_bounds__(256) void full_attn_bwd_kernel(FullP p) {
  __shared__ __attribute__((aligned(16))) float tA[FB * FP];
  __shared__ __attribute__((aligned(16))) float tB[FB * FP];
  extern __shared__ __attribute__((aligned(16))) float stat[];     // 5 x Tp: m, 1/l, D, n_pad P*, n_pad dS*
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int T = p.T, HW = p.HW;
  const int NT = (T + 15) / 16, Tp = NT * 16;
  float* stM = stat;
  float* stL = stat + Tp;
  float* stD = stat + 2 * Tp;
  float* stPp = stat + 3 * Tp;
  float* stPd = stat + 4 * Tp;
  const int64_t seq = blockIdx.x / FH;              // (b, p)
  const int h = (int)(blockIdx.x % FH), col = h * FD;
  const int64_t b = seq / HW, pp = seq % HW;
  const int64_t base = b * T * HW + pp;             // row of token 0
  const float scale = p.scale;
  const bool pad = p.n_pad > 0;
  const float fpad = (float)p.n_pad;
  const int rounds = (NT + 4 * NQ - 1) / (4 * NQ);

  // the pad column's k / v as B-operand fragments: [4 t + g]
  float kpf[FD / 4], vpf[FD / 4];
#pragma unroll
  for (int t = 0; t < FD / 4; ++t) {
    kpf[t] = pad ? p.k_pad[col + 4 * t + g] : 0.f;
    vpf[t] = pad ? p.v_pad[col + 4 * t + g] : 0.f;
  }

  // ------------------------------------------------------------------ pass Q: waves own query tiles
  for (int rd = 0; rd < rounds; ++rd) {
    int qt[NQ];
    bool on[NQ];
    float qf[NQ][FD / 4], of[NQ][FD / 4];
    float spad[NQ], dppad[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      qt[u] = (rd * NQ + u) * 4 + wave;
      on[u] = qt[u] < NT;                            // wave-uniform
      const int qi = qt[u] * 16 + r;
      const bool ok = on[u] && qi < T;
      const int64_t row = base + (int64_t)(ok ? qi : 0) * HW;
      float sp = 0.f, dp = 0.f;
#pragma unroll
      for (int t = 0; t < FD / 4; ++t) {
        qf[u][t] = ok ? p.q[row * p.ld_qkv + col + 4 * t + g] : 0.f;
        of[u][t] = ok ? p.dy[row * p.ld_dy + col + 4 * t + g] : 0.f;
        sp += qf[u][t] * kpf[t];
        dp += of[u][t] * vpf[t];
      }
      spad[u] = scale * xrow4_sum(sp);               // s_i* = scale q_i . k_pad
      dppad[u] = xrow4_sum(dp);                      // dP_i* = dy_i . v_pad
    }

    // ---- sweep 1: softmax statistics and D (S^T / dP^T tiles: lane column = query) ----
    float m_l[NQ], l_l[NQ], d_l[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) { m_l[u] = -INFINITY; l_l[u] = 0.f; d_l[u] = 0.f; }
    for (int kb = 0; kb < T; kb += FB) {
      __syncthreads();
      stage_block(tA, p.k, p.ld_qkv, base, HW, kb, T, col);
      stage_block(tB, p.v, p.ld_qkv, base, HW, kb, T, col);
      __syncthreads();
      for (int kt = 0; kt < FB / 16 && kb + kt * 16 < T; ++kt) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (!on[u]) continue;
          f32x4 sa = f32x4{0.f, 0.f, 0.f, 0.f}, pa = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < FD / 4; ++t) {
            sa = mfma_f32(tA[(kt * 16 + r) * FP + 4 * t + g], qf[u][t], sa);   // S^T[key][q]
            pa = mfma_f32(tB[(kt * 16 + r) * FP + 4 * t + g], of[u][t], pa);   // dP^T[key][q]
          }
          float sc[4], tm = -INFINITY;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = kb + kt * 16 + 4 * g + j;
            sc[j] = key < T ? scale * sa[j] : -INFINITY;
            tm = fmaxf(tm, sc[j]);
          }
          const float mn = fmaxf(m_l[u], tm);
          if (mn != -INFINITY) {
            float add = 0.f, dadd = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float e = __expf(sc[j] - mn);
              add += e;
              dadd += e * pa[j];
            }
            const float f = __expf(m_l[u] - mn);
            l_l[u] = l_l[u] * f + add;
            d_l[u] = d_l[u] * f + dadd;
            m_l[u] = mn;
          }
        }
      }
    }
    float mq[NQ], lq[NQ], Dq[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      mq[u] = 0.f; lq[u] = 0.f; Dq[u] = 0.f;
      if (!on[u]) continue;
      float M = xrow4_max(m_l[u]);                   // finite: key 0 is unmasked for every query
      if (pad) M = fmaxf(M, spad[u]);
      const float f = m_l[u] == -INFINITY ? 0.f : __expf(m_l[u] - M);
      float Lsum = xrow4_sum(l_l[u] * f);
      float Dsum = xrow4_sum(d_l[u] * f);
      float ep = 0.f;
      if (pad) {
        ep = fpad * __expf(spad[u] - M);             // the pad column, n_pad copies
        Lsum += ep;
        Dsum += ep * dppad[u];
      }
      const int qi = qt[u] * 16 + r;
      const bool ok = qi < T;
      const float linv = ok ? 1.f / Lsum : 0.f;
      mq[u] = ok ? M : 0.f;
      lq[u] = linv;
      Dq[u] = ok ? Dsum * linv : 0.f;
      const float Pp = ep * linv;                    // n_pad P_i*
      if (g == 0) {
        stM[qi] = mq[u];
        stL[qi] = lq[u];
        stD[qi] = Dq[u];
        stPp[qi] = Pp;
        stPd[qi] = Pp * (dppad[u] - Dq[u]);          // n_pad dS_i*
      }
    }

    // ---- sweep 2: dQ = scale (dS K + n_pad dS* k_pad) ----
    f32x4 dQ[NQ][2];
#pragma unroll
    for (int u = 0; u < NQ; ++u) { dQ[u][0] = f32x4{0.f, 0.f, 0.f, 0.f}; dQ[u][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kb = 0; kb < T; kb += FB) {
      __syncthreads();
      stage_block(tA, p.k, p.ld_qkv, base, HW, kb, T, col);
      stage_block(tB, p.v, p.ld_qkv, base, HW, kb, T, col);
      __syncthreads();
      for (int kt = 0; kt < FB / 16 && kb + kt * 16 < T; ++kt) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (!on[u]) continue;
          f32x4 sa = f32x4{0.f, 0.f, 0.f, 0.f}, pa = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < FD / 4; ++t) {
            sa = mfma_f32(tA[(kt * 16 + r) * FP + 4 * t + g], qf[u][t], sa);   // S^T[key][q]
            pa = mfma_f32(tB[(kt * 16 + r) * FP + 4 * t + g], of[u][t], pa);   // dP^T[key][q]
          }
          float dS[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = kb + kt * 16 + 4 * g + j;
            dS[j] = key < T ? __expf(scale * sa[j] - mq[u]) * lq[u] * (pa[j] - Dq[u]) : 0.f;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int kl = kt * 16 + 4 * g + j;
#pragma unroll
            for (int e = 0; e < 2; ++e) dQ[u][e] = mfma_f32(dS[j], tA[kl * FP + 16 * e + r], dQ[u][e]);
          }
        }
      }
    }
    // lane holds rows q = qt*16 + 4g + j, column d = 16e + r; the pad term through the LDS table
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      if (!on[u]) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qq = qt[u] * 16 + 4 * g + j;
        if (qq >= T) continue;
        const float pd = pad ? stPd[qq] : 0.f;
        const int64_t row = base + (int64_t)qq * HW;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const float kp = pad ? p.k_pad[col + 16 * e + r] : 0.f;
          p.dq[row * p.ld_dqkv + col + 16 * e + r] = scale * (dQ[u][e][j] + pd * kp);
        }
      }
    }
  }

  // ------------------------------------------------------------------ pass K: waves own key tiles
  // pad partials: thread -> column d of d k_pad (which = 0) or d v_pad (which = 1), rows 16 wave .. + 15 of a block
  const int pd_d = tid & 31, pd_which = (tid >> 5) & 1;
  float padacc = 0.f;
  for (int rd = 0; rd < rounds; ++rd) {
    int kt0[NQ];
    bool on[NQ];
    float kf[NQ][FD / 4], vf[NQ][FD / 4];
    f32x4 dV[NQ][2], dK[NQ][2];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      kt0[u] = ((rd * NQ + u) * 4 + wave) * 16;
      on[u] = kt0[u] < T;                            // wave-uniform
      const int key = kt0[u] + r;
      const bool ok = on[u] && key < T;
      const int64_t row = base + (int64_t)(ok ? key : 0) * HW;
#pragma unroll
      for (int t = 0; t < FD / 4; ++t) {
        kf[u][t] = ok ? p.k[row * p.ld_qkv + col + 4 * t + g] : 0.f;
        vf[u][t] = ok ? p.v[row * p.ld_qkv + col + 4 * t + g] : 0.f;
      }
#pragma unroll
      for (int e = 0; e < 2; ++e) { dV[u][e] = f32x4{0.f, 0.f, 0.f, 0.f}; dK[u][e] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }
    for (int qb = 0; qb < T; qb += FB) {
      __syncthreads();                               // also orders pass Q's table writes before the reads below
      stage_block(tA, p.q, p.ld_qkv, base, HW, qb, T, col);
      stage_block(tB, p.dy, p.ld_dy, base, HW, qb, T, col);
      __syncthreads();
      if (pad && rd == 0) {
        const float* tile = pd_which ? tB : tA;
        const float* w = pd_which ? stPp : stPd;
#pragma unroll 4
        for (int i = wave * 16; i < wave * 16 + 16; ++i)
          if (qb + i < T) padacc += w[qb + i] * tile[i * FP + pd_d];
      }
      for (int qs = 0; qs < FB / 16 && qb + qs * 16 < T; ++qs) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (!on[u]) continue;
          const int key = kt0[u] + r;
          f32x4 sa = f32x4{0.f, 0.f, 0.f, 0.f}, pa = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int t = 0; t < FD / 4; ++t) {
            sa = mfma_f32(tA[(qs * 16 + r) * FP + 4 * t + g], kf[u][t], sa);   // S[q][key]
            pa = mfma_f32(tB[(qs * 16 + r) * FP + 4 * t + g], vf[u][t], pa);   // dP[q][key]
          }
          float P[4], dS[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int qq = qb + qs * 16 + 4 * g + j;
            P[j] = (qq < T && key < T) ? __expf(scale * sa[j] - stM[qq]) * stL[qq] : 0.f;
            dS[j] = P[j] * (pa[j] - stD[qq]);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ql = qs * 16 + 4 * g + j;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
              dV[u][e] = mfma_f32(P[j], tB[ql * FP + 16 * e + r], dV[u][e]);
              dK[u][e] = mfma_f32(dS[j], tA[ql * FP + 16 * e + r], dK[u][e]);
            }
          }
        }
      }
    }
    // lane holds rows key = kt0 + 4g + j, column d = 16e + r
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      if (!on[u]) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int kk = kt0[u] + 4 * g + j;
        if (kk >= T) continue;
        const int64_t row = base + (int64_t)kk * HW;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          p.dv[row * p.ld_dqkv + col + 16 * e + r] = dV[u][e][j];
          p.dk[row * p.ld_dqkv + col + 16 * e + r] = scale * dK[u][e][j];
        }
      }
    }
  }

  // the pad partials of this (pixel, head): the 4 waves' shares in wave order
  if (pad) {
    __syncthreads();
    tA[tid] = padacc;
    __syncthreads();
    if (tid < 64) {
      const float s = ((tA[tid] + tA[64 + tid]) + tA[128 + tid]) + tA[192 + tid];
      p.padpart[seq * 256 + pd_which * 128 + col + pd_d] = pd_which ? s : scale * s;
    }
  }
}

// ------------------------------------------------------------------ training forward
// y = x + softmax(scale q k^T) v on the same rows, for the training step only.  The synthesized and the
// trained heads give peaked softmax rows (|score| of tens), where fp32 rounding of a score is multiplied
// by the exponential and the gradients of the whole step amplify it; here the scores are exact: q . k on
// the f64 MFMA (v_mfma_f64_16x16x4_f64; products of fp32 values are exact in f64), the exponent
// s - m formed in f64 and rounded once.  The padding keys are one more staged key row (index T) whose
// weight in the row sum and in P is n_pad.  Two sweeps per query tile (max / sum, then P V with the
// final statistics): no accumulator rescale, and P needs no second layout (its C/D rows g + 4 j of the
// f64 tile are the k-steps of the fp32 P V product, the V rows read in the same order).
typedef double f64x4 __attribute__((ext_vector_type(4)));

struct FullF {
  const float* q; const float* k; const float* v; int64_t ld_qkv;
  const float* x; float* y; int64_t ld_xy;
  int T, HW, n_pad; float scale;
  const float* k_pad; const float* v_pad;
};

// as stage_block, with the pad row (k_pad / v_pad) as token T when n_pad > 0
DEV void stage_block_pad(float* tile, const float* src, const float* padrow, int64_t ld, int64_t base, int HW, int t0,
                         int T, int col) {
  for (int e = threadIdx.x; e < FB * (FD / 4); e += 256) {
    const int i = e / (FD / 4), c = (e % (FD / 4)) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t0 + i < T) v = *reinterpret_cast<const float4*>(src + (base + (int64_t)(t0 + i) * HW) * ld + col + c);
    else if (t0 + i == T && padrow)
      v = make_float4(padrow[col + c], padrow[col + c + 1], padrow[col + c + 2], padrow[col + c + 3]);
    *reinterpret_cast<float4*>(tile + i * FP + c) = v;
  }
}

__global__ __launch_bounds__(256) void full_attn_train_fwd_kernel(FullF p) {
  __shared__ __attribute__((aligned(16))) float tA[FB * FP];
  __shared__ __attribute__((aligned(16))) float tB[FB * FP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int T = p.T, HW = p.HW;
  const bool pad = p.n_pad > 0;
  const int TK = T + (pad ? 1 : 0);                 // staged keys: the classes, then the pad row
  const int NT = (T + 15) / 16;
  const int64_t seq = blockIdx.x / FH;
  const int h = (int)(blockIdx.x % FH), col = h * FD;
  const int64_t b = seq / HW, pp = seq % HW;
  const int64_t base = b * T * HW + pp;
  const double scale = (double)p.scale;
  const float fpad = (float)p.n_pad;
  const float* kpr = pad ? p.k_pad : nullptr;
  const float* vpr = pad ? p.v_pad : nullptr;
  const int rounds = (NT + 4 * NQ - 1) / (4 * NQ);

  for (int rd = 0; rd < rounds; ++rd) {
    int qt[NQ];
    bool on[NQ];
    double qf[NQ][FD / 4];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      qt[u] = (rd * NQ + u) * 4 + wave;
      on[u] = qt[u] < NT;                            // wave-uniform
      const int qi = qt[u] * 16 + r;
      const bool ok = on[u] && qi < T;
      const int64_t row = base + (int64_t)(ok ? qi : 0) * HW;
#pragma unroll
      for (int t = 0; t < FD / 4; ++t) qf[u][t] = ok ? (double)p.q[row * p.ld_qkv + col + 4 * t + g] : 0.0;
    }
    // ---- sweep 1: max and weighted sum per query (lane column = query, rows = keys g + 4 j) ----
    float m_l[NQ], l_l[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) { m_l[u] = -INFINITY; l_l[u] = 0.f; }
    for (int kb = 0; kb < TK; kb += FB) {
      __syncthreads();
      stage_block_pad(tA, p.k, kpr, p.ld_qkv, base, HW, kb, T, col);
      __syncthreads();
      for (int kt = 0; kt < FB / 16 && kb + kt * 16 < TK; ++kt) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (!on[u]) continue;
          f64x4 sa = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int t = 0; t < FD / 4; ++t)
            sa = __builtin_amdgcn_mfma_f64_16x16x4f64((double)tA[(kt * 16 + r) * FP + 4 * t + g], qf[u][t], sa, 0, 0, 0);
          float tm = -INFINITY;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = kb + kt * 16 + g + 4 * j;
            if (key < TK) tm = fmaxf(tm, (float)(scale * sa[j]));
          }
          const float mn = fmaxf(m_l[u], tm);
          if (mn != -INFINITY) {
            float add = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int key = kb + kt * 16 + g + 4 * j;
              const float w = key < T ? 1.f : (key < TK ? fpad : 0.f);
              add += key < TK ? w * __expf((float)(scale * sa[j] - (double)mn)) : 0.f;
            }
            l_l[u] = l_l[u] * __expf(m_l[u] - mn) + add;
            m_l[u] = mn;
          }
        }
      }
    }
    float mq[NQ], lq[NQ];
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      mq[u] = 0.f; lq[u] = 0.f;
      if (!on[u]) continue;
      const float M = xrow4_max(m_l[u]);             // finite: key 0 is unmasked
      const float f = m_l[u] == -INFINITY ? 0.f : __expf(m_l[u] - M);
      const float Lsum = xrow4_sum(l_l[u] * f);
      mq[u] = M;
      lq[u] = 1.f / Lsum;
    }
    // ---- sweep 2: O = P V with the final statistics ----
    f32x4 O[NQ][2];
#pragma unroll
    for (int u = 0; u < NQ; ++u) { O[u][0] = f32x4{0.f, 0.f, 0.f, 0.f}; O[u][1] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    for (int kb = 0; kb < TK; kb += FB) {
      __syncthreads();
      stage_block_pad(tA, p.k, kpr, p.ld_qkv, base, HW, kb, T, col);
      stage_block_pad(tB, p.v, vpr, p.ld_qkv, base, HW, kb, T, col);
      __syncthreads();
      for (int kt = 0; kt < FB / 16 && kb + kt * 16 < TK; ++kt) {
#pragma unroll
        for (int u = 0; u < NQ; ++u) {
          if (!on[u]) continue;
          f64x4 sa = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int t = 0; t < FD / 4; ++t)
            sa = __builtin_amdgcn_mfma_f64_16x16x4f64((double)tA[(kt * 16 + r) * FP + 4 * t + g], qf[u][t], sa, 0, 0, 0);
          float P[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int key = kb + kt * 16 + g + 4 * j;
            const float w = key < T ? 1.f : (key < TK ? fpad : 0.f);
            P[j] = key < TK ? w * __expf((float)(scale * sa[j] - (double)mq[u])) * lq[u] : 0.f;
          }
          // P[j] at lane (r, g): query r, key 4 j + g -> A operand of k-step j; V rows in that order
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int kl = kt * 16 + 4 * j + g;
#pragma unroll
            for (int e = 0; e < 2; ++e) O[u][e] = mfma_f32(P[j], tB[kl * FP + 16 * e + r], O[u][e]);
          }
        }
      }
    }
    // lane holds rows q = qt*16 + 4g + j, column d = 16e + r
#pragma unroll
    for (int u = 0; u < NQ; ++u) {
      if (!on[u]) continue;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int qq = qt[u] * 16 + 4 * g + j;
        if (qq >= T) continue;
        const int64_t row = base + (int64_t)qq * HW;
#pragma unroll
        for (int e = 0; e < 2; ++e)
          p.y[row * p.ld_xy + col + 16 * e + r] = p.x[row * p.ld_xy + col + 16 * e + r] + O[u][e][j];
      }
    }
  }
}

// d k_pad / d v_pad = sum over pixels (fixed order)
__global__ __launch_bounds__(256) void full_pad_reduce_kernel(const float* __restrict__ part, int64_t npix,
                                                              float* __restrict__ dk_pad, float* __restrict__ dv_pad) {
  const int c = threadIdx.x;
  float s = 0.f;
  for (int64_t i = 0; i < npix; ++i) s += part[i * 256 + c];
  if (c < 128) dk_pad[c] = s;
  else dv_pad[c - 128] = s;
}

}  // namespace

extern "C" int64_t catseg_full_attention_backward_workspace(int64_t B, int T, int HW, int n_heads, int n_pad) {
  return B > 0 && T > 0 && HW > 0 && n_heads > 0 && n_pad > 0 ? B * HW * 256 * (int64_t)sizeof(float) : 0;
}

extern "C" int catseg_full_attention_backward(const CatsegFullAttnBwdArgs* a, void* stream) {
  CATSEG_CHECK(a && a->q && a->k && a->v && a->dy && a->dq && a->dk && a->dv, "full_attention_backward: null");
  CATSEG_CHECK(a->n_heads == FH && a->head_dim == FD, "full_attention_backward: 4 heads x 32 only");
  CATSEG_CHECK(a->B > 0 && a->T > 0 && a->HW > 0 && a->n_pad >= 0, "full_attention_backward: bad shape");
  CATSEG_CHECK(a->T <= FTMAX, "full_attention_backward: at most 2048 classes");
  CATSEG_CHECK(a->ld_qkv >= FH * FD && a->ld_dy >= FH * FD && a->ld_dqkv >= FH * FD,
               "full_attention_backward: row strides too small");
  CATSEG_CHECK(a->ld_qkv % 4 == 0 && a->ld_dy % 4 == 0 && a->ld_dqkv % 4 == 0, "full_attention_backward: strides % 4");
  CATSEG_CHECK((uintptr_t)a->q % 16 == 0 && (uintptr_t)a->k % 16 == 0 && (uintptr_t)a->v % 16 == 0 &&
               (uintptr_t)a->dy % 16 == 0, "full_attention_backward: q / k / v / dy must be 16-byte aligned");
  CATSEG_CHECK(a->n_pad == 0 || (a->k_pad && a->v_pad && a->dk_pad && a->dv_pad), "full_attention_backward: pad args");
  const int64_t npix = a->B * a->HW;
  CATSEG_CHECK(npix * FH < (1LL << 31), "full_attention_backward: too many (pixel, head) pairs");
  if (a->n_pad > 0)
    CATSEG_CHECK(a->workspace && a->workspace_bytes >= npix * 256 * (int64_t)sizeof(float),
                 "full_attention_backward: workspace too small");
  FullP p;
  p.q = (const float*)a->q; p.k = (const float*)a->k; p.v = (const float*)a->v; p.ld_qkv = a->ld_qkv;
  p.dy = (const float*)a->dy; p.ld_dy = a->ld_dy;
  p.dq = (float*)a->dq; p.dk = (float*)a->dk; p.dv = (float*)a->dv; p.ld_dqkv = a->ld_dqkv;
  p.T = a->T; p.HW = a->HW; p.n_pad = a->n_pad; p.scale = a->scale;
  p.k_pad = a->k_pad; p.v_pad = a->v_pad;
  p.padpart = (float*)a->workspace;
  hipStream_t st = (hipStream_t)stream;
  const size_t table = (size_t)5 * ((a->T + 15) / 16 * 16) * sizeof(float);
  hipLaunchKernelGGL(full_attn_bwd_kernel, dim3((unsigned)(npix * FH)), dim3(256), table, st, p);
  if (a->n_pad > 0)
    hipLaunchKernelGGL(full_pad_reduce_kernel, dim3(1), dim3(256), 0, st, (const float*)a->workspace, npix, a->dk_pad,
                       a->dv_pad);
  return catseg_launch_status("full_attention_backward");
}

extern "C" int catseg_full_attention_train_forward(const CatsegFullAttnTrainFwdArgs* a, void* stream) {
  CATSEG_CHECK(a && a->q && a->k && a->v && a->x && a->y, "full_attention_train_forward: null");
  CATSEG_CHECK(a->n_heads == FH && a->head_dim == FD, "full_attention_train_forward: 4 heads x 32 only");
  CATSEG_CHECK(a->B > 0 && a->T > 0 && a->HW > 0 && a->n_pad >= 0, "full_attention_train_forward: bad shape");
  CATSEG_CHECK(a->ld_qkv >= FH * FD && a->ld_xy >= FH * FD, "full_attention_train_forward: row strides too small");
  CATSEG_CHECK(a->ld_qkv % 4 == 0, "full_attention_train_forward: strides % 4");
  CATSEG_CHECK((uintptr_t)a->q % 16 == 0 && (uintptr_t)a->k % 16 == 0 && (uintptr_t)a->v % 16 == 0,
               "full_attention_train_forward: q / k / v must be 16-byte aligned");
  CATSEG_CHECK(a->n_pad == 0 || (a->k_pad && a->v_pad), "full_attention_train_forward: pad args");
  const int64_t npix = a->B * a->HW;
  CATSEG_CHECK(npix * FH < (1LL << 31), "full_attention_train_forward: too many (pixel, head) pairs");
  FullF p;
  p.q = (const float*)a->q; p.k = (const float*)a->k; p.v = (const float*)a->v; p.ld_qkv = a->ld_qkv;
  p.x = (const float*)a->x; p.y = (float*)a->y; p.ld_xy = a->ld_xy;
  p.T = a->T; p.HW = a->HW; p.n_pad = a->n_pad; p.scale = a->scale;
  p.k_pad = a->k_pad; p.v_pad = a->v_pad;
  hipLaunchKernelGGL(full_attn_train_fwd_kernel, dim3((unsigned)(npix * FH)), dim3(256), 0, (hipStream_t)stream, p);
  return catseg_launch_status("full_attention_train_forward");
}
