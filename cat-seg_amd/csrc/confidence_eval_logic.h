// The per-pixel index logic of the calibration counters (confidence_eval.hip), as host + device functions, so
// that a host program can run the very same bin and rounding code over the edge values.  The contract is
// DESIGN.md section 4 ("Confidence outputs") and include/catseg_hip_confidence.h.
//
// Counter block of one (n_bins, K): count[n_bins], correct[n_bins], conf_q24[n_bins], hit[K], valid, nan.
// Everything after the bin and the Q24 rounding is integer, so the counters are a function of the input.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CE_HD __host__ __device__ inline
#else
#define CE_HD inline
#endif

constexpr int CE_MAX_BINS = 256;                   // n_bins
constexpr int CE_MAX_K = 4;                        // ranks of the top-k maps

CE_HD int64_t ce_counters(int64_t n_bins, int64_t K) { return 3 * n_bins + K + 2; }
CE_HD int ce_off_count(int) { return 0; }
CE_HD int ce_off_correct(int n_bins) { return n_bins; }
CE_HD int ce_off_q24(int n_bins) { return 2 * n_bins; }
CE_HD int ce_off_hit(int n_bins) { return 3 * n_bins; }
CE_HD int ce_off_valid(int n_bins, int K) { return 3 * n_bins + K; }
CE_HD int ce_off_nan(int n_bins, int K) { return 3 * n_bins + K + 1; }

// labels >= clamp fold to clamp (clamp < 0: no fold), as confusion_labels_kernel (evaluate.hip)
CE_HD int ce_fold(int label, int clamp) { return (clamp >= 0 && label >= clamp) ? clamp : label; }

// NaN on the bits, whatever float mode the file is built with
CE_HD bool ce_is_nan(float v) {
  union {
    float f;
    uint32_t u;
  } b;
  b.f = v;
  return (b.u & 0x7fffffffu) > 0x7f800000u;
}

// min(max(conf, 0), 1) of a confidence that is not a NaN (+-inf included)
CE_HD float ce_clamp01(float conf) { return conf < 0.f ? 0.f : conf > 1.f ? 1.f : conf; }

// the bin of a clamped confidence: min(n_bins - 1, (int)(c * n_bins)), the product in fp32
CE_HD int ce_bin(float c, int n_bins) {
  const int b = (int)(c * (float)n_bins);
  return b < n_bins - 1 ? b : n_bins - 1;
}

// the clamped confidence in Q24: c * 2^24 is exact in fp32 up to the bits below 2^-24 that rintf rounds (to even)
CE_HD int64_t ce_q24(float c) { return (int64_t)rintf(c * 16777216.f); }

// The counters one pixel adds to: add(i, n) is called with every flat index i and its increment n.  ranks: the K
// raw labels of the pixel, rank 0 first; g: its ground truth.  A pixel whose ground truth is the ignore label, or
// no class at all (outside 0 .. N-1), enters nothing; one with a NaN confidence counts in `nan` only.
template <class A>
CE_HD void ce_count_pixel(const int (&ranks)[CE_MAX_K], int K, float conf, int g, int N, int ignore_label,
                          int clamp_pred, int n_bins, const A& add) {
  if (g == ignore_label || g < 0 || g >= N) return;
  if (ce_is_nan(conf)) {
    add(ce_off_nan(n_bins, K), (int64_t)1);
    return;
  }
  const float c = ce_clamp01(conf);
  const int b = ce_bin(c, n_bins);
  add(ce_off_count(n_bins) + b, (int64_t)1);
  if (ce_fold(ranks[0], clamp_pred) == g) add(ce_off_correct(n_bins) + b, (int64_t)1);
  const int64_t q = ce_q24(c);
  if (q) add(ce_off_q24(n_bins) + b, q);
  bool hit = false;
  for (int k = 0; k < K; ++k) {
    hit = hit || ce_fold(ranks[k], clamp_pred) == g;
    if (hit) add(ce_off_hit(n_bins) + k, (int64_t)1);
  }
  add(ce_off_valid(n_bins, K), (int64_t)1);
}
