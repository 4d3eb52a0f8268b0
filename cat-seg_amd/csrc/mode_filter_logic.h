// The vote logic of the majority filter and the mode overviews (mode_filter.hip), as host + device functions, so
// that tools/mode_filter_host.cpp runs the very same code sequentially on the host before a kernel ever runs.  The
// contract is include/catseg_hip_mode.h and DESIGN.md section 4 ("Mode filter and overviews").  Integer arithmetic
// only, after the one conversion of a score to its weight.
//
// A winner is found without a dictionary: the labels that vote are visited in ascending order (mf_next_key: the
// smallest key above the current one), each with the sum of its votes, and mf_offer keeps a candidate only on a
// strictly greater sum, so that among equal sums the smallest label stays.  The filter then lets the pixel's own
// label replace the kept one where its sum equals the best (mf_decide).
#pragma once
#include <stdint.h>

#include "region_outlines_logic.h"

constexpr int MF_MAX_SIDE = 16384;                 // H, W
constexpr int MF_MIN_SIZE = 3;
constexpr int MF_MAX_SIZE = 15;                    // the filter's window, odd
constexpr int MF_MIN_FACTOR = 2;
constexpr int MF_MAX_FACTOR = 32;                  // the overview's cell
constexpr int MF_ONE = 65536;                      // the weight of score 1 (the Q16 of label_regions)
constexpr int MF_TILE_W = 64;                      // output pixels of a workgroup of the filter along x
constexpr int MF_TILE_H = 16;                      // and along y
// every vote sum fits int32: a window holds at most 15 * 15 * 65536 = 14 745 600 (twice that in the "half" test),
// a cell at most 32 * 32 * 65536 = 67 108 864
static_assert((int64_t)2 * MF_MAX_SIZE * MF_MAX_SIZE * MF_ONE < INT32_MAX, "window sums fit int32");
static_assert((int64_t)2 * MF_MAX_FACTOR * MF_MAX_FACTOR * MF_ONE < INT32_MAX, "cell sums fit int32");

// clamp(rint(score * 65536), 0, 65536) and 0 for a NaN, from the score's bits, so that no floating-point compare (and
// no compiler's NaN assumption) decides it: 0 for a set sign (-0, negatives, -inf, NaN), 0 for NaN, 65536 for
// score >= 1 (+inf included).  score * 65536 is exact and below 65536; the rounding is to nearest even.
RO_HD int mf_weight(float score) {
  uint32_t u;
  __builtin_memcpy(&u, &score, 4);
  if (u >> 31) return 0;
  if (u > 0x7f800000u) return 0;
  if (u >= 0x3f800000u) return MF_ONE;
  return (int)__builtin_rintf(score * 65536.0f);
}

// the votes pixel q casts for its own label: its weight (1 without a score map), none for the novote label
RO_HD int mf_votes(int label, bool has_score, float score, bool has_novote, int novote_label) {
  if (has_novote && label == novote_label) return 0;
  return has_score ? mf_weight(score) : 1;
}

// labels in their order as non-negative keys; MF_NO_KEY is above every label and MF_FIRST below
constexpr int64_t MF_NO_KEY = (int64_t)1 << 32;
constexpr int64_t MF_FIRST = -1;
RO_HD int64_t mf_key(int label) { return (int64_t)label + ((int64_t)1 << 31); }
RO_HD int mf_label(int64_t key) { return (int)(key - ((int64_t)1 << 31)); }

// the running minimum of the keys above `cur` of the pixels that vote
RO_HD int64_t mf_next_key(int64_t running, int64_t cur, int label, int votes) {
  const int64_t k = mf_key(label);
  return (votes > 0 && k > cur && k < running) ? k : running;
}

// the best (sum, label) so far; candidates arrive in ascending label order
struct MfBest {
  int sum, label;
};
RO_HD MfBest mf_offer(MfBest b, int sum, int label) { return sum > b.sum ? MfBest{sum, label} : b; }

// The filter's result for one pixel.  own: its value; own_sum: the vote sum of that value in its window (0 for
// the novote label); best: the winner after every candidate was offered, starting from {0, any}; total: the
// window's vote sum.
RO_HD int mf_decide(int own, int own_sum, MfBest best, int total, bool rule_half, bool has_novote, int novote_label,
                    bool fill) {
  if (has_novote && own == novote_label && !fill) return own;
  if (total <= 0) return own;                                   // no vote in the window
  const int winner = own_sum == best.sum ? own : best.label;    // best.sum > 0, so an equal own label votes
  if (rule_half && !(2 * best.sum > total)) return own;
  return winner;
}

// the sum of get(q) over q in [lo, hi]
template <class Get>
RO_HD int mf_span_sum(int lo, int hi, const Get& get) {
  int s = 0;
  for (int q = lo; q <= hi; ++q) s += get(q);
  return s;
}

// lanes that share one overview cell: the smallest power of two >= factor^2, at most a wave
RO_HD int mo_group(int factor) {
  int g = 1;
  while (g < factor * factor && g < 64) g *= 2;
  return g;
}
