// The per-pixel and per-column logic of the boundary evaluation kernels (boundary_eval.hip), as host + device
// functions, so that tools/boundary_eval_host.cpp runs the very same code sequentially on the host against the
// brute-force definition before a kernel ever runs.  The contract is DESIGN.md section 4 ("Boundary-aware
// evaluation").
//
// D(p) = the Chebyshev distance from pixel p to the nearest pixel of another (folded) label, the outside of the map
// counting as another label; the kernels return min(D, cap).  It is computed separably:
//   h(x, y)  = the same distance inside row y alone = min(x - s + 1, e - x), [s, e) the run of equal labels round x;
//   D(x, y)  = min over y' in [-1, H] of max(|y - y'|, g(y')), g(y') = h(x, y') where row y' is inside the map and
//              L(x, y') == L(x, y), else 0.
// A row's runs are a bit line: bit x of the line (bit x % 64 of word x / 64) is set where pixel x starts a run
// (x == 0 or its folded label differs from its left neighbour's).
#pragma once
#include <stdint.h>

#include "region_outlines_logic.h"

constexpr int BE_MAX_SIDE = 16384;                 // H, W and cap
constexpr int BE_MAX_WIDTHS = 8;                   // K of the counters
constexpr int BE_ROW_WORDS = BE_MAX_SIDE / RO_WORD;   // words of the longest bit line

struct BeWidths {
  int w[BE_MAX_WIDTHS];
};

// labels >= clamp fold to clamp (clamp < 0: no fold)
RO_HD int be_fold(int label, int clamp) { return (clamp >= 0 && label >= clamp) ? clamp : label; }

// h of pixel x of a row of W pixels from its bit line, capped: the walk over the words stops once the distance
// reaches cap, so a pixel reads at most cap / 64 + 2 words each way.  Bit 0 of the line is always set.
RO_HD int be_row_distance(const unsigned long long* line, int W, int x, int cap) {
  int w = x >> 6;
  unsigned long long m = line[w] & (ro_below(x & 63) | (1ull << (x & 63)));
  int left = cap;                                   // x - s + 1
  for (;;) {
    if (m) {
      left = x - (w * RO_WORD + ro_top(m)) + 1;
      break;
    }
    if (x - (w * RO_WORD) + 1 >= cap) break;        // every start further left is at least cap away
    m = line[--w];
  }
  if (left > cap) left = cap;
  const int words = (W + RO_WORD - 1) / RO_WORD;
  w = x >> 6;
  m = line[w] & ro_above(x & 63);
  int right = cap;                                  // e - x
  for (;;) {
    if (m) {
      right = w * RO_WORD + ro_ctz(m) - x;
      break;
    }
    if (++w >= words) {
      right = W - x;
      break;
    }
    if (w * RO_WORD - x >= cap) break;
    m = line[w];
  }
  if (right > cap) right = cap;
  return left < right ? left : right;
}

// min(D, cap) of pixel (x, y) from the row distances: h0 = min(h(x, y), cap) and g(y') for a row inside the map =
// min(h(x, y'), cap) where the labels agree, else 0.  |dy| grows until it reaches the best value so far: a pixel
// reads at most 2 (D - 1) other rows, whatever cap is.
template <class G>
RO_HD int be_column_distance(int y, int H, int h0, const G& g) {
  int best = h0;
  for (int dy = 1; dy < best; ++dy) {
    const int up = (y - dy >= 0) ? g(y - dy) : 0;
    const int dn = (y + dy < H) ? g(y + dy) : 0;
    const int v = up < dn ? up : dn;
    const int c = v > dy ? v : dy;
    if (c < best) best = c;
  }
  return best;
}

// Counter layout of one width: band_conf (N+1)^2 indexed [pred][gt], then inter, gt_band, pred_band of N each.
RO_HD int64_t be_counters_per_width(int64_t N) { return (N + 1) * (N + 1) + 3 * N; }

// The counters one pixel adds to: add(i) is called with every flat index i that gains 1.  p, g0: the raw prediction
// and ground truth; dp, dg: their distances (dp on the folded prediction).  A pixel the confusion kernel counts as
// invalid adds nothing.
template <class A>
RO_HD void be_count_pixel(int p, int g0, int dp, int dg, int N, int ignore_label, int clamp_pred,
                          const BeWidths& widths, int K, const A& add) {
  const int a = be_fold(p, clamp_pred);
  const int g = (g0 == ignore_label) ? N : g0;
  if (g < 0 || g > N || a < 0 || a > N) return;
  const int per = (N + 1) * (N + 1) + 3 * N, n1 = N + 1;
  for (int k = 0; k < K; ++k) {
    const int base = k * per;
    const bool in_g = dg <= widths.w[k], in_p = dp <= widths.w[k];
    if (in_g) add(base + a * n1 + g);
    if (g < N) {
      if (in_g) add(base + n1 * n1 + N + g);
      if (a < N && in_p) add(base + n1 * n1 + 2 * N + a);
      if (a == g && in_g && in_p) add(base + n1 * n1 + g);
    }
  }
}
