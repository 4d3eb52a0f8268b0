// The per-pixel logic of the label-map renderer (render.hip), as host + device functions, so that
// tools/render_host.cpp runs the very same code sequentially on the host before a kernel ever runs.  The contract
// is include/catseg_hip_render.h and DESIGN.md section 4 ("Rendering").  Integer arithmetic only; a colour is
// packed 0xRRGGBB.
//
// The edge test is separable without a minimum and a maximum: the (2e + 1)^2 window of (x, y), clipped to the map,
// holds another label exactly when some row y' of it is not uniform over [x - e, x + e] (rl_row_uniform, one flag
// per pixel of the row) or its centre label L(x, y') differs from L(x, y) (rl_edge).
#pragma once
#include <stdint.h>

#include "boundary_eval_logic.h"

constexpr int RL_MAX_SIDE = BE_MAX_SIDE;           // H, W, ih, iw
constexpr int RL_MAX_PALETTE = 8192;
constexpr int RL_MAX_EDGE = 8;
constexpr int RL_MAX_FACTOR = 64;
constexpr int RL_TILE_W = 64;                      // full-resolution pixels of a tile along x, at most
constexpr int RL_TILE_H = 16;                      // and along y, unless one cell is taller

// cells of a tile along an axis whose full-resolution extent is at most `extent`: at least one
RO_HD int rl_tile_cells(int extent, int factor) { return factor >= extent ? 1 : extent / factor; }

// s8 of a score from its bits, so that no floating-point compare (and no compiler's NaN assumption) decides it:
// 256 for score >= 1 (+inf included), (int)(score * 256) for 0 < score < 1, 0 for everything else (-0, negatives,
// NaN of either sign).  score * 256 is exact.
RO_HD int rl_s8(float score) {
  uint32_t u;
  __builtin_memcpy(&u, &score, 4);
  if (u >> 31) return 0;
  if (u > 0x7f800000u) return 0;
  if (u >= 0x3f800000u) return 256;
  return (int)(score * 256.0f);
}

// nearest source index by pixel centre of destination x of n onto m source pixels; the identity for n == m
RO_HD int rl_src(int x, int n, int m) {
  const int s = (int)(((int64_t)(2 * x + 1) * m) / (2 * (int64_t)n));
  return s < m - 1 ? s : m - 1;
}

// PIL's convert("L")
RO_HD int rl_gray(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

RO_HD int rl_blend(int i, int c, int a) { return (i * (256 - a) + c * a + 128) >> 8; }

// steps 1 .. 3 of the contract.  l: the folded label; pal(l): the packed palette colour of 0 <= l < P
struct RlStyle {
  int P, other_rgb, alpha_q8, ignore_label, error_rgb, ignore_rgb, edge_rgb, gray;
};

template <class Pal>
RO_HD int rl_label_color(int l, const RlStyle& s, const Pal& pal) {
  return (l >= 0 && l < s.P) ? pal(l) : s.other_rgb;
}

// steps 2 .. 5 for one pixel.  c: rl_label_color of l; has_gt / g, has_score / score, has_image / (ir, ig, ib) the
// source pixel's channels, edge: the result of rl_edge (false with edge_px == 0)
RO_HD int rl_pixel_color(int l, int c, const RlStyle& s, bool has_gt, int g, bool has_score, float score,
                         bool has_image, int ir, int ig, int ib, bool edge) {
  if (edge) return s.edge_rgb;
  int a = s.alpha_q8;
  if (has_gt) {
    if (g == s.ignore_label)
      c = s.ignore_rgb;
    else if (g != l)
      c = s.error_rgb;
  }
  if (has_score) a = (a * rl_s8(score)) >> 8;
  if (has_image) {
    if (s.gray) ir = ig = ib = rl_gray(ir, ig, ib);
    const int r = rl_blend(ir, (c >> 16) & 255, a), gg = rl_blend(ig, (c >> 8) & 255, a), b = rl_blend(ib, c & 255, a);
    c = (r << 16) | (gg << 8) | b;
  }
  return c;
}

// row(x'): the folded label of pixel x' of one row, asked for x' in [max(0, x - e), min(W - 1, x + e)] only
template <class Row>
RO_HD bool rl_row_uniform(int x, int W, int e, const Row& row) {
  const int lo = x - e > 0 ? x - e : 0, hi = x + e < W - 1 ? x + e : W - 1;
  const int v = row(x);
  bool same = true;
  for (int xx = lo; xx <= hi; ++xx) same = same && row(xx) == v;
  return same;
}

// uniform(y'), label(y'): rl_row_uniform and the folded label at column x of row y', asked for
// y' in [max(0, y - e), min(H - 1, y + e)] only
template <class U, class Lb>
RO_HD bool rl_edge(int y, int H, int e, int l, const U& uniform, const Lb& label) {
  const int lo = y - e > 0 ? y - e : 0, hi = y + e < H - 1 ? y + e : H - 1;
  bool edge = false;
  for (int yy = lo; yy <= hi; ++yy) edge = edge || !uniform(yy) || label(yy) != l;
  return edge;
}

// the rounded mean of a cell of n pixels
RO_HD int rl_cell_mean(int sum, int n) { return (sum + n / 2) / n; }
