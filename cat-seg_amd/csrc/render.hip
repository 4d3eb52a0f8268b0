// The label-map renderer (include/catseg_hip_render.h; DESIGN.md section 4, "Rendering"): an int32 label map as an
// RGB picture, blended over an image, faded by a score, marked against a ground truth, with the label edges drawn,
// reduced by an integer factor f.  One launch, integer only, the logic in render_logic.h.
//
//   tile     a workgroup owns TCX x TCY output cells, TCX = max(1, 64 / f), TCY = max(1, 16 / f): a full-resolution
//            footprint of at most 64 x 16 pixels (64 x f once one cell is taller than 16), cut where the map ends;
//   labels   the folded labels of the footprint plus an edge_px halo, clipped to the map, into LDS once;
//   edges    rows: one "the window [x - e, x + e] of this row is uniform" flag per pixel of the footprint's rows
//            (halo rows included); columns: a pixel is an edge when a row of its window is not uniform or that
//            row's centre label differs, the same answer as minimum != maximum over the window, with one byte where
//            those take two ints;
//   colour   once per pixel: palette, ground truth, score, image (nearest by pixel centre), blend; with f == 1
//            straight into the staging rows, else packed into LDS;
//   cells    f > 1: a thread per (pixel row, cell) sums its f pixels, then a thread per cell sums its f rows and
//            rounds the mean into the staging rows;
//   store    a staging row is the tile's 3 TCX bytes of one output row: the dwords that lie whole inside it go out
//            as dwords, the at most 3 + 3 bytes before and after them as bytes (ld_out and the base need no alignment,
//            and a neighbouring tile owns the bytes next to it).
// Per pixel 4 B of labels (the halo again per tile), 3 B of image, 4 B of score, 4 B of ground truth and 3 / f^2 B of
// output move; the palette (at most 24 KB) stays in cache.  No workgroup waits for another; every map index is 64-bit.
#include "common.h"
#include "capi.h"
#include "render_logic.h"

namespace {

struct RlArgs {
  const int32_t* labels;
  const uint8_t* palette;
  const uint8_t* image;
  const float* score;
  const int32_t* gt;
  uint8_t* out;
  int64_t ld, ld_score, ld_gt, ld_out, is_row, is_col, is_ch;
  int H, W, ih, iw, clamp_pred, edge_px, factor, tcx, tcy;
  RlStyle style;
};

// bytes of LDS of one workgroup; the kernel lays its arrays out in the same order
struct RlLds {
  int lab, uni, col, rs, stage, total;            // byte offsets
};

__host__ __device__ inline RlLds rl_lds(int f, int e, int TCX, int TCY) {
  const int FW = TCX * f, FH = TCY * f, LW = FW + 2 * e, LH = FH + 2 * e;
  RlLds l;
  l.lab = 0;
  l.uni = l.lab + LH * LW * 4;
  l.col = l.uni + (e ? (LH * FW + 3) / 4 * 4 : 0);
  l.rs = l.col + (f > 1 ? FH * FW * 4 : 0);
  l.stage = l.rs + (f > 1 ? FH * TCX * 12 : 0);
  l.total = l.stage + (TCY * TCX * 3 + 3) / 4 * 4;
  return l;
}

__global__ __launch_bounds__(256) void render_labels_kernel(RlArgs a) {
  extern __shared__ int rl_shared[];
  const int f = a.factor, e = a.edge_px, TCX = a.tcx, TCY = a.tcy, H = a.H, W = a.W;
  const int FW = TCX * f, FH = TCY * f, LW = FW + 2 * e, SP = 3 * TCX;
  const RlLds off = rl_lds(f, e, TCX, TCY);
  unsigned char* base = (unsigned char*)rl_shared;
  int* lab = (int*)(base + off.lab);               // [FH + 2e][LW], pixel (x, y) at (y - y0 + e, x - x0 + e)
  unsigned char* uni = base + off.uni;             // [FH + 2e][FW]
  int* col = (int*)(base + off.col);               // [FH][FW] packed colours
  int* rs = (int*)(base + off.rs);                 // [FH][TCX][3] sums of a pixel row of a cell
  unsigned char* stage = base + off.stage;         // [TCY][3 TCX]
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * FW, y0 = blockIdx.y * FH;
  const int fw = min(FW, W - x0), fh = min(FH, H - y0);          // the tile inside the map
  const int lx0 = max(x0 - e, 0), lx1 = min(x0 + fw + e, W), ly0 = max(y0 - e, 0), ly1 = min(y0 + fh + e, H);
  const int lw = lx1 - lx0, lh = ly1 - ly0;

  for (int i = tid; i < lw * lh; i += 256) {
    const int yy = i / lw, x = lx0 + (i - yy * lw), y = ly0 + yy;
    lab[(y - y0 + e) * LW + (x - x0 + e)] = be_fold(a.labels[(int64_t)y * a.ld + x], a.clamp_pred);
  }
  __syncthreads();
  if (e) {
    for (int i = tid; i < lh * fw; i += 256) {
      const int yy = i / fw, xx = i - yy * fw, r = ly0 + yy - y0 + e;
      const int* row = lab + r * LW + e;             // row[x' - x0]
      uni[r * FW + xx] = rl_row_uniform(x0 + xx, W, e, [&](int q) { return row[q - x0]; });
    }
    __syncthreads();
  }
  for (int i = tid; i < fh * fw; i += 256) {
    const int yy = i / fw, xx = i - yy * fw, x = x0 + xx, y = y0 + yy;
    const int l = lab[(yy + e) * LW + xx + e];
    const bool edge = e && rl_edge(y, H, e, l, [&](int q) { return uni[(q - y0 + e) * FW + xx] != 0; },
                                   [&](int q) { return lab[(q - y0 + e) * LW + xx + e]; });
    int c = rl_label_color(l, a.style, [&](int k) {
      const uint8_t* p = a.palette + 3 * k;
      return ((int)p[0] << 16) | ((int)p[1] << 8) | (int)p[2];
    });
    const int g = a.gt ? a.gt[(int64_t)y * a.ld_gt + x] : 0;
    const float s = a.score ? a.score[(int64_t)y * a.ld_score + x] : 0.0f;
    int ir = 0, ig = 0, ib = 0;
    if (a.image) {
      const uint8_t* px = a.image + (int64_t)rl_src(y, H, a.ih) * a.is_row + (int64_t)rl_src(x, W, a.iw) * a.is_col;
      ir = px[0];
      ig = px[a.is_ch];
      ib = px[2 * a.is_ch];
    }
    c = rl_pixel_color(l, c, a.style, a.gt != nullptr, g, a.score != nullptr, s, a.image != nullptr, ir, ig, ib, edge);
    if (f == 1) {
      unsigned char* d = stage + yy * SP + 3 * xx;
      d[0] = (unsigned char)(c >> 16);
      d[1] = (unsigned char)(c >> 8);
      d[2] = (unsigned char)c;
    } else {
      col[yy * FW + xx] = c;
    }
  }
  __syncthreads();
  const int tcx = (fw + f - 1) / f, tcy = (fh + f - 1) / f;      // the tile's cells inside the map
  if (f > 1) {
    for (int i = tid; i < fh * tcx; i += 256) {
      const int yy = i / tcx, cx = i - yy * tcx, xa = cx * f, xb = min(xa + f, fw);
      int r = 0, g = 0, b = 0;
      for (int xx = xa; xx < xb; ++xx) {
        const int c = col[yy * FW + xx];
        r += (c >> 16) & 255;
        g += (c >> 8) & 255;
        b += c & 255;
      }
      int* d = rs + (yy * TCX + cx) * 3;
      d[0] = r;
      d[1] = g;
      d[2] = b;
    }
    __syncthreads();
    for (int i = tid; i < tcy * tcx; i += 256) {
      const int cy = i / tcx, cx = i - cy * tcx, ya = cy * f, yb = min(ya + f, fh);
      int r = 0, g = 0, b = 0;
      for (int yy = ya; yy < yb; ++yy) {
        const int* p = rs + (yy * TCX + cx) * 3;
        r += p[0];
        g += p[1];
        b += p[2];
      }
      const int n = (min(cx * f + f, fw) - cx * f) * (yb - ya);
      unsigned char* d = stage + cy * SP + 3 * cx;
      d[0] = (unsigned char)rl_cell_mean(r, n);
      d[1] = (unsigned char)rl_cell_mean(g, n);
      d[2] = (unsigned char)rl_cell_mean(b, n);
    }
    __syncthreads();
  }
  // 64 slots per staging row: at most 48 dwords, 3 bytes before and 3 after them
  const int nb = 3 * tcx;
  for (int i = tid; i < tcy * 64; i += 256) {
    const int r = i >> 6, s = i & 63;
    uint8_t* g = a.out + ((int64_t)blockIdx.y * TCY + r) * a.ld_out + (int64_t)blockIdx.x * SP;
    const unsigned char* src = stage + r * SP;
    const int head = min((int)((0 - (uintptr_t)g) & 3), nb), ndw = (nb - head) >> 2, tail = nb - head - 4 * ndw;
    if (s < ndw) {
      const int o = head + 4 * s;
      *(uint32_t*)(g + o) = (uint32_t)src[o] | ((uint32_t)src[o + 1] << 8) | ((uint32_t)src[o + 2] << 16) |
                            ((uint32_t)src[o + 3] << 24);
    } else if (s < ndw + head) {
      const int o = s - ndw;
      g[o] = src[o];
    } else if (s < ndw + head + tail) {
      const int o = head + 4 * ndw + (s - ndw - head);
      g[o] = src[o];
    }
  }
}

bool rl_side(int64_t v) { return v >= 1 && v <= RL_MAX_SIDE; }
bool rl_rgb(int v) { return v >= 0 && v <= 0xffffff; }

}  // namespace

extern "C" int catseg_render_labels(const int32_t* labels, int64_t H, int64_t W, int64_t ld, int clamp_pred,
                                    const uint8_t* palette, int P, int other_rgb, const uint8_t* image, int64_t ih,
                                    int64_t iw, int64_t is_row, int64_t is_col, int64_t is_ch, int gray,
                                    const float* score, int64_t ld_score, const int32_t* gt, int64_t ld_gt,
                                    int ignore_label, int error_rgb, int ignore_rgb, int alpha_q8, int edge_px,
                                    int edge_rgb, int factor, uint8_t* out, int64_t ld_out, void* stream) {
  CATSEG_CHECK(labels && palette && out, "render_labels: null pointer");
  CATSEG_CHECK(rl_side(H) && rl_side(W), "render_labels: H and W must lie in 1 .. 16384");
  CATSEG_CHECK(P >= 1 && P <= RL_MAX_PALETTE, "render_labels: P (palette entries) must lie in 1 .. 8192");
  CATSEG_CHECK(alpha_q8 >= 0 && alpha_q8 <= 256, "render_labels: alpha_q8 must lie in 0 .. 256");
  CATSEG_CHECK(edge_px >= 0 && edge_px <= RL_MAX_EDGE, "render_labels: edge_px must lie in 0 .. 8");
  CATSEG_CHECK(factor >= 1 && factor <= RL_MAX_FACTOR, "render_labels: factor must lie in 1 .. 64");
  CATSEG_CHECK(rl_rgb(other_rgb) && rl_rgb(edge_rgb) && (!gt || (rl_rgb(error_rgb) && rl_rgb(ignore_rgb))),
               "render_labels: a colour is outside 0x000000 .. 0xFFFFFF");
  const int64_t Wo = (W + factor - 1) / factor;
  CATSEG_CHECK(ld >= W && (!score || ld_score >= W) && (!gt || ld_gt >= W), "render_labels: a row stride is smaller than W");
  CATSEG_CHECK(ld_out >= 3 * Wo, "render_labels: the row stride of out is smaller than 3 Wo");
  CATSEG_CHECK(!image || (rl_side(ih) && rl_side(iw)), "render_labels: the image's ih and iw must lie in 1 .. 16384");
  CATSEG_CHECK(!image || (is_row >= 0 && is_col >= 0 && is_ch >= 0), "render_labels: negative image stride");
  CATSEG_CHECK(((uintptr_t)labels % 4) == 0 && ((uintptr_t)score % 4) == 0 && ((uintptr_t)gt % 4) == 0,
               "render_labels: misaligned pointer");
  RlArgs a = {};
  a.labels = labels, a.palette = palette, a.image = image, a.score = score, a.gt = gt, a.out = out;
  a.ld = ld, a.ld_score = ld_score, a.ld_gt = ld_gt, a.ld_out = ld_out;
  a.is_row = is_row, a.is_col = is_col, a.is_ch = is_ch;
  a.H = (int)H, a.W = (int)W, a.ih = (int)ih, a.iw = (int)iw, a.clamp_pred = clamp_pred, a.edge_px = edge_px;
  a.factor = factor, a.tcx = rl_tile_cells(RL_TILE_W, factor), a.tcy = rl_tile_cells(RL_TILE_H, factor);
  a.style = RlStyle{P, other_rgb, alpha_q8, ignore_label, error_rgb, ignore_rgb, edge_rgb, gray != 0};
  const int FW = a.tcx * factor, FH = a.tcy * factor;
  const RlLds lds = rl_lds(factor, edge_px, a.tcx, a.tcy);
  hipLaunchKernelGGL(render_labels_kernel, dim3((unsigned)((W + FW - 1) / FW), (unsigned)((H + FH - 1) / FH)),
                     dim3(256), (size_t)lds.total, (hipStream_t)stream, a);
  return catseg_launch_status("render_labels");
}
