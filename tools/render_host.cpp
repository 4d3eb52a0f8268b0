// Host run of the renderer's logic of csrc/render_logic.h (what render.hip's kernel calls), pass by pass as the
// kernel runs it but sequentially over the whole map: the "row window is uniform" flag of every pixel, the edge test
// down the columns, the colour of every pixel, the cell means.  It reads one case from a file and writes the picture
// to another; tests/test_render_cpu.py writes random cases, runs it and compares with the numpy restatement
// (tests/render_ref.py), which shares nothing with the header.  Every array lives in a vector of exactly its size
// and is read through at(), so a read outside a map is an error.  No GPU; build with host sanitizers if wanted:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I cat-seg_amd/csrc tools/render_host.cpp -o /tmp/rh
//   /tmp/rh case.bin out.bin
// The case file: 18 int32 (H, W, clamp_pred, P, other_rgb, has_image, ih, iw, gray, has_score, has_gt,
// ignore_label, error_rgb, ignore_rgb, alpha_q8, edge_px, edge_rgb, factor), then labels int32 [H][W], palette
// uint8 [P][3], image uint8 [ih][iw][3], score float [H][W], gt int32 [H][W] (the optional ones only when present).
// The result: uint8 [Ho][Wo][3].  Exit 0 on success, 2 on a malformed case.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "render_logic.h"

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> h;
  if (!read_vec(f, h, 18)) return 2;
  const int H = h[0], W = h[1], clamp = h[2], P = h[3], has_image = h[5], ih = h[6], iw = h[7], has_score = h[9],
            has_gt = h[10], e = h[15], factor = h[17];
  if (H < 1 || W < 1 || H > RL_MAX_SIDE || W > RL_MAX_SIDE || P < 1 || P > RL_MAX_PALETTE || e < 0 ||
      e > RL_MAX_EDGE || factor < 1 || factor > RL_MAX_FACTOR)
    return 2;
  const RlStyle style = {P, h[4], h[14], h[11], h[12], h[13], h[16], h[8]};
  const size_t HW = (size_t)H * W;
  std::vector<int32_t> labels, gt;
  std::vector<uint8_t> palette, image;
  std::vector<float> score;
  if (!read_vec(f, labels, HW) || !read_vec(f, palette, (size_t)P * 3) ||
      !read_vec(f, image, has_image ? (size_t)ih * iw * 3 : 0) || !read_vec(f, score, has_score ? HW : 0) ||
      !read_vec(f, gt, has_gt ? HW : 0))
    return 2;
  fclose(f);

  std::vector<int> lab(HW);
  for (size_t p = 0; p < HW; ++p) lab[p] = be_fold(labels[p], clamp);
  std::vector<unsigned char> uni(e ? HW : 0);
  if (e)
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x)
        uni[(size_t)y * W + x] = rl_row_uniform(x, W, e, [&](int q) { return lab.at((size_t)y * W + q); });
  std::vector<int> colour(HW);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const size_t p = (size_t)y * W + x;
      const int l = lab[p];
      const bool edge = e && rl_edge(y, H, e, l, [&](int q) { return uni.at((size_t)q * W + x) != 0; },
                                     [&](int q) { return lab.at((size_t)q * W + x); });
      const int c = rl_label_color(l, style, [&](int k) {
        return (palette.at(3 * (size_t)k) << 16) | (palette.at(3 * (size_t)k + 1) << 8) | palette.at(3 * (size_t)k + 2);
      });
      int ir = 0, ig = 0, ib = 0;
      if (has_image) {
        const size_t s = ((size_t)rl_src(y, H, ih) * iw + rl_src(x, W, iw)) * 3;
        ir = image.at(s), ig = image.at(s + 1), ib = image.at(s + 2);
      }
      colour[p] = rl_pixel_color(l, c, style, has_gt != 0, has_gt ? gt[p] : 0, has_score != 0,
                                 has_score ? score[p] : 0.0f, has_image != 0, ir, ig, ib, edge);
    }
  const int Ho = (H + factor - 1) / factor, Wo = (W + factor - 1) / factor;
  std::vector<uint8_t> out((size_t)Ho * Wo * 3);
  for (int Y = 0; Y < Ho; ++Y)
    for (int X = 0; X < Wo; ++X) {
      int sum[3] = {0, 0, 0}, n = 0;
      for (int y = Y * factor; y < (Y + 1) * factor && y < H; ++y)
        for (int x = X * factor; x < (X + 1) * factor && x < W; ++x, ++n) {
          const int c = colour.at((size_t)y * W + x);
          sum[0] += (c >> 16) & 255, sum[1] += (c >> 8) & 255, sum[2] += c & 255;
        }
      for (int k = 0; k < 3; ++k) out[((size_t)Y * Wo + X) * 3 + k] = (uint8_t)rl_cell_mean(sum[k], n);
    }
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 1, out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("ok %d %d\n", Ho, Wo);
  return 0;
}
