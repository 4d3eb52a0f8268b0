// Host run of the vote logic of csrc/mode_filter_logic.h (what mode_filter.hip's kernels call), pass by pass as the
// kernels run it but sequentially over the whole map: the votes of every pixel, the total of every window or cell,
// then one pass per voting label in ascending order (the next label by a minimum over the map, its masked votes, the
// row sums, the column sums, the offer to every pixel's best), and the decision.  It reads one case from a file and
// writes the result to another; tests/test_mode_filter_cpu.py writes cases, runs it and compares with the numpy
// restatement (tests/mode_ref.py), which shares nothing with the header; tools/micro_mode_filter.py times it as the
// host stand-in.  Every array lives in a vector of exactly its size and is read through at(), so a read outside a
// map is an error.  No GPU; build with host sanitizers if wanted:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I cat-seg_amd/csrc tools/mode_filter_host.cpp -o /tmp/mf
//   /tmp/mf case.bin out.bin
// The case file: 10 int32 (H, W, op, size or factor, rule_half, has_score, has_novote, novote_label, fill,
// iterations), then labels int32 [H][W] and, with has_score, score float [H][W].  op 0 is the filter, whose result
// is int32 [H][W]; op 1 the overview, whose result is labels, votes and total, int32 [Ho][Wo] each.  It prints
// "ok <rows> <cols> <microseconds of the computation>".  Exit 0 on success, 2 on a malformed case.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mode_filter_logic.h"

template <class T>
static bool read_vec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

struct Case {
  int H, W, rule_half, has_score, has_novote, novote_label, fill;
  std::vector<float> score;
};

static std::vector<int> votes_of(const Case& c, const std::vector<int32_t>& lab) {
  std::vector<int> v(lab.size());
  for (size_t p = 0; p < lab.size(); ++p)
    v[p] = mf_votes(lab[p], c.has_score != 0, c.has_score ? c.score.at(p) : 0.0f, c.has_novote != 0, c.novote_label);
  return v;
}

// the smallest key above cur among the pixels that vote, MF_NO_KEY when there is none
static int64_t next_key(const std::vector<int32_t>& lab, const std::vector<int>& vot, int64_t cur) {
  int64_t k = MF_NO_KEY;
  for (size_t p = 0; p < lab.size(); ++p) k = mf_next_key(k, cur, lab[p], vot[p]);
  return k;
}

// the windowed sums of msk: rows, then columns, the windows clipped to the map
static void box_sums(const Case& c, int r, const std::vector<int>& msk, std::vector<int>& rs, std::vector<int>& s) {
  const int H = c.H, W = c.W;
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      rs[(size_t)y * W + x] = mf_span_sum(x - r > 0 ? x - r : 0, x + r < W - 1 ? x + r : W - 1,
                                          [&](int q) { return msk.at((size_t)y * W + q); });
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x)
      s[(size_t)y * W + x] = mf_span_sum(y - r > 0 ? y - r : 0, y + r < H - 1 ? y + r : H - 1,
                                         [&](int q) { return rs.at((size_t)q * W + x); });
}

static std::vector<int32_t> filter_once(const Case& c, int size, const std::vector<int32_t>& lab) {
  const size_t HW = lab.size();
  const std::vector<int> vot = votes_of(c, lab);
  std::vector<int> msk(vot), rs(HW), s(HW), total(HW), own_sum(HW, 0);
  std::vector<MfBest> best(HW);
  for (size_t p = 0; p < HW; ++p) best[p] = MfBest{0, lab[p]};
  box_sums(c, size / 2, msk, rs, total);
  int64_t cand = next_key(lab, vot, MF_FIRST);
  for (size_t pass = 0; pass < HW && cand != MF_NO_KEY; ++pass, cand = next_key(lab, vot, cand)) {
    const int l = mf_label(cand);
    for (size_t p = 0; p < HW; ++p) msk[p] = lab[p] == l ? vot[p] : 0;
    box_sums(c, size / 2, msk, rs, s);
    for (size_t p = 0; p < HW; ++p) {
      best[p] = mf_offer(best[p], s[p], l);
      if (lab[p] == l) own_sum[p] = s[p];
    }
  }
  std::vector<int32_t> out(HW);
  for (size_t p = 0; p < HW; ++p)
    out[p] = mf_decide(lab[p], own_sum[p], best[p], total[p], c.rule_half != 0, c.has_novote != 0, c.novote_label,
                       c.fill != 0);
  return out;
}

static void overview(const Case& c, int f, const std::vector<int32_t>& lab, int Ho, int Wo, std::vector<int32_t>& out) {
  const std::vector<int> vot = votes_of(c, lab);
  const size_t n = (size_t)Ho * Wo;
  out.assign(3 * n, 0);
  for (int Y = 0; Y < Ho; ++Y)
    for (int X = 0; X < Wo; ++X) {
      const int ya = Y * f, yb = ya + f < c.H ? ya + f : c.H, xa = X * f, xb = xa + f < c.W ? xa + f : c.W;
      int total = 0;
      int64_t least = MF_NO_KEY;
      for (int y = ya; y < yb; ++y)
        for (int x = xa; x < xb; ++x) {
          total += vot.at((size_t)y * c.W + x);
          least = mf_key(lab.at((size_t)y * c.W + x)) < least ? mf_key(lab[(size_t)y * c.W + x]) : least;
        }
      MfBest best = {0, c.has_novote ? c.novote_label : mf_label(least)};
      int64_t cand = MF_FIRST;
      for (int pass = 0; pass <= f * f; ++pass) {
        int64_t k = MF_NO_KEY;
        for (int y = ya; y < yb; ++y)
          for (int x = xa; x < xb; ++x) k = mf_next_key(k, cand, lab[(size_t)y * c.W + x], vot[(size_t)y * c.W + x]);
        if (k == MF_NO_KEY) break;
        cand = k;
        const int l = mf_label(cand);
        int s = 0;
        for (int y = ya; y < yb; ++y)
          s += mf_span_sum(xa, xb - 1, [&](int x) {
            return lab[(size_t)y * c.W + x] == l ? vot[(size_t)y * c.W + x] : 0;
          });
        best = mf_offer(best, s, l);
      }
      const size_t o = (size_t)Y * Wo + X;
      out[o] = best.label, out[n + o] = best.sum, out[2 * n + o] = total;
    }
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> h;
  if (!read_vec(f, h, 10)) return 2;
  Case c = {h[0], h[1], h[4], h[5], h[6], h[7], h[8], {}};
  const int op = h[2], k = h[3], iterations = h[9];
  if (c.H < 1 || c.W < 1 || c.H > MF_MAX_SIDE || c.W > MF_MAX_SIDE || (op != 0 && op != 1)) return 2;
  if (op == 0 && (k < MF_MIN_SIZE || k > MF_MAX_SIZE || !(k & 1) || iterations < 1 || iterations > 8)) return 2;
  if (op == 1 && (k < MF_MIN_FACTOR || k > MF_MAX_FACTOR)) return 2;
  const size_t HW = (size_t)c.H * c.W;
  std::vector<int32_t> lab;
  if (!read_vec(f, lab, HW) || !read_vec(f, c.score, c.has_score ? HW : 0)) return 2;
  fclose(f);

  const auto t0 = std::chrono::steady_clock::now();
  std::vector<int32_t> out;
  int rows = c.H, cols = c.W;
  if (op == 0) {
    out = lab;
    for (int i = 0; i < iterations; ++i) out = filter_once(c, k, out);
  } else {
    rows = (c.H + k - 1) / k, cols = (c.W + k - 1) / k;
    overview(c, k, lab, rows, cols, out);
  }
  const long long us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
  FILE* g = fopen(argv[2], "wb");
  if (!g || fwrite(out.data(), 4, out.size(), g) != out.size()) return 2;
  fclose(g);
  printf("ok %d %d %lld\n", rows, cols, us);
  return 0;
}
