// Host run of the boundary-evaluation logic of csrc/boundary_eval_logic.h (what boundary_eval.hip's kernels call),
// pass by pass as the kernels run it but sequentially: the "starts a run" bit line of every row, be_row_distance per
// pixel, be_column_distance per pixel, be_count_pixel per pixel.  Checked against a brute-force restatement that
// shares nothing with the header: the distance from the definition (growing windows), the counters from the
// contract's four rules.  The bit lines and the row distances live in vectors of exactly their size, so a read past
// a line or a row is a sanitizer error.  No GPU; build with host sanitizers if wanted:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I cat-seg_amd/csrc tools/boundary_eval_host.cpp -o /tmp/beh && /tmp/beh
// Prints one line per failing case and "ok <cases>" at the end; exit 1 on a miss.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "boundary_eval_logic.h"

typedef std::vector<int> Map;
typedef unsigned long long u64;

// ---- brute force ----
static int brute_distance(const Map& m, int H, int W, int clamp, int cap, int y, int x) {
  auto at = [&](int yy, int xx) {
    const int v = m[(size_t)yy * W + xx];
    return (clamp >= 0 && v >= clamp) ? clamp : v;
  };
  const int mine = at(y, x);
  for (int k = 1; k < cap; ++k) {
    for (int yy = y - k; yy <= y + k; ++yy)
      for (int xx = x - k; xx <= x + k; ++xx) {
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return k;
        if (at(yy, xx) != mine) return k;
      }
  }
  return cap;
}

static std::vector<long long> brute_counters(const Map& P, const Map& G, const std::vector<int>& dP,
                                             const std::vector<int>& dG, int N, int ignore, int clamp,
                                             const std::vector<int>& widths) {
  const int n1 = N + 1, per = n1 * n1 + 3 * N;
  std::vector<long long> c(widths.size() * (size_t)per, 0);
  for (size_t p = 0; p < P.size(); ++p) {
    int a = P[p], g = G[p];
    if (clamp >= 0 && a >= clamp) a = clamp;
    if (g == ignore) g = N;
    if (g < 0 || g > N || a < 0 || a > N) continue;
    for (size_t k = 0; k < widths.size(); ++k) {
      long long* band = &c[k * per];
      long long *inter = band + n1 * n1, *gtb = inter + N, *prb = gtb + N;
      if (dG[p] <= widths[k]) band[a * n1 + g]++;
      if (g == N) continue;
      if (dG[p] <= widths[k]) gtb[g]++;
      if (a < N && dP[p] <= widths[k]) prb[a]++;
      if (a == g && dG[p] <= widths[k] && dP[p] <= widths[k]) inter[g]++;
    }
  }
  return c;
}

// ---- the kernels' passes, sequentially ----
static std::vector<int> logic_distance(const Map& m, int H, int W, int clamp, int cap) {
  const int words = (W + RO_WORD - 1) / RO_WORD;
  std::vector<int> h((size_t)H * W), d((size_t)H * W);
  for (int y = 0; y < H; ++y) {
    std::vector<u64> line(words, 0);                // exactly the row's words
    const int* row = &m[(size_t)y * W];
    for (int x = 0; x < W; ++x)
      if (x == 0 || be_fold(row[x], clamp) != be_fold(row[x - 1], clamp)) line[x >> 6] |= 1ull << (x & 63);
    for (int x = 0; x < W; ++x) h[(size_t)y * W + x] = be_row_distance(line.data(), W, x, cap);
  }
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      const int mine = be_fold(m[(size_t)y * W + x], clamp);
      d[(size_t)y * W + x] = be_column_distance(y, H, h[(size_t)y * W + x], [&](int yy) {
        return be_fold(m.at((size_t)yy * W + x), clamp) == mine ? h.at((size_t)yy * W + x) : 0;
      });
    }
  return d;
}

static Map random_map(std::mt19937& rng, int H, int W, int nlab, int blob, double speckle, bool wild) {
  static const int WILD[] = {-1, 255, INT_MIN, INT_MAX, 0, 7};
  Map m((size_t)H * W);
  const int by = (H + blob - 1) / blob, bx = (W + blob - 1) / blob;
  std::vector<int> coarse((size_t)by * bx);
  for (int& v : coarse) v = (int)(rng() % nlab);
  std::uniform_real_distribution<double> u(0.0, 1.0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int v = coarse[(size_t)(y / blob) * bx + x / blob];
      if (u(rng) < speckle) v = (int)(rng() % nlab);
      m[(size_t)y * W + x] = wild ? WILD[v % 6] : v;
    }
  return m;
}

int main() {
  std::mt19937 rng(1234);
  int cases = 0, bad = 0;
  const int shapes[][2] = {{1, 1}, {1, 9}, {9, 1}, {1, 130}, {130, 1}, {7, 7}, {34, 25}, {63, 64}, {64, 65},
                           {70, 100}, {40, 129}, {3, 200}};
  const int caps[] = {1, 2, 5, 7, 30, 40, 64, 65, 300};
  for (const auto& s : shapes)
    for (int cap : caps)
      for (int variant = 0; variant < 4; ++variant) {
        const int H = s[0], W = s[1];
        // 0: blobs + speckle, 1: uniform, 2: large blobs with wild labels, 3: 5 labels folded at 2
        const Map m = variant == 1 ? Map((size_t)H * W, 3)
                                   : random_map(rng, H, W, variant == 3 ? 5 : 3, variant == 2 ? 23 : 6,
                                                variant == 2 ? 0.0 : 0.02, variant == 2);
        const int clamp = variant == 3 ? 2 : -1;
        const std::vector<int> d = logic_distance(m, H, W, clamp, cap);
        ++cases;
        for (int y = 0; y < H && bad < 20; ++y)
          for (int x = 0; x < W; ++x) {
            const int want = brute_distance(m, H, W, clamp, cap, y, x);
            if (d[(size_t)y * W + x] != want) {
              printf("distance %d x %d cap %d variant %d: (%d, %d) got %d want %d\n", H, W, cap, variant, y, x,
                     d[(size_t)y * W + x], want);
              ++bad;
              break;
            }
          }
      }
  // the counters: N = 5, ignore 255, some ground truth out of range, with and without the fold
  for (int variant = 0; variant < 4; ++variant) {
    const int H = 33, W = 41, N = 5, ignore = 255, clamp = (variant & 1) ? 3 : -1;
    Map G = random_map(rng, H, W, N, 7, 0.01, false), P = random_map(rng, H, W, N + 2, 7, 0.05, false);
    for (int y = 4; y < 9; ++y)
      for (int x = 10; x < 20; ++x) G[(size_t)y * W + x] = ignore;
    G[5] = 77;                                      // neither a class nor the ignore label: skipped
    G[6] = -3;
    if (variant & 2) P[17] = -1;
    const std::vector<int> widths = variant < 2 ? std::vector<int>{3, 1, 3} : std::vector<int>{1, 2, 3, 5, 8, 13, 21, 34};
    const int cap = *std::max_element(widths.begin(), widths.end()) + 1;
    const std::vector<int> dP = logic_distance(P, H, W, clamp, cap), dG = logic_distance(G, H, W, -1, cap);
    const std::vector<long long> want = brute_counters(P, G, dP, dG, N, ignore, clamp, widths);
    std::vector<long long> got(want.size(), 0);
    BeWidths w = {};
    for (size_t k = 0; k < widths.size(); ++k) w.w[k] = widths[k];
    for (size_t p = 0; p < P.size(); ++p)
      be_count_pixel(P[p], G[p], dP[p], dG[p], N, ignore, clamp, w, (int)widths.size(),
                     [&](int i) { got.at((size_t)i)++; });
    ++cases;
    if ((long long)want.size() != (long long)widths.size() * be_counters_per_width(N) || got != want) {
      printf("counters variant %d differ\n", variant);
      ++bad;
    }
  }
  if (bad) return 1;
  printf("ok %d\n", cases);
  return 0;
}
