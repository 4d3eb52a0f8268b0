// Host run of the connected-region logic of csrc/label_regions_logic.h (what label_regions.hip's kernels
// call per pixel), phase by phase as the kernels run it, with the pixels of every phase in a shuffled order,
// against a brute-force flood fill and a brute-force sieve.  No GPU; build with host sanitizers if wanted:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I cat-seg_amd/csrc tools/label_regions_host.cpp -o /tmp/lrh && /tmp/lrh
// Prints one line per (shape, pattern, connectivity) on failure and "ok <cases>" at the end; exit 1 on a miss.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "label_regions_logic.h"

struct HostMem {
  int* p;
  int load(int i) { return p[i]; }
  int fetch_min(int i, int v) {
    const int old = p[i];
    if (v < old) p[i] = v;
    return old;
  }
};
struct HostKeys {
  unsigned long long* k;
  void fetch_max(int i, unsigned long long v) {
    if (v > k[i]) k[i] = v;
  }
};

typedef std::vector<int> Map;

static std::vector<int> shuffled(int n, std::mt19937& rng) {
  std::vector<int> o(n);
  for (int i = 0; i < n; ++i) o[i] = i;
  std::shuffle(o.begin(), o.end(), rng);
  return o;
}

// the three labelling phases, as the kernels run them; returns parent with every pixel at its root
static std::vector<int> label_phases(const Map& lab, int H, int W, bool conn8, std::mt19937& rng) {
  std::vector<int> parent(H * W, -1);
  const int T = CC_TILE;
  for (int y0 = 0; y0 < H; y0 += T)
    for (int x0 = 0; x0 < W; x0 += T) {
      const int th = std::min(T, H - y0), tw = std::min(T, W - x0);
      std::vector<int> tl(T * T, 0x55555555), tp(T * T);
      for (int ly = 0; ly < th; ++ly)
        for (int lx = 0; lx < tw; ++lx) tl[ly * T + lx] = lab[(y0 + ly) * W + x0 + lx];
      for (int ly = 0; ly < T; ++ly) {               // the kernel's ballot: bit lx = a run starts at column lx
        unsigned long long starts = 0;
        for (int lx = 0; lx < T; ++lx)
          if (lx == 0 || lx >= tw || tl[ly * T + lx] != tl[ly * T + lx - 1]) starts |= 1ull << lx;
        for (int lx = 0; lx < T; ++lx) tp[ly * T + lx] = ly * T + cc_run_start(starts, lx);
      }
      HostMem m{tp.data()};
      auto L = [&](int i) { return tl.at(i); };
      for (int o : shuffled(T * T, rng)) {
        const int ly = o / T, lx = o % T;
        if (ly < th && lx < tw) cc_tile_pixel(m, L, ly, lx, tw, conn8);
      }
      for (int o : shuffled(T * T, rng)) {
        const int ly = o / T, lx = o % T;
        if (ly < th && lx < tw) cc_tile_settle(m, L, ly, lx);
      }
      for (int ly = 0; ly < th; ++ly)
        for (int lx = 0; lx < tw; ++lx) {
          const int r = cc_find(m, ly * T + lx);
          parent.at((y0 + ly) * W + x0 + lx) = (y0 + r / T) * W + x0 + r % T;
        }
    }
  HostMem m{parent.data()};
  auto G = [&](int y, int x) { return lab.at(y * W + x); };
  const int nbx = (W - 1) / T, nby = (H - 1) / T, nv = nbx * H, nh = nby * W;
  for (int t : shuffled(nv + nh, rng)) {
    if (t < nv) cc_border_vertical(m, G, t % H, (t / H + 1) * T, H, W, conn8);
    else cc_border_horizontal(m, G, ((t - nv) / W + 1) * T, (t - nv) % W, H, W, conn8);
  }
  for (int p : shuffled(H * W, rng)) parent[p] = cc_find(m, p);
  return parent;
}

static std::vector<int> flood(const Map& lab, int H, int W, bool conn8) {
  std::vector<int> root(H * W, -1), stack;
  for (int s = 0; s < H * W; ++s) {
    if (root[s] >= 0) continue;
    root[s] = s;
    stack.assign(1, s);
    while (!stack.empty()) {
      const int p = stack.back(), y = p / W, x = p % W;
      stack.pop_back();
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if ((!dy && !dx) || (!conn8 && dy && dx)) continue;
          const int yy = y + dy, xx = x + dx;
          if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
          const int q = yy * W + xx;
          if (root[q] < 0 && lab[q] == lab[p]) {
            root[q] = s;
            stack.push_back(q);
          }
        }
    }
  }
  return root;
}

// the sieve as the kernels run it (areas at the roots, keys by forward neighbour pairs) against a direct
// restatement (every ordered pair of touching regions, the best large neighbour by (area, -root))
static bool sieve_ok(const Map& lab, const std::vector<int>& root, int H, int W, bool conn8, int min_area) {
  const int n = H * W;
  std::vector<int> area(n, 0);
  for (int p = 0; p < n; ++p) area[root[p]]++;
  std::vector<unsigned long long> keys(n, 0);
  HostKeys K{keys.data()};
  const int dy[4] = {0, 1, 1, 1}, dx[4] = {1, 0, -1, 1};
  std::map<int, std::pair<int, int>> best;         // small root -> (area, -root) of its best large neighbour
  for (int p = 0; p < n; ++p) {
    const int y = p / W, x = p % W;
    for (int k = 0; k < (conn8 ? 4 : 2); ++k) {
      const int yy = y + dy[k], xx = x + dx[k];
      if (yy >= H || xx < 0 || xx >= W) continue;
      const int rp = root[p], rq = root[yy * W + xx];
      if (rp == rq) continue;
      cc_sieve_pair(K, rp, area[rp], rq, area[rq], min_area);
      for (int s = 0; s < 2; ++s) {
        const int a = s ? rq : rp, b = s ? rp : rq;
        if (area[a] < min_area && area[b] >= min_area) {
          const std::pair<int, int> c(area[b], -b);
          if (!best.count(a) || c > best[a]) best[a] = c;
        }
      }
    }
  }
  for (int p = 0; p < n; ++p) {
    const int r = root[p];
    const int src = cc_sieve_source(r, area[r], keys[r], min_area);
    const int want = best.count(r) ? -best[r].second : r;
    if (src != want) return false;
  }
  return true;
}

static Map pattern(const std::string& name, int H, int W, std::mt19937& rng) {
  Map m(H * W, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int& v = m[y * W + x];
      if (name == "uniform") v = 7;
      else if (name == "checker") v = (x + y) & 1;
      else if (name == "vstripe1") v = x & 1;
      else if (name == "vstripe3") v = (x / 3) & 1;
      else if (name == "hstripe1") v = y & 1;
      else if (name == "hstripe3") v = (y / 3) & 1;
      else if (name == "rings") v = (std::max(std::abs(y - H / 2), std::abs(x - W / 2)) / 2) % 3;
      else if (name == "serpentine") v = (y % 2 == 0) ? 1 : ((y / 2) % 2 == 0 ? x == W - 1 : x == 0);
      else if (name == "noise3") v = (int)(rng() % 3);
      else if (name == "blobs") v = ((y / 23) * 5 + (x / 31) * 3) % 4 + (rng() % 50 == 0 ? 9 : 0);
      else if (name == "diagonals") v = ((x + y) % 4 == 0) ? 1 : ((x - y + 4096) % 4 == 2 ? 2 : 0);
    }
  return m;
}

int main() {
  const int shapes[][2] = {{1, 1}, {1, 130}, {130, 1}, {64, 64}, {65, 67}, {127, 129}, {200, 333}, {5, 5}, {128, 128}};
  const char* names[] = {"uniform", "checker", "vstripe1", "vstripe3", "hstripe1", "hstripe3",
                         "rings", "serpentine", "noise3", "blobs", "diagonals"};
  std::mt19937 rng(12345);
  int cases = 0, bad = 0;
  for (auto& s : shapes)
    for (const char* nm : names)
      for (int conn8 = 0; conn8 < 2; ++conn8) {
        const int H = s[0], W = s[1];
        const Map lab = pattern(nm, H, W, rng);
        const std::vector<int> want = flood(lab, H, W, conn8);
        for (int rep = 0; rep < 2; ++rep) {
          const std::vector<int> got = label_phases(lab, H, W, conn8, rng);
          ++cases;
          if (got != want) {
            ++bad;
            printf("MISS labelling %dx%d %s conn%d\n", H, W, nm, conn8 ? 8 : 4);
            break;
          }
        }
        // region numbers from the flags: the scan restated, cc_region_id against a running count
        std::vector<int> seg((H * W + 63) / 64, 0);
        std::vector<unsigned long long> mask(seg.size(), 0);
        for (int p = 0; p < H * W; ++p)
          if (want[p] == p) {
            seg[p >> 6]++;
            mask[p >> 6] |= 1ull << (p & 63);
          }
        int run = 0, id = 0;
        for (size_t i = 0; i < seg.size(); ++i) {
          const int c = seg[i];
          seg[i] = run;
          run += c;
        }
        for (int p = 0; p < H * W; ++p)
          if (want[p] == p && cc_region_id(seg[p >> 6], mask[p >> 6], p) != id++) {
            ++bad;
            printf("MISS region id %dx%d %s conn%d\n", H, W, nm, conn8 ? 8 : 4);
            break;
          }
        for (int min_area : {1, 2, 8, 40, H * W + 1}) {
          ++cases;
          if (!sieve_ok(lab, want, H, W, conn8, min_area)) {
            ++bad;
            printf("MISS sieve %dx%d %s conn%d min_area %d\n", H, W, nm, conn8 ? 8 : 4, min_area);
          }
        }
      }
  if (cc_score_q16(0.5f / 65536.0f) != 0 || cc_score_q16(1.5f / 65536.0f) != 2 || cc_score_q16(1.0f) != 65536 ||
      cc_score_q16(2.5f / 65536.0f) != 2) {
    ++bad;
    printf("MISS score_q16 rounding\n");
  }
  printf("%s %d cases, %d missed\n", bad ? "FAILED" : "ok", cases, bad);
  return bad ? 1 : 0;
}
