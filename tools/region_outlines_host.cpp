// Host run of the region-outline logic of csrc/region_outlines_logic.h (what region_outlines.hip's kernels call
// per vertex and per corner), phase by phase as the kernels run it, with the items of every phase in a shuffled
// order, against a brute-force tracer that enumerates the directed boundary edges and follows the successor
// rule one lattice unit at a time.  No GPU; build with host sanitizers if wanted:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I cat-seg_amd/csrc tools/region_outlines_host.cpp -o /tmp/roh && /tmp/roh
// Prints one line per (shape, pattern, connectivity) on failure and "ok <cases>" at the end; exit 1 on a miss.
//
// Second use, the host baseline of tools/micro_region_outlines.py:
//   region_outlines_host --trace FILE H W CONNECTIVITY REPS
// reads H * W little-endian int32 from FILE, runs the brute-force tracer REPS times and prints one JSON line
// {"K", "NR", "ms": [..]}.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "region_outlines_logic.h"

typedef std::vector<int> Map;

struct Rings {
  std::vector<int> offset, value, vx, vy;
  std::vector<long long> area2;
  bool operator==(const Rings& o) const {
    return offset == o.offset && value == o.value && vx == o.vx && vy == o.vy && area2 == o.area2;
  }
};

// ---- the brute-force tracer: written from the rules of DESIGN.md, shares nothing with the logic header ----
struct Brute {
  const Map& m;
  int H, W;
  bool conn8;
  bool has(int y, int x) const { return y >= 0 && y < H && x >= 0 && x < W; }
  int at(int y, int x) const { return m[(size_t)y * W + x]; }
  // right / left pixel of the unit edge from vertex (x, y) heading d, as (y, x); may lie outside
  static void sides(int x, int y, int d, int& ry, int& rx, int& ly, int& lx) {
    switch (d) {
      case 0: ry = y, rx = x, ly = y - 1, lx = x; break;
      case 1: ry = y, rx = x - 1, ly = y, lx = x; break;
      case 2: ry = y - 1, rx = x - 1, ly = y, lx = x - 1; break;
      default: ry = y - 1, rx = x, ly = y - 1, lx = x - 1; break;
    }
  }
  bool boundary(int x, int y, int d, int& r) const {
    int ry, rx, ly, lx;
    sides(x, y, d, ry, rx, ly, lx);
    if (!has(ry, rx)) return false;
    r = at(ry, rx);
    return !(has(ly, lx) && at(ly, lx) == r);
  }
  int turn(int x, int y, int d, int r) const {
    int ay, ax, by, bx;
    sides(x, y, d, ay, ax, by, bx);
    const bool a = has(ay, ax) && at(ay, ax) == r, b = has(by, bx) && at(by, bx) == r;
    if (a && b) return (d + 3) & 3;
    if (a) return d;
    if (b) return conn8 ? (d + 3) & 3 : (d + 1) & 3;
    return (d + 1) & 3;
  }
  Rings trace() const {
    static const int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};
    const int VW = W + 1;
    // an edge is named by its END vertex and direction, as a corner's key is
    std::vector<unsigned char> seen((size_t)(H + 1) * VW * 4, 0);
    Rings out;
    out.offset.push_back(0);
    // keys ascending: the first unseen edge that is a corner is its ring's smallest corner, so rings come out in
    // order; an unseen edge that goes straight is skipped here and reached from its ring's first corner
    std::vector<int> cx, cy;
    for (int y = 0; y <= H; ++y)
      for (int x = 0; x <= W; ++x)
        for (int d = 0; d < 4; ++d) {
          const size_t k = ((size_t)y * VW + x) * 4 + d;
          if (seen[k]) continue;
          const int sx = x - DX[d], sy = y - DY[d];
          if (sx < 0 || sy < 0 || sx > W || sy > H) continue;
          int r;
          if (!boundary(sx, sy, d, r)) continue;
          if (turn(x, y, d, r) == d) continue;
          cx.clear();
          cy.clear();
          int px = x, py = y, pd = d;
          do {
            seen[((size_t)py * VW + px) * 4 + pd] = 1;
            const int o = turn(px, py, pd, r);
            if (o != pd) cx.push_back(px), cy.push_back(py);
            px += DX[o], py += DY[o], pd = o;
          } while (!(px == x && py == y && pd == d));
          long long a2 = 0;
          const size_t n = cx.size();
          for (size_t i = 0; i < n; ++i) {
            const size_t j = (i + 1) % n;
            a2 += (long long)cx[i] * cy[j] - (long long)cx[j] * cy[i];
          }
          out.value.push_back(r);
          out.area2.push_back(a2);
          out.vx.insert(out.vx.end(), cx.begin(), cx.end());
          out.vy.insert(out.vy.end(), cy.begin(), cy.end());
          out.offset.push_back((int)out.vx.size());
        }
    return out;
  }
};

// ---- the kernels' phases over the logic header ----
static std::vector<int> shuffled(int n, std::mt19937& rng) {
  std::vector<int> o(n);
  for (int i = 0; i < n; ++i) o[i] = i;
  std::shuffle(o.begin(), o.end(), rng);
  return o;
}

struct HostBits {
  const std::vector<unsigned long long>*mask4, *colbits;
  int row_words, col_words, W;
  unsigned long long row(int d, int y, int xw) const { return mask4->at(((size_t)y * row_words + xw) * 4 + d); }
  unsigned long long col(int d, int x, int yw) const {
    return colbits->at(((size_t)(d >> 1) * (W + 1) + x) * col_words + yw);
  }
};

static std::vector<int> exscan(const std::vector<int>& v, int& total) {
  std::vector<int> o(v.size());
  total = 0;
  for (size_t i = 0; i < v.size(); ++i) o[i] = total, total += v[i];
  return o;
}

static Rings logic_phases(const Map& m, int H, int W, bool conn8, std::mt19937& rng, bool& ok) {
  const int VW = W + 1, VH = H + 1;
  const int row_words = (VW + RO_WORD - 1) / RO_WORD, col_words = (VH + RO_WORD - 1) / RO_WORD;
  const int nwords = VH * row_words;
  auto G = [&](int y, int x) { return m.at((size_t)y * W + x); };
  auto code_of = [&](int x, int y) -> unsigned {
    if (x > W) return 0u;
    int q[4];
    const unsigned have = ro_quad(G, x, y, H, W, q);
    return ro_corners(q, have, conn8);
  };
  // count
  std::vector<int> cnt(nwords, -1);
  std::vector<unsigned long long> mask4((size_t)nwords * 4, ~0ull), colbits((size_t)2 * VW * col_words, 0ull);
  for (int gw : shuffled(nwords, rng)) {
    const int y = gw / row_words, xw = gw % row_words;
    unsigned long long mm[4] = {0, 0, 0, 0};
    for (int lane = 0; lane < RO_WORD; ++lane) {
      const int x = xw * RO_WORD + lane;
      const unsigned code = code_of(x, y);
      for (int d = 0; d < 4; ++d)
        if (ro_is_corner(code, d)) mm[d] |= 1ull << lane;
      if (ro_is_corner(code, 1)) colbits.at((size_t)x * col_words + (y >> 6)) |= 1ull << (y & 63);
      if (ro_is_corner(code, 3)) colbits.at(((size_t)VW + x) * col_words + (y >> 6)) |= 1ull << (y & 63);
    }
    cnt[gw] = ro_popc(mm[0]) + ro_popc(mm[1]) + ro_popc(mm[2]) + ro_popc(mm[3]);
    for (int d = 0; d < 4; ++d) mask4[(size_t)gw * 4 + d] = mm[d];
  }
  int K;
  const std::vector<int> off = exscan(cnt, K);
  // link
  std::vector<int> key(K, -1), succ(K, -1);
  std::vector<RoJump> st[2] = {std::vector<RoJump>(K), std::vector<RoJump>(K)};
  const HostBits bits{&mask4, &colbits, row_words, col_words, W};
  for (int v : shuffled(VH * row_words * RO_WORD, rng)) {
    const int gw = v / RO_WORD, lane = v % RO_WORD;
    const int y = gw / row_words, xw = gw % row_words, x = xw * RO_WORD + lane;
    const unsigned code = code_of(x, y);
    for (int d = 0; d < 4; ++d) {
      if (!ro_is_corner(code, d)) continue;
      const int i = ro_corner_index(off[gw], &mask4[(size_t)gw * 4], lane, d);
      const int o = ro_out(code, d);
      const int c = ro_successor(bits, x, y, o, H, W);
      const int x1 = (o & 1) ? x : c, y1 = (o & 1) ? c : y;
      if (c < 0 || x1 > W || y1 > H) {
        ok = false;
        return Rings();
      }
      const int w1 = y1 * row_words + (x1 >> 6);
      const int j = ro_corner_index(off[w1], &mask4[(size_t)w1 * 4], x1 & 63, o);
      key.at(i) = (y * VW + x) * 4 + d;
      succ.at(i) = j;
      st[0].at(i) = RoJump{j, i, 0};
    }
  }
  // jump
  const int rounds = ro_rounds(K);
  for (int r = 0; r < rounds; ++r) {
    const std::vector<RoJump>& in = st[r & 1];
    std::vector<RoJump>& out = st[(r + 1) & 1];
    for (int i : shuffled(K, rng)) out[i] = ro_jump(in[i], in.at(in[i].nxt), r);
  }
  const std::vector<RoJump>& fin = st[rounds & 1];
  // final + scans
  std::vector<int> start(K), rank(K), a(K), b(K);
  for (int i : shuffled(K, rng)) {
    const int s = fin[i].mn;
    const int len = ro_ring_length(fin.at(succ.at(s)).off);
    start[i] = s;
    rank[i] = ro_rank(len, fin[i].off);
    a[i] = s == i;
    b[i] = s == i ? len : 0;
  }
  int NR, total;
  const std::vector<int> ringno = exscan(a, NR), ringoff = exscan(b, total);
  if (total != K) ok = false;
  // write
  Rings out;
  out.offset.assign(NR + 1, -1);
  out.value.assign(NR, -1);
  out.area2.assign(NR, 0);
  out.vx.assign(K, -1);
  out.vy.assign(K, -1);
  out.offset[NR] = total;
  for (int i : shuffled(K, rng)) {
    const int s = start[i], ring = ringno.at(s), first = ringoff.at(s);
    const int k0 = key[i] >> 2, d0 = key[i] & 3, k1 = key.at(succ[i]) >> 2;
    const int y0 = k0 / VW, x0 = k0 % VW, y1 = k1 / VW, x1 = k1 % VW;
    out.area2.at(ring) += ro_area_term(x0, y0, x1, y1);
    out.vx.at(first + rank[i]) = x0;
    out.vy.at(first + rank[i]) = y0;
    if (s == i) {
      out.offset.at(ring) = first;
      const int py = y0 - (d0 == 1 || d0 == 2 ? 1 : 0), px = x0 - (d0 == 0 || d0 == 1 ? 1 : 0);
      out.value.at(ring) = G(py, px);
    }
  }
  return out;
}

// ---- maps ----
static Map pattern(const std::string& name, int H, int W, std::mt19937& rng) {
  Map m((size_t)H * W, 0);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) {
      int v = 0;
      if (name == "const") v = 7;
      else if (name == "checker") v = (x + y) & 1;
      else if (name == "speckle") v = (int)(rng() % 3);
      else if (name == "blobs") v = ((x / 5) * 7 + (y / 3) * 3) % 4 + ((rng() % 50) == 0);
      else if (name == "serpentine") v = (y % 2 == 0) ? 1 : ((y / 2) % 2 == 0 ? (x == W - 1) : (x == 0));
      else if (name == "frames") {
        const int ring = std::min(std::min(x, W - 1 - x), std::min(y, H - 1 - y));
        v = ring & 1;
      } else if (name == "ids") v = y * W + x;
      m[(size_t)y * W + x] = v;
    }
  return m;
}

static int trace_mode(int argc, char** argv) {
  if (argc != 7) {
    std::fprintf(stderr, "usage: %s --trace FILE H W CONNECTIVITY REPS\n", argv[0]);
    return 2;
  }
  const int H = std::atoi(argv[3]), W = std::atoi(argv[4]), conn = std::atoi(argv[5]), reps = std::atoi(argv[6]);
  if (H <= 0 || W <= 0 || (conn != 4 && conn != 8) || reps <= 0) return 2;
  Map m((size_t)H * W);
  FILE* f = std::fopen(argv[2], "rb");
  if (!f || std::fread(m.data(), 4, m.size(), f) != m.size()) {
    std::fprintf(stderr, "cannot read %zu ints from %s\n", m.size(), argv[2]);
    return 2;
  }
  std::fclose(f);
  std::string ms;
  size_t K = 0, NR = 0;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    const Rings out = Brute{m, H, W, conn == 8}.trace();
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    K = out.vx.size(), NR = out.value.size();
    char buf[32];
    std::snprintf(buf, sizeof buf, "%s%.3f", r ? ", " : "", dt);
    ms += buf;
  }
  std::printf("{\"K\": %zu, \"NR\": %zu, \"ms\": [%s]}\n", K, NR, ms.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::strcmp(argv[1], "--trace") == 0) return trace_mode(argc, argv);
  std::mt19937 rng(12345);
  const int shapes[][2] = {{1, 1}, {1, 2}, {2, 2}, {1, 200}, {200, 1}, {3, 63}, {3, 64}, {63, 3}, {64, 3}, {5, 5},
                           {33, 65}, {70, 130}, {67, 129}, {130, 67}, {96, 96}};
  const char* names[] = {"const", "checker", "speckle", "blobs", "serpentine", "frames", "ids"};
  int cases = 0, bad = 0;
  for (const auto& s : shapes)
    for (const char* name : names)
      for (int conn = 4; conn <= 8; conn += 4) {
        const int H = s[0], W = s[1];
        const Map m = pattern(name, H, W, rng);
        const Rings want = Brute{m, H, W, conn == 8}.trace();
        bool ok = true;
        const Rings got = logic_phases(m, H, W, conn == 8, rng, ok);
        ++cases;
        if (!ok || !(got == want)) {
          ++bad;
          std::printf("MISS %d x %d %s conn %d: rings %zu vs %zu, corners %zu vs %zu\n", H, W, name, conn,
                      got.value.size(), want.value.size(), got.vx.size(), want.vx.size());
        }
        // the corner bound of the contract
        if ((long long)want.vx.size() > 4ll * (H + 1) * (W + 1)) ++bad;
      }
  if (bad) return 1;
  std::printf("ok %d\n", cases);
  return 0;
}
