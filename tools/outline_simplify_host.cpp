// Host run of the outline-simplification logic of csrc/outline_simplify_logic.h (what outline_simplify.hip's
// kernels call), phase by phase as the kernels run it but sequentially: junction bitmaps, node counts from
// popcounts, node write, anchor bitmap, arcs, os_douglas_peucker with its explicit stack, compaction.  Checked
// against a brute-force restatement that shares nothing with the header: junctions from the lattice edges, nodes by
// walking every ring edge one lattice unit at a time, and a recursive Douglas-Peucker.  No GPU; build with host
// sanitizers if wanted:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I cat-seg_amd/csrc tools/outline_simplify_host.cpp -o /tmp/osh && /tmp/osh
// Prints one line per failing case and "ok <cases>" at the end; exit 1 on a miss.
//
// Second use, the host baseline of tools/micro_outline_simplify.py:
//   outline_simplify_host --simplify FILE H W NR K TOLERANCE REPS
// reads from FILE little-endian int32: H * W ids, NR + 1 ring offsets, 2 K vertex coordinates (x, y); runs the
// sequential pipeline REPS times and prints one JSON line {"N", "K2", "arcs", "hist": [..], "ms": [..]}, hist[b] =
// the number of arcs of at least 2 edges whose length has b as its highest set bit.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "outline_simplify_logic.h"

typedef std::vector<int> Map;
typedef unsigned long long u64;

struct Rings {
  std::vector<int> offset, vx, vy;
};
struct Simplified {
  std::vector<int> offset, vx, vy;
  std::vector<long long> area2;
  long long N = 0, arcs = 0;
  std::vector<long long> hist;
  bool operator==(const Simplified& o) const {
    return offset == o.offset && vx == o.vx && vy == o.vy && area2 == o.area2 && N == o.N;
  }
};

static const int DX[4] = {1, 0, -1, 0}, DY[4] = {0, 1, 0, -1};

// ---- brute force: the rings of a map (connectivity 4 or 8), written from the rules of DESIGN.md ----
struct Brute {
  const Map& m;
  int H, W;
  bool has(int y, int x) const { return y >= 0 && y < H && x >= 0 && x < W; }
  int at(int y, int x) const { return m[(size_t)y * W + x]; }
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
  int turn(int x, int y, int d, int r, bool conn8) const {
    int ay, ax, by, bx;
    sides(x, y, d, ay, ax, by, bx);
    const bool a = has(ay, ax) && at(ay, ax) == r, b = has(by, bx) && at(by, bx) == r;
    if (a && b) return (d + 3) & 3;
    if (a) return d;
    if (b) return conn8 ? (d + 3) & 3 : (d + 1) & 3;
    return (d + 1) & 3;
  }
  Rings trace(bool conn8) const {
    const int VW = W + 1;
    std::vector<unsigned char> seen((size_t)(H + 1) * VW * 4, 0);
    Rings out;
    out.offset.push_back(0);
    for (int y = 0; y <= H; ++y)
      for (int x = 0; x <= W; ++x)
        for (int d = 0; d < 4; ++d) {
          if (seen[((size_t)y * VW + x) * 4 + d]) continue;
          const int sx = x - DX[d], sy = y - DY[d];
          int r;
          if (sx < 0 || sy < 0 || sx > W || sy > H || !boundary(sx, sy, d, r) || turn(x, y, d, r, conn8) == d) continue;
          int px = x, py = y, pd = d;
          do {
            seen[((size_t)py * VW + px) * 4 + pd] = 1;
            const int o = turn(px, py, pd, r, conn8);
            if (o != pd) out.vx.push_back(px), out.vy.push_back(py);
            px += DX[o], py += DY[o], pd = o;
          } while (!(px == x && py == y && pd == d));
          out.offset.push_back((int)out.vx.size());
        }
    return out;
  }
  // a junction by the definition: the lattice edges at the vertex whose two pixels differ
  bool junction(int x, int y) const {
    auto differ = [&](int y0, int x0, int y1, int x1) { return !(has(y0, x0) && has(y1, x1) && at(y0, x0) == at(y1, x1)); };
    int deg = 0;
    if (x < W) deg += differ(y - 1, x, y, x);
    if (x > 0) deg += differ(y - 1, x - 1, y, x - 1);
    if (y > 0) deg += differ(y - 1, x - 1, y - 1, x);
    if (y < H) deg += differ(y, x - 1, y, x);
    return deg >= 3 || ((x == 0 || x == W) && (y == 0 || y == H));
  }
};

struct Pt {
  long long x, y;
  bool anchor;
};

static void brute_dp(const std::vector<Pt>& P, int i, int j, long long tol, int W, std::vector<char>& keep) {
  if (j - i < 2) return;
  long long m = -1, mv = 0;
  int mk = -1;
  const bool closed = P[i].x == P[j].x && P[i].y == P[j].y;
  const long long dx = P[j].x - P[i].x, dy = P[j].y - P[i].y, L = closed ? 1 : dx * dx + dy * dy;
  for (int k = i + 1; k < j; ++k) {
    const long long rx = P[k].x - P[i].x, ry = P[k].y - P[i].y;
    const long long c = dx * ry - dy * rx, s = closed ? rx * rx + ry * ry : c * c, v = P[k].y * (W + 1) + P[k].x;
    if (s > m || (s == m && v < mv)) m = s, mv = v, mk = k;
  }
  if (16 * m <= tol * L) return;
  keep[mk] = 1;
  brute_dp(P, i, mk, tol, W, keep);
  brute_dp(P, mk, j, tol, W, keep);
}

static Simplified brute_simplify(const Map& m, int H, int W, const Rings& rings, long long tol) {
  const Brute b{m, H, W};
  Simplified out;
  out.offset.push_back(0);
  for (size_t r = 0; r + 1 < rings.offset.size(); ++r) {
    const int lo = rings.offset[r], n = rings.offset[r + 1] - lo;
    std::vector<Pt> nodes;
    for (int i = 0; i < n; ++i) {
      const int x0 = rings.vx[lo + i], y0 = rings.vy[lo + i], x1 = rings.vx[lo + (i + 1) % n], y1 = rings.vy[lo + (i + 1) % n];
      nodes.push_back(Pt{x0, y0, b.junction(x0, y0)});
      const int dx = (x1 > x0) - (x1 < x0), dy = (y1 > y0) - (y1 < y0);
      for (int x = x0 + dx, y = y0 + dy; x != x1 || y != y1; x += dx, y += dy)
        if (b.junction(x, y)) nodes.push_back(Pt{x, y, true});
    }
    const int nn = (int)nodes.size();
    out.N += nn;
    std::vector<int> anchors;
    for (int i = 0; i < nn; ++i)
      if (nodes[i].anchor) anchors.push_back(i);
    std::vector<char> keep(nn, 0);
    if (anchors.empty()) anchors.push_back(0);
    for (size_t a = 0; a < anchors.size(); ++a) {
      const int s = anchors[a], e = anchors[(a + 1) % anchors.size()];
      const int len = anchors.size() == 1 ? nn : (e - s + nn) % nn;
      std::vector<Pt> P;
      for (int k = 0; k <= len; ++k) P.push_back(nodes[(s + k) % nn]);
      std::vector<char> kk(len + 1, 0);
      kk[0] = kk[len] = 1;
      brute_dp(P, 0, len, tol, W, kk);
      for (int k = 0; k <= len; ++k)
        if (kk[k]) keep[(s + k) % nn] = 1;
    }
    std::vector<Pt> kept;
    for (int i = 0; i < nn; ++i)
      if (keep[i]) kept.push_back(nodes[i]);
    long long a2 = 0;
    for (size_t i = 0; i < kept.size(); ++i) {
      const Pt &p = kept[i], &q = kept[(i + 1) % kept.size()];
      a2 += p.x * q.y - q.x * p.y;
      out.vx.push_back((int)p.x), out.vy.push_back((int)p.y);
    }
    out.area2.push_back(a2);
    out.offset.push_back((int)out.vx.size());
  }
  return out;
}

// ---- the kernels' phases over the logic header, sequentially ----
struct HostMap {
  const Map* m;
  int W;
  int operator()(int y, int x) const { return (*m)[(size_t)y * W + x]; }
};

struct HostArc {                                   // the policy of os_douglas_peucker
  const std::vector<int>& nodes;
  std::vector<int>& keep_flags;
  std::vector<int>& stack;                         // 2 ints per node slot
  int s, ringlen, first, W;
  int slot(int k) const { return s + (first + k) % ringlen; }
  int node(int k) const { return nodes[slot(k)]; }
  void keep(int k) { keep_flags[slot(k)] = 1; }
  void push(int sp, int i, int j) { stack[2 * slot(sp)] = i, stack[2 * slot(sp) + 1] = j; }
  void pop(int sp, int& i, int& j) { i = stack[2 * slot(sp)], j = stack[2 * slot(sp) + 1]; }
  OsBest best(int i, int j, int pi, int pj) {
    OsBest b = os_none();
    for (int k = j - 1; k > i; --k) {              // any order gives the same pick
      const int pk = node(k);
      b = os_pick(b, OsBest{os_score(pi, pj, pk), os_vkey(pk, W), k});
    }
    return b;
  }
};

static Simplified logic_simplify(const Map& m, int H, int W, const Rings& rings, long long tol) {
  const int NR = (int)rings.offset.size() - 1, K = (int)rings.vx.size();
  const int row_words = (W + RO_WORD) / RO_WORD, col_words = (H + RO_WORD) / RO_WORD;
  std::vector<u64> rowbits((size_t)(H + 1) * row_words, 0), colbits((size_t)(W + 1) * col_words, 0);
  const HostMap g{&m, W};
  for (int y = 0; y <= H; ++y)
    for (int x = 0; x <= W; ++x) {
      int q[4];
      const unsigned have = ro_quad(g, x, y, H, W, q);
      if (!os_junction(q, have, x, y, H, W)) continue;
      rowbits[(size_t)y * row_words + (x >> 6)] |= 1ull << (x & 63);
      colbits[(size_t)x * col_words + (y >> 6)] |= 1ull << (y & 63);
    }
  // per corner: its edge's bit line and ends, the count, the scan
  struct Edge {
    const u64* line;
    int a, b, ring, lo;
    bool horizontal;
  };
  auto edge = [&](int i) {
    Edge e;
    e.ring = os_ring_of(rings.offset.data(), NR, i);
    e.lo = rings.offset[e.ring];
    const int hi = rings.offset[e.ring + 1], j = i + 1 < hi ? i + 1 : e.lo;
    e.horizontal = rings.vy[i] == rings.vy[j];
    e.line = e.horizontal ? &rowbits[(size_t)rings.vy[i] * row_words] : &colbits[(size_t)rings.vx[i] * col_words];
    e.a = e.horizontal ? rings.vx[i] : rings.vy[i];
    e.b = e.horizontal ? rings.vx[j] : rings.vy[j];
    return e;
  };
  std::vector<int> off(K + 1, 0);
  for (int i = 0; i < K; ++i) {
    const Edge e = edge(i);
    off[i + 1] = off[i] + 1 + os_count_open(e.line, e.a, e.b);
  }
  const int N = off[K];
  std::vector<int> node(N), ring(N), keep(N, 0), ringstart(NR + 1, 0), stack(2 * (size_t)N, 0);
  ringstart[NR] = N;
  for (int i = 0; i < K; ++i) {
    const Edge e = edge(i);
    int p = off[i];
    if (i == e.lo) ringstart[e.ring] = p;
    node[p] = os_pack(rings.vx[i], rings.vy[i]);
    ring[p] = e.ring;
    keep[p] = os_bit(&rowbits[(size_t)rings.vy[i] * row_words], rings.vx[i]);
    for (int cur = os_next_open(e.line, e.a, e.b); cur >= 0; cur = os_next_open(e.line, cur, e.b)) {
      ++p;
      node[p] = e.horizontal ? os_pack(cur, rings.vy[i]) : os_pack(rings.vx[i], cur);
      ring[p] = e.ring;
      keep[p] = 1;
    }
    if (p + 1 != off[i + 1]) {
      printf("count and walk disagree at corner %d\n", i);
      exit(1);
    }
  }
  std::vector<u64> abits((size_t)(N + RO_WORD) / RO_WORD + 1, 0);
  for (int p = 0; p < N; ++p)
    if (keep[p]) abits[p >> 6] |= 1ull << (p & 63);
  Simplified out;
  out.N = N;
  out.hist.assign(32, 0);
  std::vector<int> arcs, arclen(N, 0);
  for (int p = 0; p < N; ++p) {
    const int s = ringstart[ring[p]], e = ringstart[ring[p] + 1];
    int len = 0;
    if (os_bit(abits.data(), p)) {
      int q = os_next_open(abits.data(), p, e);
      if (q < 0) q = os_first_in(abits.data(), s, p + 1);
      len = q > p ? q - p : q + (e - s) - p;
    } else if (p == s && os_first_in(abits.data(), s, e) < 0) {
      len = e - s;
      keep[p] = 1;
    }
    arclen[p] = len;
    if (len >= 2) arcs.push_back(p), ++out.hist[ro_top((u64)len)];
  }
  out.arcs = (long long)arcs.size();
  for (int p : arcs) {
    const int s = ringstart[ring[p]], e = ringstart[ring[p] + 1];
    HostArc arc{node, keep, stack, s, e - s, p - s, W};
    os_douglas_peucker(arc, arclen[p], tol);
  }
  out.offset.assign(NR + 1, 0);
  out.area2.assign(NR, 0);
  std::vector<int> kxy;
  for (int r = 0, p = 0; r < NR; ++r) {
    out.offset[r] = (int)kxy.size();
    for (; p < ringstart[r + 1]; ++p)
      if (keep[p]) kxy.push_back(node[p]);
  }
  out.offset[NR] = (int)kxy.size();
  for (int r = 0; r < NR; ++r)
    for (int q = out.offset[r]; q < out.offset[r + 1]; ++q) {
      const int p0 = kxy[q], p1 = kxy[q + 1 < out.offset[r + 1] ? q + 1 : out.offset[r]];
      out.area2[r] += ro_area_term(os_x(p0), os_y(p0), os_x(p1), os_y(p1));
      out.vx.push_back(os_x(p0)), out.vy.push_back(os_y(p0));
    }
  return out;
}

// ---- maps ----
static Map random_map(std::mt19937& rng, int H, int W, int nlab, double keep) {
  Map m((size_t)H * W);
  std::uniform_int_distribution<int> lab(0, nlab - 1);
  std::uniform_real_distribution<double> u(0, 1);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) m[(size_t)y * W + x] = (x > 0 && u(rng) < keep) ? m[(size_t)y * W + x - 1] : lab(rng);
  return m;
}
static Map sawtooth(int H, int W, int amp) {       // a coastline: one long arc from the left frame to the right
  Map m((size_t)H * W);
  for (int y = 0; y < H; ++y)
    for (int x = 0; x < W; ++x) m[(size_t)y * W + x] = y < H / 2 + ((x / 2) % amp) - amp / 2 + (x % 7 == 0) ? 1 : 2;
  return m;
}

static int self_test() {
  std::mt19937 rng(12345);
  const int shapes[][2] = {{1, 1}, {1, 9}, {7, 1}, {2, 2}, {3, 63}, {3, 64}, {3, 65}, {3, 129}, {63, 3}, {64, 3},
                           {65, 3}, {129, 3}, {13, 13}, {24, 31}, {37, 59}, {70, 130}};
  const double tols[] = {0.0, 0.5, 1.0, 1.5, 3.0, 1000.0};
  int cases = 0, bad = 0;
  auto check = [&](const Map& m, int H, int W, const char* what) {
    const Brute b{m, H, W};
    for (int conn8 = 0; conn8 < 2; ++conn8) {
      const Rings rings = b.trace(conn8 != 0);
      for (double t : tols) {
        const long long tol = os_tol2_q4(t);
        ++cases;
        if (!(logic_simplify(m, H, W, rings, tol) == brute_simplify(m, H, W, rings, tol))) {
          printf("MISS %s %d x %d connectivity %d tolerance %g\n", what, H, W, conn8 ? 8 : 4, t);
          ++bad;
        }
      }
    }
  };
  for (auto& s : shapes) {
    check(random_map(rng, s[0], s[1], 3, 0.6), s[0], s[1], "smear");
    check(random_map(rng, s[0], s[1], 2, 0.0), s[0], s[1], "speckle");
    check(Map((size_t)s[0] * s[1], 7), s[0], s[1], "constant");
  }
  check(sawtooth(8, 700, 3), 8, 700, "sawtooth");
  check(sawtooth(12, 300, 5), 12, 300, "sawtooth");
  if (bad) return 1;
  printf("ok %d\n", cases);
  return 0;
}

static int baseline(int argc, char** argv) {
  if (argc != 9) {
    fprintf(stderr, "usage: outline_simplify_host --simplify FILE H W NR K TOLERANCE REPS\n");
    return 2;
  }
  const int H = atoi(argv[3]), W = atoi(argv[4]), NR = atoi(argv[5]), K = atoi(argv[6]), reps = atoi(argv[8]);
  const double t = atof(argv[7]);
  if (H < 1 || W < 1 || H > OS_MAX_SIDE || W > OS_MAX_SIDE || NR < 1 || K < NR || t < 0 || t > OS_MAX_SIDE || reps < 1) {
    fprintf(stderr, "outline_simplify_host: bad arguments\n");
    return 2;
  }
  std::vector<int> raw((size_t)H * W + NR + 1 + 2 * (size_t)K);
  FILE* f = fopen(argv[2], "rb");
  if (!f || fread(raw.data(), 4, raw.size(), f) != raw.size()) {
    fprintf(stderr, "outline_simplify_host: cannot read %zu ints from %s\n", raw.size(), argv[2]);
    return 2;
  }
  fclose(f);
  const Map m(raw.begin(), raw.begin() + (size_t)H * W);
  Rings rings;
  rings.offset.assign(raw.begin() + (size_t)H * W, raw.begin() + (size_t)H * W + NR + 1);
  const int* v = raw.data() + (size_t)H * W + NR + 1;
  for (int i = 0; i < K; ++i) rings.vx.push_back(v[2 * i]), rings.vy.push_back(v[2 * i + 1]);
  if (rings.offset[0] != 0 || rings.offset[NR] != K || !std::is_sorted(rings.offset.begin(), rings.offset.end())) {
    fprintf(stderr, "outline_simplify_host: ring offsets are not those of K corners\n");
    return 2;
  }
  for (int i = 0; i < K; ++i)
    if (rings.vx[i] < 0 || rings.vx[i] > W || rings.vy[i] < 0 || rings.vy[i] > H) {
      fprintf(stderr, "outline_simplify_host: a vertex lies outside the lattice\n");
      return 2;
    }
  std::string ms;
  Simplified out;
  for (int r = 0; r < reps; ++r) {
    const auto t0 = std::chrono::steady_clock::now();
    out = logic_simplify(m, H, W, rings, os_tol2_q4(t));
    const double dt = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    ms += (r ? ", " : "") + std::to_string(dt);
  }
  std::string hist;
  for (size_t b = 0; b < out.hist.size(); ++b) hist += (b ? ", " : "") + std::to_string(out.hist[b]);
  printf("{\"N\": %lld, \"K2\": %zu, \"arcs\": %lld, \"hist\": [%s], \"ms\": [%s]}\n", out.N, out.vx.size(), out.arcs,
         hist.c_str(), ms.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--simplify")) return baseline(argc, argv);
  return self_test();
}
