// The index and score logic of the outline simplifier (outline_simplify.hip), as host + device functions, so that
// tools/outline_simplify_host.cpp runs the very same code sequentially on the host against a brute-force
// recursive Douglas-Peucker before a kernel ever runs.  The contract is DESIGN.md section 4 ("Outline
// simplification").
//
// Lattice, directions and the four pixels q[0..3] = SW, NW, NE, SE round a vertex are those of
// region_outlines_logic.h.  A bit line is one lattice row or column of the junction bitmaps: bit p of the line is
// bit p % 64 of word p / 64.  A node is one int: x | y << 16 (x, y <= 16384).  Inside an arc of `len` edges the
// nodes are numbered 0 .. len; node 0 and node len are its ends (the same node for a closed arc).
#pragma once
#include <stdint.h>

#include "region_outlines_logic.h"

constexpr int OS_MAX_SIDE = 16384;                 // H, W and the tolerance: every product below fits an int64
constexpr int OS_BLOCK_LEN = 512;                  // arcs of at least this many edges take a workgroup, shorter a wave

// A junction: at least 3 of the (up to 4) lattice edges at the vertex are boundary edges, or a map corner.  The
// edge E lies between NE and SE, W between NW and SW, N between NW and NE, S between SW and SE; an absent pixel
// differs from every pixel.  q, have: ro_quad of the vertex.
RO_HD bool os_junction(const int q[4], unsigned have, int x, int y, int H, int W) {
  const bool l = x > 0, r = x < W, u = y > 0, b = y < H;
  const unsigned both01 = (have & 3u) == 3u, both23 = (have & 12u) == 12u, both12 = (have & 6u) == 6u,
                 both03 = (have & 9u) == 9u;
  const int deg = (int)(r && !(both23 && q[2] == q[3])) + (int)(l && !(both01 && q[0] == q[1])) +
                  (int)(u && !(both12 && q[1] == q[2])) + (int)(b && !(both03 && q[0] == q[3]));
  return deg >= 3 || ((x == 0 || x == W) && (y == 0 || y == H));
}

RO_HD int os_pack(int x, int y) { return x | (y << 16); }
RO_HD int os_x(int p) { return p & 0xffff; }
RO_HD int os_y(int p) { return (int)((unsigned)p >> 16); }
RO_HD int os_vkey(int p, int W) { return os_y(p) * (W + 1) + os_x(p); }

RO_HD bool os_bit(const unsigned long long* line, int p) { return (line[p >> 6] >> (p & 63)) & 1ull; }

// the number of set bits of a line strictly between positions a and b (either order), a word at a time
RO_HD int os_count_open(const unsigned long long* line, int a, int b) {
  const int lo = (a < b ? a : b) + 1, hi = (a < b ? b : a) - 1;   // the closed range [lo, hi]
  if (lo > hi) return 0;
  const int w0 = lo >> 6, w1 = hi >> 6;
  const unsigned long long first = ~ro_below(lo & 63), last = ro_below(hi & 63) | (1ull << (hi & 63));
  if (w0 == w1) return ro_popc(line[w0] & first & last);
  int n = ro_popc(line[w0] & first) + ro_popc(line[w1] & last);
  for (int w = w0 + 1; w < w1; ++w) n += ro_popc(line[w]);
  return n;
}

// the first set bit of a line after `pos` towards `end` and strictly before it, or -1; end > pos goes up, else down
RO_HD int os_next_open(const unsigned long long* line, int pos, int end) {
  if (end > pos) {
    const int hi = end - 1;
    if (pos + 1 > hi) return -1;
    int w = (pos + 1) >> 6;
    unsigned long long m = line[w] & ~ro_below((pos + 1) & 63);
    for (;;) {
      if (m) {
        const int p = w * RO_WORD + ro_ctz(m);
        return p <= hi ? p : -1;
      }
      if (++w > (hi >> 6)) return -1;
      m = line[w];
    }
  }
  const int lo = end + 1;
  if (pos - 1 < lo) return -1;
  int w = (pos - 1) >> 6;
  unsigned long long m = line[w] & (ro_below((pos - 1) & 63) | (1ull << ((pos - 1) & 63)));
  for (;;) {
    if (m) {
      const int p = w * RO_WORD + ro_top(m);
      return p >= lo ? p : -1;
    }
    if (--w < (lo >> 6)) return -1;
    m = line[w];
  }
}

// the first set bit of a line in [lo, hi), or -1
RO_HD int os_first_in(const unsigned long long* line, int lo, int hi) { return os_next_open(line, lo - 1, hi); }

// The ring of corner i: the last r in [0, nr) with ring_offset[r] <= i (ring_offset ascending, nr >= 1).  At most
// 32 halvings whatever the table holds.
RO_HD int os_ring_of(const int32_t* ring_offset, int nr, int i) {
  int lo = 0, hi = nr;                             // ring_offset[lo] <= i < ring_offset[hi], taken for granted at the ends
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const int mid = lo + (hi - lo) / 2;
    if (ring_offset[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// The candidate of one interior node for the split of a segment: larger score first, then the smaller vertex key,
// then (never on rings of a map, where no vertex repeats inside an arc) the smaller node number.
struct OsBest {
  long long score;
  int v, k;
};
RO_HD OsBest os_none() { return OsBest{-1, 0x7fffffff, 0x7fffffff}; }
RO_HD bool os_better(const OsBest& a, const OsBest& b) {     // a before b
  if (a.score != b.score) return a.score > b.score;
  if (a.v != b.v) return a.v < b.v;
  return a.k < b.k;
}
RO_HD OsBest os_pick(const OsBest& a, const OsBest& b) { return os_better(a, b) ? a : b; }

// score of node pk against the segment from pi to pj; the same number in either walking direction
RO_HD long long os_score(int pi, int pj, int pk) {
  const long long ax = os_x(pj) - os_x(pi), ay = os_y(pj) - os_y(pi);
  const long long bx = os_x(pk) - os_x(pi), by = os_y(pk) - os_y(pi);
  if (pi == pj) return bx * bx + by * by;
  const long long c = ax * by - ay * bx;
  return c * c;
}
RO_HD long long os_chord2(int pi, int pj) {
  if (pi == pj) return 1;
  const long long ax = os_x(pj) - os_x(pi), ay = os_y(pj) - os_y(pi);
  return ax * ax + ay * ay;
}
// every interior node lies within the tolerance: 16 m <= tol2_q4 * L  (m <= 2^58, tol2_q4 <= 2^32, L <= 2^29)
RO_HD bool os_within(long long m, long long chord2, long long tol2_q4) { return 16 * m <= tol2_q4 * chord2; }

RO_HD long long os_tol2_q4(double t) {             // round(16 t^2), 0 <= t <= OS_MAX_SIDE
  return (long long)(16.0 * t * t + 0.5);
}

// Douglas-Peucker over one arc of `len` edges with an explicit stack of open segments.
//   A.node(k)              the node k of the arc, k in 0 .. len
//   A.best(i, j, pi, pj)   os_pick over the interior nodes of segment (i, j): sequential on the host, lanes
//                          striding plus a cross-lane reduction on the device; the same value in every thread
//   A.push(sp, i, j), A.pop(sp, i, j)   entry sp of the arc's stack, sp in 0 .. len - 1
//   A.keep(k)              marks node k
// The segment at hand (i, j) stays in registers: a split goes on with its left part and pushes the right part
// only when that has an interior node, so an arc that never splits, or splits off single edges, never touches the
// stack.  Open segments are disjoint and have at least two edges each, so at most len / 2 are pending.  A round
// either splits, which keeps one of the len - 1 interior nodes, or closes the segment at hand, of which there is
// the first one, one per split (its left part) and one per pop (a right part): fewer than 2 len rounds.  Both
// bounds are enforced, so that no content of the stack's memory can make the loop run on.
template <class A>
RO_HD void os_douglas_peucker(A& arc, int len, long long tol2_q4) {
  int sp = 0, i = 0, j = len;
  for (int it = 0; it < 2 * len; ++it) {
    if (i >= 0 && j <= len && j - i >= 2) {
      const int pi = arc.node(i), pj = arc.node(j);
      const OsBest b = arc.best(i, j, pi, pj);
      if (b.k > i && b.k < j && !os_within(b.score, os_chord2(pi, pj), tol2_q4)) {
        arc.keep(b.k);
        if (j - b.k >= 2 && sp < len) arc.push(sp++, b.k, j);
        j = b.k;
        continue;
      }
    }
    if (sp == 0) return;
    arc.pop(--sp, i, j);
  }
}
