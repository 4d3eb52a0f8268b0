// The index, union and key logic of the connected-region kernels (label_regions.hip), as host + device
// functions over a memory policy, so that tools/label_regions_host.cpp runs the very same code sequentially
// on the host (in any pixel order) against a brute-force flood fill before a kernel ever runs.
//
// A memory policy M has  int load(int i)  and  int fetch_min(int i, int v)  (returns the old value); on
// the device these are relaxed atomics of the scope the phase needs, on the host plain array accesses.
//
// Union-find with min-index roots: parent[i] <= i always (parent starts as i and is only ever lowered, by
// fetch_min), a root has parent[i] == i, and the root of a finished set is its smallest index.  Every loop
// below terminates by construction: cc_find follows strictly decreasing links, and every round of cc_union
// either ends or replaces one of its two non-negative indices by a strictly smaller one.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define CC_HD __host__ __device__ __forceinline__
#else
#define CC_HD inline
#endif

constexpr int CC_TILE = 64;                        // rows and columns of a tile of the tile-local phase

CC_HD int cc_fold(int l, int clamp) { return (clamp >= 0 && l >= clamp) ? clamp : l; }

// SPLIT: path splitting on the way (every visited index is re-hung under its grandparent, by fetch_min, so
// links still only descend): used where the same chains are walked many times (the tile phase, in LDS)
template <bool SPLIT = false, class M>
CC_HD int cc_find(M& m, int x) {
  for (;;) {
    const int p = m.load(x);
    if ((unsigned)p >= (unsigned)x) return x;       // a root (p == x); never follows a link that does not descend
    if (SPLIT) {
      const int g = m.load(p);
      if ((unsigned)g < (unsigned)p) m.fetch_min(x, g);
    }
    x = p;
  }
}

// joins the sets of a and b; the smaller root becomes the root of both
template <bool SPLIT = false, class M>
CC_HD void cc_union(M& m, int a, int b) {
  for (;;) {
    a = cc_find<SPLIT>(m, a);
    b = cc_find<SPLIT>(m, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }                                               // a > b, both roots when read
    const int old = m.fetch_min(a, b);
    if (old == a) return;                           // a was still a root and now hangs under b
    a = old;                                        // another union lowered parent[a] first: old < a, and
  }                                                 // parent[a] = min(old, b) keeps a with both; join old and b
}

// Tile-local phase.  A tile row's parent entries start at the first pixel of their horizontal run of equal
// label: starts = one bit per column, set where a run starts (column 0 always); the run start of column lx
// is the highest set bit at or below lx.  No union joins row neighbours.
CC_HD int cc_run_start(unsigned long long starts, int lx) {
  const unsigned long long below = starts & ((2ull << lx) - 1ull);   // lx = 63: 2 << 63 wraps to 0, - 1 = all ones
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)below);
#else
  return 63 - __builtin_clzll(below);
#endif
}

// One call per pixel (ly, lx) of a tile of tw valid columns, after the run-start initialisation; lab(i) is
// the folded label of local index i = ly * CC_TILE + lx, m the tile's parent array over the same indices.
// Joins the pixel with its upper neighbour of equal label unless the pair to its left joins the same two runs
// (left and upper-left pixel both of this label: that pair, or one further left, is joined), and under
// 8-connectivity with the upper diagonals where no 4-path through the two rows already joins them (upper
// neighbour equal: it is a row neighbour of both diagonals; left / right neighbour equal: it lies below the
// diagonal pixel and is joined to it as a straight pair).
template <class M, class L>
CC_HD void cc_tile_pixel(M& m, const L& lab, int ly, int lx, int tw, bool conn8) {
  if (ly == 0) return;
  const int i = ly * CC_TILE + lx;
  const int v = lab(i);
  const bool left = lx > 0 && lab(i - 1) == v;
  if (lab(i - CC_TILE) == v) {
    if (!left || lab(i - CC_TILE - 1) != v) cc_union<true>(m, i, i - CC_TILE);
  } else if (conn8) {
    if (lx > 0 && !left && lab(i - CC_TILE - 1) == v) cc_union<true>(m, i, i - CC_TILE - 1);
    if (lx + 1 < tw && lab(i + 1) != v && lab(i - CC_TILE + 1) == v) cc_union<true>(m, i, i - CC_TILE + 1);
  }
}

// after the joins: a run start looks its root up (and keeps it); afterwards every pixel of the run is two
// links from its root
template <class M, class L>
CC_HD void cc_tile_settle(M& m, const L& lab, int ly, int lx) {
  const int i = ly * CC_TILE + lx;
  if (lx == 0 || lab(i - 1) != lab(i)) m.fetch_min(i, cc_find<true>(m, i));
}

// Border phase.  g(y, x) is the folded label of a pixel of the map, m the global parent array over
// p = y * W + x.  Every pair of neighbouring pixels in different tiles crosses a vertical border (then one
// of them has x % CC_TILE == 0 and the other x - 1) or a horizontal one (y % CC_TILE == 0 and y - 1), so
// the two functions below, called for every such (y, x), see every cross-tile pair at least once.
//
// A straight pair is left out when the pair one step back along the border has the same two labels and
// lies in the same two tiles: both its pixels are then tile-local neighbours of this pair's pixels, and
// that pair (or, by the same argument, one further back) is joined.  A diagonal pair is left out when the
// straight neighbour across the border has the pixel's label: it is a 4-neighbour of the diagonal one, and
// they are joined in their tile or by the straight pair of the other border.
template <class M, class G>
CC_HD void cc_border_vertical(M& m, const G& g, int y, int x, int H, int W, bool conn8) {   // x % CC_TILE == 0, x > 0
  const int v = g(y, x), p = y * W + x;
  if (g(y, x - 1) == v) {
    if (!(y % CC_TILE != 0 && g(y - 1, x) == v && g(y - 1, x - 1) == v)) cc_union(m, p, p - 1);
  } else if (conn8) {
    if (y > 0 && g(y - 1, x - 1) == v) cc_union(m, p, p - W - 1);
    if (y + 1 < H && g(y + 1, x - 1) == v) cc_union(m, p, p + W - 1);
  }
}

template <class M, class G>
CC_HD void cc_border_horizontal(M& m, const G& g, int y, int x, int H, int W, bool conn8) {  // y % CC_TILE == 0, y > 0
  const int v = g(y, x), p = y * W + x;
  if (g(y - 1, x) == v) {
    if (!(x % CC_TILE != 0 && g(y, x - 1) == v && g(y - 1, x - 1) == v)) cc_union(m, p, p - W);
  } else if (conn8) {
    if (x > 0 && g(y - 1, x - 1) == v) cc_union(m, p, p - W - 1);
    if (x + 1 < W && g(y - 1, x + 1) == v) cc_union(m, p, p - W + 1);
  }
}

// Compaction: region number of a root from the exclusive scan of the root counts per 64 pixels (seg_off)
// and the root flags of the root's 64 pixels (mask): roots before it in row-major order.
CC_HD int cc_region_id(int seg_off, unsigned long long mask, int root) {
  const unsigned long long below = mask & ((1ull << (root & 63)) - 1ull);
#if defined(__HIP_DEVICE_COMPILE__)
  return seg_off + __popcll(below);
#else
  return seg_off + __builtin_popcountll(below);
#endif
}

// score -> Q16 fixed point, ties to even; the table's score_q16 is the integer sum of these
CC_HD long long cc_score_q16(float s) { return (long long)__builtin_rintf(s * 65536.0f); }

// Sieve.  A small region's key is the maximum over its large neighbours of (area << 32) | (0xffffffff - root):
// the largest area wins, ties go to the smallest root = the smallest region number; 0 = no large neighbour.
CC_HD unsigned long long cc_key(int area, int root) {
  return ((unsigned long long)(unsigned)area << 32) | (unsigned long long)(0xffffffffu - (unsigned)root);
}
CC_HD int cc_key_root(unsigned long long key) { return (int)(0xffffffffu - (unsigned)key); }

// one neighbour pair of roots rp != rq with areas ap, aq: posts the large side's key to the small side.
// K has  void fetch_max(int i, unsigned long long v).
template <class K>
CC_HD void cc_sieve_pair(K& keys, int rp, int ap, int rq, int aq, int min_area) {
  if (ap < min_area && aq >= min_area) keys.fetch_max(rp, cc_key(aq, rq));
  else if (aq < min_area && ap >= min_area) keys.fetch_max(rq, cc_key(ap, rp));
}

// the root whose label a pixel of the region with root r takes: its own, or the winning large neighbour's
CC_HD int cc_sieve_source(int r, int area, unsigned long long key, int min_area) {
  return (area < min_area && key != 0ull) ? cc_key_root(key) : r;
}
