// The index logic of the region-outline kernels (region_outlines.hip), as host + device functions, so that
// tools/region_outlines_host.cpp runs the very same code sequentially on the host against a brute-force
// tracer before a kernel ever runs.  The contract is DESIGN.md section 4 ("Region outlines").
//
// Lattice: vertex (x, y), x in 0..W, y in 0..H, is the top-left corner of pixel (y, x).  Directions E=0, S=1,
// W=2, N=3.  The four pixels round a vertex, in the order this file uses everywhere:
//   q[0] = SW (y, x-1)   q[1] = NW (y-1, x-1)   q[2] = NE (y-1, x)   q[3] = SE (y, x)
// so that for an edge ARRIVING at the vertex with direction d
//   q[d] is the pixel on its right (the ring's value r), q[d+1] the one on its left,
//   q[d+2] the pixel ahead-left (b) and q[d+3] the pixel ahead-right (a), indices mod 4.
// A pixel outside the map is "absent": it equals nothing.
//
// Corners are numbered in key order, key = (y * (W + 1) + x) * 4 + d_in.  The vertices of a lattice row are cut
// into words of 64 (RO_WORD): word w = y * row_words + x / 64 holds one 64-bit mask per incoming direction
// (bit x % 64 = the vertex has a corner with that d_in) and, after the scan, the number of corners before it.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RO_HD __host__ __device__ __forceinline__
#else
#define RO_HD inline
#endif

constexpr int RO_WORD = 64;                        // lattice vertices of one mask word

RO_HD int ro_popc(unsigned long long v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(v);
#else
  return __builtin_popcountll(v);
#endif
}
RO_HD int ro_ctz(unsigned long long v) {           // v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return __ffsll((long long)v) - 1;
#else
  return __builtin_ctzll(v);
#endif
}
RO_HD int ro_top(unsigned long long v) {           // index of the highest set bit, v != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)v);
#else
  return 63 - __builtin_clzll(v);
#endif
}
RO_HD unsigned long long ro_below(int b) { return (1ull << b) - 1ull; }          // bits [0, b), b in 0..63
RO_HD unsigned long long ro_above(int b) { return ~ro_below(b) & ~(1ull << b); }   // bits (b, 63]

// the four pixels round vertex (x, y) of the map g(y, x): values into q, bit i of the result = q[i] exists
template <class G>
RO_HD unsigned ro_quad(const G& g, int x, int y, int H, int W, int q[4]) {
  const bool l = x > 0, r = x < W, u = y > 0, b = y < H;
  q[0] = (l && b) ? g(y, x - 1) : 0;
  q[1] = (l && u) ? g(y - 1, x - 1) : 0;
  q[2] = (r && u) ? g(y - 1, x) : 0;
  q[3] = (r && b) ? g(y, x) : 0;
  return (unsigned)(l && b) | (unsigned)(l && u) << 1 | (unsigned)(r && u) << 2 | (unsigned)(r && b) << 3;
}

// The corners of a vertex: bit d of the result = an edge arriving with direction d is a boundary edge and the
// ring turns here; bits 4 + 2 d, 5 + 2 d = its outgoing direction.
//   a == r and b == r   left        a == r and b != r   straight (no corner)
//   a != r and b == r   the diagonal pinch: left under connectivity 8, right under 4
//   a != r and b != r   right
RO_HD unsigned ro_corners(const int q[4], unsigned have, bool conn8) {
  unsigned code = 0;
  for (int d = 0; d < 4; ++d) {
    const int ir = d, il = (d + 1) & 3, ib = (d + 2) & 3, ia = (d + 3) & 3;
    if (!((have >> ir) & 1u)) continue;
    const int r = q[ir];
    if (((have >> il) & 1u) && q[il] == r) continue;        // no boundary edge arrives with d
    const bool a = ((have >> ia) & 1u) && q[ia] == r;
    const bool b = ((have >> ib) & 1u) && q[ib] == r;
    if (a && !b) continue;
    const int out = b ? ((a || conn8) ? (d + 3) & 3 : (d + 1) & 3) : (d + 1) & 3;
    code |= 1u << d | (unsigned)out << (4 + 2 * d);
  }
  return code;
}
RO_HD bool ro_is_corner(unsigned code, int d) { return (code >> d) & 1u; }
RO_HD int ro_out(unsigned code, int d) { return (int)(code >> (4 + 2 * d)) & 3; }

// number of the corner (bit, d) of a word: off = corners before the word, m[d] = the word's four masks
RO_HD int ro_corner_index(int off, const unsigned long long m[4], int bit, int d) {
  const unsigned long long lo = ro_below(bit);
  int i = off + ro_popc(m[0] & lo) + ro_popc(m[1] & lo) + ro_popc(m[2] & lo) + ro_popc(m[3] & lo);
  for (int e = 0; e < d; ++e) i += (int)((m[e] >> bit) & 1ull);
  return i;
}

// The successor of a corner at vertex (x, y) leaving with direction o: the first vertex along that ray that has a
// corner with d_in == o (the edges between go straight, and a directed edge bounds one value only, so no corner
// of another ring with that d_in lies between).  A bitmap policy B has
//   unsigned long long row(int d, int y, int xw)   the mask of direction d of word xw of lattice row y  (d = 0, 2)
//   unsigned long long col(int d, int x, int yw)   bit y % 64 of word yw of lattice column x           (d = 1, 3)
// and is walked a word at a time: no step depends on the run's length in vertices, only in words.
// Returns the coordinate that changes along the ray (x for E / W, y for S / N), or -1 when the bitmaps hold none
// (never for bitmaps made from a map).
template <class B>
RO_HD int ro_successor(const B& bits, int x, int y, int o, int H, int W) {
  const int row_words = (W + RO_WORD) / RO_WORD, col_words = (H + RO_WORD) / RO_WORD;   // ceil((W + 1) / 64)
  if (o == 0) {
    unsigned long long m = bits.row(0, y, x >> 6) & ro_above(x & 63);
    for (int w = x >> 6;;) {
      if (m) return w * RO_WORD + ro_ctz(m);
      if (++w >= row_words) return -1;
      m = bits.row(0, y, w);
    }
  } else if (o == 2) {
    unsigned long long m = bits.row(2, y, x >> 6) & ro_below(x & 63);
    for (int w = x >> 6;;) {
      if (m) return w * RO_WORD + ro_top(m);
      if (--w < 0) return -1;
      m = bits.row(2, y, w);
    }
  } else if (o == 1) {
    unsigned long long m = bits.col(1, x, y >> 6) & ro_above(y & 63);
    for (int w = y >> 6;;) {
      if (m) return w * RO_WORD + ro_ctz(m);
      if (++w >= col_words) return -1;
      m = bits.col(1, x, w);
    }
  } else {
    unsigned long long m = bits.col(3, x, y >> 6) & ro_below(y & 63);
    for (int w = y >> 6;;) {
      if (m) return w * RO_WORD + ro_top(m);
      if (--w < 0) return -1;
      m = bits.col(3, x, w);
    }
  }
}

// Ring ranking by pointer jumping.  The state of corner i after r rounds describes the 2^r corners from i on
// along its ring: nxt = the corner 2^r steps ahead, mn = the smallest corner number among them, off = the number
// of steps from i to the first occurrence of mn.  Round r joins the window of i with the window of nxt (which
// starts 2^r steps ahead); on a tie (the same corner seen again after a lap) the nearer occurrence stays.  After
// ceil(log2 K) rounds the window covers the ring: mn is the ring's start, off the distance from i forward to it.
struct RoJump {
  int nxt, mn, off;
};
RO_HD RoJump ro_jump(const RoJump& a, const RoJump& b, int round) {
  RoJump o;
  o.nxt = b.nxt;
  const bool take = b.mn < a.mn;
  o.mn = take ? b.mn : a.mn;
  o.off = take ? (int)((1u << round) + (unsigned)b.off) : a.off;
  return o;
}
RO_HD int ro_rounds(int64_t K) {                   // the smallest R with 2^R >= K
  int r = 0;
  while (((int64_t)1 << r) < K) ++r;
  return r;
}
// length of a ring from the distance-to-start of the corner after the start, and a corner's position in it
RO_HD int ro_ring_length(int off_after_start) { return off_after_start + 1; }
RO_HD int ro_rank(int length, int off) { return off == 0 ? 0 : length - off; }

// one term of the shoelace sum, vertex (x0, y0) followed by (x1, y1)
RO_HD long long ro_area_term(int x0, int y0, int x1, int y1) {
  return (long long)x0 * (long long)y1 - (long long)x1 * (long long)y0;
}
