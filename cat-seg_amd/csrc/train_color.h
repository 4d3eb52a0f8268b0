// The colour operations of ColorAugSSDTransform as the host mapper computes them
// (cat_seg/data/transforms.py: _convert, _rgb_to_hsv_u8, _hsv_to_rgb_u8), one pixel at a time.
// Every expression is the numpy float32 expression in the same operation order, one rounding per
// operation: the including translation unit MUST be compiled without contraction of a * b + c into an
// fma (-ffp-contract=off / #pragma clang fp contract(off)), without fast-math, and with the correctly
// rounded float32 division.  np.round = rintf (half to even), numpy's float % = fmodf + the sign fix,
// // = floorf of the quotient, astype(uint8) of a clipped value = truncation.
// Host-callable as well, so the restatement can be checked on a CPU against numpy over all 2^24 colours.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef TRAIN_COLOR_FN
#define TRAIN_COLOR_FN __host__ __device__ inline
#endif

namespace train_color {

// numpy's float remainder (npy_divmod): the sign of the divisor
TRAIN_COLOR_FN float pymod(float a, float b) {
  float m = fmodf(a, b);
  if (m != 0.f) {
    if ((b < 0.f) != (m < 0.f)) m = m + b;
  } else {
    m = copysignf(0.f, b);
  }
  return m;
}

// ColorAugSSD._convert: clip(float32(px) * alpha + beta, 0, 255) truncated to uint8
TRAIN_COLOR_FN int convert(int px, float alpha, float beta) {
  float r = (float)px * alpha;
  r = r + beta;
  r = fminf(fmaxf(r, 0.f), 255.f);
  return (int)r;
}

TRAIN_COLOR_FN int round_clip(float x) {
  x = rintf(x);
  x = fminf(fmaxf(x, 0.f), 255.f);
  return (int)x;
}

// _rgb_to_hsv_u8: OpenCV's uint8 convention, H in [0, 180)
TRAIN_COLOR_FN void rgb_to_hsv(int ri, int gi, int bi, int& H, int& S, int& V) {
  const float r = (float)ri, g = (float)gi, b = (float)bi;
  const float v = fmaxf(fmaxf(r, g), b);
  const float mn = fminf(fminf(r, g), b);
  const float d = v - mn;
  const float s = v > 0.f ? (255.0f * d) / fmaxf(v, 1e-6f) : 0.f;
  const float dd = fmaxf(d, 1e-6f);
  float h;
  if (v == r) {
    h = (60.0f * (g - b)) / dd;
  } else if (v == g) {
    h = 120.0f + (60.0f * (b - r)) / dd;
  } else {
    h = 240.0f + (60.0f * (r - g)) / dd;
  }
  if (d == 0.f) h = 0.f;
  h = pymod(h, 360.0f);
  H = (int)pymod(rintf(h / 2.f), 180.f);
  S = (int)rintf(s);
  V = (int)v;
}

// _hsv_to_rgb_u8
TRAIN_COLOR_FN void hsv_to_rgb(int H, int S, int V, int& ro, int& go, int& bo) {
  const float h = (float)H * 2.0f;
  const float s = (float)S / 255.0f;
  const float v = (float)V;
  const float c = v * s;
  const float q = h / 60.0f;
  const float x = c * (1.f - fabsf(pymod(q, 2.f) - 1.f));
  const float m = v - c;
  const int k = ((int)floorf(q)) % 6;
  float r, g, b;
  switch (k) {
    case 0: r = c; g = x; b = 0.f; break;
    case 1: r = x; g = c; b = 0.f; break;
    case 2: r = 0.f; g = c; b = x; break;
    case 3: r = 0.f; g = x; b = c; break;
    case 4: r = x; g = 0.f; b = c; break;
    default: r = c; g = 0.f; b = x; break;
  }
  ro = round_clip(r + m);
  go = round_clip(g + m);
  bo = round_clip(b + m);
}

struct Record {
  int bright, order, contrast, sat, hue, hue_delta;
  float beta, c_alpha, s_alpha;
};

TRAIN_COLOR_FN void contrast(const Record& p, int& r, int& g, int& b) {
  if (!p.contrast) return;
  r = convert(r, p.c_alpha, 0.f);
  g = convert(g, p.c_alpha, 0.f);
  b = convert(b, p.c_alpha, 0.f);
}

TRAIN_COLOR_FN void saturation(const Record& p, int& r, int& g, int& b) {
  if (!p.sat) return;
  int H, S, V;
  rgb_to_hsv(r, g, b, H, S, V);
  S = convert(S, p.s_alpha, 0.f);
  hsv_to_rgb(H, S, V, r, g, b);
}

TRAIN_COLOR_FN void hue(const Record& p, int& r, int& g, int& b) {
  if (!p.hue) return;
  int H, S, V;
  rgb_to_hsv(r, g, b, H, S, V);
  H = (H + p.hue_delta) % 180;
  if (H < 0) H += 180;
  hsv_to_rgb(H, S, V, r, g, b);
}

// ColorAugSSD.apply_image with its draws pinned: brightness, then one of the two orders
TRAIN_COLOR_FN void apply(const Record& p, int& r, int& g, int& b) {
  if (p.bright) {
    r = convert(r, 1.0f, p.beta);
    g = convert(g, 1.0f, p.beta);
    b = convert(b, 1.0f, p.beta);
  }
  if (p.order) {
    contrast(p, r, g, b);
    saturation(p, r, g, b);
    hue(p, r, g, b);
  } else {
    saturation(p, r, g, b);
    hue(p, r, g, b);
    contrast(p, r, g, b);
  }
}

}  // namespace train_color
