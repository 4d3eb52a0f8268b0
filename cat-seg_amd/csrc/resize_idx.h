// The bilinear source taps shared by every resize kernel (preprocess, postprocess, the fused
// postprocess + argmax): one definition, so the kernels that must agree bit for bit do.
#pragma once
#include "common.h"

// torch bilinear, align_corners=False: src = max(scale*(dst+0.5)-0.5, 0), scale = in/out
DEV void lin_idx(int dst, int in_size, float scale, int& i0, int& i1, float& l1) {
  float src = scale * ((float)dst + 0.5f) - 0.5f;
  src = fmaxf(src, 0.f);
  i0 = (int)src;
  i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
  l1 = src - (float)i0;
}
