// The chroma tap of a 2:1 subsampled axis, shared by input_yuv.hip (8-bit 4:2:0) and input_yuvp.hip (8..16 bits, 4:2:0 / 4:2:2 / 4:4:4): one
// definition, so that the same samples interpolate to the same value through either kernel (DESIGN.md sections 19 and 26).
#pragma once
#include "common.hpp"

namespace fgvc {

namespace {

struct ChromaTap {
  int i0, i1;
  float l;                         // weight of i1: a multiple of 1/4
};

// chroma samples around luma index p of an axis with n chroma samples: s = p / 2 - 0.25 (`back`) or p / 2, clamped to [0, n - 1]; in quarter
// samples that is the integer 2 p - 1 or 2 p
__device__ __forceinline__ ChromaTap chroma_tap(int p, int back, int n) {
  const int q = imax(imin(2 * p - back, 4 * (n - 1)), 0);
  ChromaTap t;
  t.i0 = q >> 2;
  t.i1 = imin(t.i0 + 1, n - 1);
  t.l = 0.25f * (float)(q & 3);
  return t;
}

}  // namespace

}  // namespace fgvc
