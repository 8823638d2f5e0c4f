// What the two input kernels share (input.hip: uint8 RGB; input_yuv.hip: Y'CbCr planes): the arithmetic from R'G'B' on the 0..255 scale to
// the normalised Lab planes, the resize taps and the launch geometry.  One definition, so that the same R'G'B' gives the same bits through
// either kernel (DESIGN.md sections 14 and 19).
#pragma once
#include <math.h>

#include "common.hpp"

// every product / sum below is written out (fmaf where one rounding is wanted): the padded and the unpadded call and every layout must give
// the same bits, whatever the optimiser would contract at one place and not at another
#pragma clang fp contract(off)

namespace fgvc {

namespace {

constexpr int IN_ROWS = 4;          // padded output rows per workgroup (one after another: the column taps are computed once)
constexpr int IN_BLOCK = 256;       // lanes per workgroup = 1024 columns

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));     // a row of the planar output starts at any 4-byte address

// datasets.rgb_to_lab, value by value: x in [0, 1]
__device__ __forceinline__ float srgb_to_linear(float x) {
  return x > 0.04045f ? powf((x + 0.055f) / 1.055f, 2.4f) : x / 12.92f;
}

__device__ __forceinline__ float unit_of(float v) { return fminf(fmaxf(v / 255.0f, 0.0f), 1.0f); }

__device__ __forceinline__ float lab_f(float t) { return t > 0.008856f ? cbrtf(t) : fmaf(7.787f, t, (float)(16.0 / 116.0)); }

// linear RGB -> the three normalised planes
__device__ __forceinline__ void lab_normalised(float r, float g, float b, float& o0, float& o1, float& o2) {
  const float X = fmaf(0.180423f, b, fmaf(0.357580f, g, 0.412453f * r)) / 0.950456f;
  const float Y = fmaf(0.072169f, b, fmaf(0.715160f, g, 0.212671f * r)) / 1.0f;
  const float Z = fmaf(0.950227f, b, fmaf(0.119193f, g, 0.019334f * r)) / 1.088754f;
  const float fx = lab_f(X), fy = lab_f(Y), fz = lab_f(Z);
  const float L = Y > 0.008856f ? fmaf(116.0f, fy, -16.0f) : 903.3f * Y;
  o0 = (L - 50.0f) / 50.0f;
  o1 = (500.0f * (fx - fy)) / 127.0f;
  o2 = (200.0f * (fy - fz)) / 127.0f;
}

// F.interpolate(mode='bilinear', align_corners=False) along one axis: output index o of n_out -> taps i0, i1 of n_in and their weights
__device__ __forceinline__ void bilinear_taps(int o, int n_in, int n_out, int& i0, int& i1, float& w0, float& w1) {
  double s = ((double)n_in / (double)n_out) * ((double)o + 0.5) - 0.5;
  s = s < 0.0 ? 0.0 : s;
  i0 = imin((int)s, n_in - 1);
  i1 = imin(i0 + 1, n_in - 1);
  const double l1 = fmin(fmax(s - (double)i0, 0.0), 1.0);
  w0 = (float)(1.0 - l1);
  w1 = (float)l1;
}

}  // namespace

}  // namespace fgvc
