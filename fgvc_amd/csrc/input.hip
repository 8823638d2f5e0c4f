// The input stage: decoded uint8 RGB frames -> the network's planar f32 input in ONE launch,
//   bilinear resize (align_corners=False, no antialiasing, edge clamped) -> / 255, clamp -> sRGB -> linear -> XYZ -> CIE Lab (D65) ->
//   (x - [50, 0, 0]) / [50, 127, 127] -> written at (pad_top, pad_left) of a zero border,
// what datasets.preprocess_tapvid_frames (+ F.pad in the label-map calls) defines through some sixty element-wise torch launches.
//   * four byte strides: channels-last decoder output, planar tensors and non-contiguous crops of either are read in place;
//   * a lane owns 4 consecutive columns of one padded output row: its source coordinates and bilinear weights are computed in DOUBLE from the
//     integer sizes and rounded once (torch's f32 coordinates are what dominates the chain's own resize error), held in registers and
//     reused over the ROWS rows of its workgroup; everything after them is f32;
//   * one 16-byte store per plane and lane (a wave writes 1 KiB runs); a lane across the row's end stores its columns one by one;
//   * same size, channels-last: the lane's 12 source bytes come as three dwords (six halfwords) where the address is 4 (2) byte aligned;
//   * same size: only 256 inputs reach the sRGB transfer -- a table in LDS, built per workgroup by the SAME device function the resize path
//     calls (powf per value instead measured 0.078 ms against the table's 0.025 on 8 x 480 x 854: DESIGN.md section 14).
// No workspace, no atomics, nothing allocates or synchronises.
#include "input_lab.hpp"      // the R'G'B' -> Lab arithmetic, the resize taps and the launch geometry, shared with input_yuv.hip

namespace fgvc {

namespace {

struct InputArgs {
  const uint8_t* src;
  float* out;
  long long st, sy, sx, sc;        // byte strides of frame, row, column, channel
  int h0, w0, h, w, left, top, hp, wp;
};

}  // namespace

template <bool RESIZE>
__global__ __launch_bounds__(IN_BLOCK) void frames_rgb8_to_lab_kernel(const InputArgs a) {
  constexpr bool LUT = !RESIZE;                                       // same size: the values are the 256 bytes themselves
  __shared__ float lut[LUT ? 256 : 1];
  if constexpr (LUT) {
    lut[threadIdx.x] = srgb_to_linear(unit_of((float)threadIdx.x));
    __syncthreads();
  }
  const int xo = (blockIdx.x * IN_BLOCK + threadIdx.x) * 4;          // the lane's first column of the padded row
  if (xo >= a.wp) return;
  const int t = blockIdx.z;
  const int xi = xo - a.left;                                         // ... of the frame
  bool cin[4];
  int cx0[4], cx1[4];
  float cw0[4], cw1[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cin[j] = xi + j >= 0 && xi + j < a.w;
    cx0[j] = cx1[j] = xi + j;
    cw0[j] = 1.0f;
    cw1[j] = 0.0f;
    if (RESIZE && cin[j]) bilinear_taps(xi + j, a.w0, a.w, cx0[j], cx1[j], cw0[j], cw1[j]);
  }
  const bool all_in = cin[0] && cin[3];
  const bool whole = xo + 3 < a.wp;
  const bool packed = !RESIZE && a.sx == 3 && a.sc == 1;
  const uint8_t* frame = a.src + (long long)t * a.st;
  const size_t plane = (size_t)a.hp * a.wp;

  for (int r = 0; r < IN_ROWS; ++r) {
    const int yo = blockIdx.y * IN_ROWS + r;
    if (yo >= a.hp) break;
    const int yi = yo - a.top;
    float v[4][3];                                                    // 0 .. 255 per column and channel
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j][0] = v[j][1] = v[j][2] = 0.0f;
    const bool row_in = yi >= 0 && yi < a.h;
    if (row_in) {
      if constexpr (RESIZE) {
        int y0, y1;
        float wy0, wy1;
        bilinear_taps(yi, a.h0, a.h, y0, y1, wy0, wy1);
        const uint8_t* p0 = frame + (long long)y0 * a.sy;
        const uint8_t* p1 = frame + (long long)y1 * a.sy;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!cin[j]) continue;
          const long long o0 = (long long)cx0[j] * a.sx, o1 = (long long)cx1[j] * a.sx;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const long long oc = (long long)c * a.sc;
            const float v00 = (float)p0[o0 + oc], v01 = (float)p0[o1 + oc], v10 = (float)p1[o0 + oc], v11 = (float)p1[o1 + oc];
            const float top = fmaf(cw1[j], v01, cw0[j] * v00), bot = fmaf(cw1[j], v11, cw0[j] * v10);
            v[j][c] = fmaf(wy1, bot, wy0 * top);
          }
        }
      } else {
        const uint8_t* p = frame + (long long)yi * a.sy;
        const uint8_t* q = p + (long long)xi * 3;                     // (used on the packed route only)
        const unsigned al = (unsigned)reinterpret_cast<uintptr_t>(q);
        if (packed && all_in && (al & 1u) == 0) {
          uint32_t d[3];
          if ((al & 3u) == 0) {
            const uint32_t* q4 = reinterpret_cast<const uint32_t*>(q);
            d[0] = q4[0]; d[1] = q4[1]; d[2] = q4[2];
          } else {
            const uint16_t* q2 = reinterpret_cast<const uint16_t*>(q);
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = (uint32_t)q2[2 * k] | ((uint32_t)q2[2 * k + 1] << 16);
          }
#pragma unroll
          for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const int k = 3 * j + c;
              v[j][c] = (float)((d[k >> 2] >> (8 * (k & 3))) & 255u);
            }
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (!cin[j]) continue;
            const long long o = (long long)(xi + j) * a.sx;
#pragma unroll
            for (int c = 0; c < 3; ++c) v[j][c] = (float)p[o + (long long)c * a.sc];
          }
        }
      }
    }
    f32x4 o[3] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
    for (int j = 0; j < 4 && row_in; ++j) {                           // (a border row, the same for the whole workgroup: zeros, no arithmetic)
      float lin[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if constexpr (LUT) lin[c] = lut[(int)v[j][c]];
        else lin[c] = srgb_to_linear(unit_of(v[j][c]));
      }
      float l0, l1, l2;
      lab_normalised(lin[0], lin[1], lin[2], l0, l1, l2);
      const bool in = cin[j];                                         // the border is exactly 0
      o[0][j] = in ? l0 : 0.0f;
      o[1][j] = in ? l1 : 0.0f;
      o[2][j] = in ? l2 : 0.0f;
    }
    float* dst = a.out + (size_t)t * 3 * plane + (size_t)yo * a.wp + xo;
    if (whole) {
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<f32x4u*>(dst + c * plane) = o[c];
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (xo + j < a.wp) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[c * plane + j] = o[c][j];
        }
    }
  }
}

int frames_rgb8_to_lab_launch(const uint8_t* frames, int T, int h0, int w0, long long st, long long sy, long long sx, long long sc, int h,
                              int w, int left, int right, int top, int bottom, float* out, hipStream_t s) {
  InputArgs a;
  a.src = frames; a.out = out;
  a.st = st; a.sy = sy; a.sx = sx; a.sc = sc;
  a.h0 = h0; a.w0 = w0; a.h = h; a.w = w; a.left = left; a.top = top;
  a.hp = top + h + bottom; a.wp = left + w + right;
  const dim3 grid(cdiv(cdiv(a.wp, 4), IN_BLOCK), cdiv(a.hp, IN_ROWS), T);
  if (h != h0 || w != w0) frames_rgb8_to_lab_kernel<true><<<grid, IN_BLOCK, 0, s>>>(a);
  else frames_rgb8_to_lab_kernel<false><<<grid, IN_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_frames_rgb8_to_lab_f32");
  return FGVC_OK;
}

}  // namespace fgvc
