// The input stage for 8-bit YUV 4:2:0 video: what a decoder hands out -- NV12, I420 and their swapped kin -- goes
//   chroma at the luma pixel (bilinear, edge clamped, 'left' or 'center' siting) -> R'G'B' on the 0..255 scale, NOT clamped, NOT rounded ->
// and from there either
//   * fgvc_frames_yuv420_to_lab_f32: the steps of input.hip in the same arithmetic (input_lab.hpp) -- bilinear resize, / 255 and clamp,
//     sRGB -> Lab, normalise, written at (pad_top, pad_left) of a zero border -- in ONE launch, what datasets.preprocess_yuv420_frames defines;
//   * fgvc_frames_yuv420_to_rgb8: rint(clamp(R'G'B', 0, 255)) as packed bytes, what the render kernel draws on.
// The three planes are read in place: luma by frame and row stride (columns are adjacent), chroma by frame, row and PIXEL stride (1: I420's
// planes, 2: NV12's interleaved pairs), the same for u and v.
//   * a lane owns 4 consecutive columns of one output row, as in input.hip; its chroma columns and quarter weights are integers worked out
//     once (the position in quarter chroma samples is 2 x - 1 or 2 x: no float rounds) and reused over the workgroup's rows;
//   * same size: the lane's 4 luma bytes come as one dword where the address is aligned; chroma is 2 rows of at most 4 bytes per plane,
//     plain loads that the neighbouring lanes share through the vector cache;
//   * resize: each of the 4 luma taps of an output pixel is decoded at its own chroma position (decode first, then the fma nest of
//     input.hip on the unclamped R'G'B');
//   * the interpolated chroma has quarter steps, so no 256-entry table applies: the sRGB transfer is evaluated per value in both paths.
// No workspace, no atomics, no LDS, nothing allocates or synchronises.
#include "input_lab.hpp"
#include "yuv_taps.hpp"

namespace fgvc {

namespace {

struct YuvArgs {
  const uint8_t *y, *u, *v;
  void* out;
  long long yst, ysy;              // luma: byte strides of frame and row
  long long cst, csy, csx;         // chroma: of frame, row and pixel
  float y_off, cy, crv, cgu, cgv, cbu;
  int center;                      // siting: 0 = left (co-sited columns), 1 = center
  int h0, w0, ch, cw, h, w, left, top, hp, wp;
};

// (ChromaTap, chroma_tap: yuv_taps.hpp, shared with input_yuvp.hip)

// (every weight a multiple of 1/4, every sample an integer <= 255: exact whatever the order)
__device__ __forceinline__ float chroma_at(const uint8_t* r0, const uint8_t* r1, long long o0, long long o1, float lx, float ly) {
  const float c00 = (float)r0[o0], c01 = (float)r0[o1], c10 = (float)r1[o0], c11 = (float)r1[o1];
  const float top = (1.0f - lx) * c00 + lx * c01, bot = (1.0f - lx) * c10 + lx * c11;
  return (1.0f - ly) * top + ly * bot;
}

// the two chroma rows of each plane around one luma row, and the lower one's weight
struct ChromaRows {
  const uint8_t *u0, *u1, *v0, *v1;
  float l;
};

__device__ __forceinline__ ChromaRows chroma_rows(const YuvArgs& a, int t, int y) {
  const ChromaTap ty = chroma_tap(y, 1, a.ch);
  const long long f = (long long)t * a.cst, o0 = f + (long long)ty.i0 * a.csy, o1 = f + (long long)ty.i1 * a.csy;
  ChromaRows r;
  r.u0 = a.u + o0; r.u1 = a.u + o1; r.v0 = a.v + o0; r.v1 = a.v + o1; r.l = ty.l;
  return r;
}

// one luma value and its chroma -> R'G'B' (0..255 scale, unclamped): every operation rounded, none contracted
__device__ __forceinline__ void decode(const YuvArgs& a, float Y, const ChromaRows& c, const ChromaTap& tx, float (&rgb)[3]) {
  const long long o0 = (long long)tx.i0 * a.csx, o1 = (long long)tx.i1 * a.csx;
  const float U = chroma_at(c.u0, c.u1, o0, o1, tx.l, c.l), V = chroma_at(c.v0, c.v1, o0, o1, tx.l, c.l);
  const float yy = a.cy * (Y - a.y_off), cb = U - 128.0f, cr = V - 128.0f;
  rgb[0] = yy + a.crv * cr;
  rgb[1] = (yy + a.cgu * cb) + a.cgv * cr;
  rgb[2] = yy + a.cbu * cb;
}

// same size: the R'G'B' of the lane's 4 columns xi .. xi + 3 of luma row yi (columns off the frame keep 0)
__device__ __forceinline__ void decode_row4(const YuvArgs& a, int t, int yi, int xi, const bool (&cin)[4], const ChromaTap (&tx)[4],
                                            float (&v)[4][3]) {
  const uint8_t* p = a.y + (long long)t * a.yst + (long long)yi * a.ysy;
  const ChromaRows c = chroma_rows(a, t, yi);
  float Y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (cin[0] && cin[3] && ((unsigned)reinterpret_cast<uintptr_t>(p + xi) & 3u) == 0) {
    const uint32_t d = *reinterpret_cast<const uint32_t*>(p + xi);
#pragma unroll
    for (int j = 0; j < 4; ++j) Y[j] = (float)((d >> (8 * j)) & 255u);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (cin[j]) Y[j] = (float)p[xi + j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (cin[j]) decode(a, Y[j], c, tx[j], v[j]);
}

}  // namespace

template <bool RESIZE>
__global__ __launch_bounds__(IN_BLOCK) void frames_yuv420_to_lab_kernel(const YuvArgs a) {
  constexpr int NT = RESIZE ? 2 : 1;                                  // luma columns behind one output column
  const int xo = (blockIdx.x * IN_BLOCK + threadIdx.x) * 4;          // the lane's first column of the padded row
  if (xo >= a.wp) return;
  const int t = blockIdx.z;
  const int xi = xo - a.left;                                         // ... of the frame
  bool cin[4];
  int cx[4][NT];
  float cw0[4], cw1[4];
  ChromaTap tx[4][NT];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cin[j] = xi + j >= 0 && xi + j < a.w;
    cw0[j] = 1.0f;
    cw1[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < NT; ++k) cx[j][k] = 0;
    if (cin[j]) {
      if constexpr (RESIZE) bilinear_taps(xi + j, a.w0, a.w, cx[j][0], cx[j][NT - 1], cw0[j], cw1[j]);
      else cx[j][0] = xi + j;
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) tx[j][k] = chroma_tap(cx[j][k], a.center, a.cw);
  }
  const bool whole = xo + 3 < a.wp;
  const size_t plane = (size_t)a.hp * a.wp;
  float* out = static_cast<float*>(a.out);

  for (int r = 0; r < IN_ROWS; ++r) {
    const int yo = blockIdx.y * IN_ROWS + r;
    if (yo >= a.hp) break;
    const int yi = yo - a.top;
    float v[4][3];                                                    // R'G'B', 0 .. 255 scale, per column
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j][0] = v[j][1] = v[j][2] = 0.0f;
    const bool row_in = yi >= 0 && yi < a.h;
    if (row_in) {
      if constexpr (RESIZE) {
        int y0, y1;
        float wy0, wy1;
        bilinear_taps(yi, a.h0, a.h, y0, y1, wy0, wy1);
        const uint8_t* p0 = a.y + (long long)t * a.yst + (long long)y0 * a.ysy;
        const uint8_t* p1 = a.y + (long long)t * a.yst + (long long)y1 * a.ysy;
        const ChromaRows c0 = chroma_rows(a, t, y0), c1 = chroma_rows(a, t, y1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!cin[j]) continue;
          float v00[3], v01[3], v10[3], v11[3];
          decode(a, (float)p0[cx[j][0]], c0, tx[j][0], v00);
          decode(a, (float)p0[cx[j][NT - 1]], c0, tx[j][NT - 1], v01);
          decode(a, (float)p1[cx[j][0]], c1, tx[j][0], v10);
          decode(a, (float)p1[cx[j][NT - 1]], c1, tx[j][NT - 1], v11);
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const float top = fmaf(cw1[j], v01[c], cw0[j] * v00[c]), bot = fmaf(cw1[j], v11[c], cw0[j] * v10[c]);
            v[j][c] = fmaf(wy1, bot, wy0 * top);
          }
        }
      } else {
        ChromaTap t1[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t1[j] = tx[j][0];
        decode_row4(a, t, yi, xi, cin, t1, v);
      }
    }
    f32x4 o[3] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
#pragma unroll
    for (int j = 0; j < 4 && row_in; ++j) {                           // (a border row, the same for the whole workgroup: zeros, no arithmetic)
      float lin[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) lin[c] = srgb_to_linear(unit_of(v[j][c]));
      float l0, l1, l2;
      lab_normalised(lin[0], lin[1], lin[2], l0, l1, l2);
      const bool in = cin[j];                                         // the border is exactly 0
      o[0][j] = in ? l0 : 0.0f;
      o[1][j] = in ? l1 : 0.0f;
      o[2][j] = in ? l2 : 0.0f;
    }
    float* dst = out + (size_t)t * 3 * plane + (size_t)yo * a.wp + xo;
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

// packed bytes (T, h0, w0, 3): a lane's 4 pixels are 12 adjacent bytes, three dwords where their address is aligned
__global__ __launch_bounds__(IN_BLOCK) void frames_yuv420_to_rgb8_kernel(const YuvArgs a) {
  const int xi = (blockIdx.x * IN_BLOCK + threadIdx.x) * 4;
  if (xi >= a.w0) return;
  const int t = blockIdx.z;
  bool cin[4];
  ChromaTap tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cin[j] = xi + j < a.w0;
    tx[j] = chroma_tap(cin[j] ? xi + j : 0, a.center, a.cw);
  }
  uint8_t* out = static_cast<uint8_t*>(a.out);
  for (int r = 0; r < IN_ROWS; ++r) {
    const int yi = blockIdx.y * IN_ROWS + r;
    if (yi >= a.h0) break;
    float v[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j][0] = v[j][1] = v[j][2] = 0.0f;
    decode_row4(a, t, yi, xi, cin, tx, v);
    uint32_t b[12];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) b[3 * j + c] = (uint32_t)rintf(fminf(fmaxf(v[j][c], 0.0f), 255.0f));      // half to even
    uint8_t* dst = out + (((size_t)t * a.h0 + yi) * a.w0 + xi) * 3;
    if (cin[3] && ((unsigned)reinterpret_cast<uintptr_t>(dst) & 3u) == 0) {
      uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
      for (int k = 0; k < 3; ++k) d4[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (cin[j]) {
#pragma unroll
          for (int c = 0; c < 3; ++c) dst[3 * j + c] = (uint8_t)b[3 * j + c];
        }
    }
  }
}

namespace {

YuvArgs yuv_args(const uint8_t* y, const uint8_t* u, const uint8_t* v, int h0, int w0, long long yst, long long ysy, long long cst,
                 long long csy, long long csx, const float* coef, int siting, void* out) {
  YuvArgs a;
  a.y = y; a.u = u; a.v = v; a.out = out;
  a.yst = yst; a.ysy = ysy; a.cst = cst; a.csy = csy; a.csx = csx;
  a.y_off = coef[0]; a.cy = coef[1]; a.crv = coef[2]; a.cgu = coef[3]; a.cgv = coef[4]; a.cbu = coef[5];
  a.center = siting;
  a.h0 = h0; a.w0 = w0; a.ch = (h0 + 1) / 2; a.cw = (w0 + 1) / 2;
  a.h = h0; a.w = w0; a.left = 0; a.top = 0; a.hp = h0; a.wp = w0;
  return a;
}

}  // namespace

int frames_yuv420_to_lab_launch(const uint8_t* y, const uint8_t* u, const uint8_t* v, int T, int h0, int w0, long long yst, long long ysy,
                                long long cst, long long csy, long long csx, const float* coef, int siting, int h, int w, int left, int right,
                                int top, int bottom, float* out, hipStream_t s) {
  YuvArgs a = yuv_args(y, u, v, h0, w0, yst, ysy, cst, csy, csx, coef, siting, out);
  a.h = h; a.w = w; a.left = left; a.top = top;
  a.hp = top + h + bottom; a.wp = left + w + right;
  const dim3 grid(cdiv(cdiv(a.wp, 4), IN_BLOCK), cdiv(a.hp, IN_ROWS), T);
  if (h != h0 || w != w0) frames_yuv420_to_lab_kernel<true><<<grid, IN_BLOCK, 0, s>>>(a);
  else frames_yuv420_to_lab_kernel<false><<<grid, IN_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_frames_yuv420_to_lab_f32");
  return FGVC_OK;
}

int frames_yuv420_to_rgb8_launch(const uint8_t* y, const uint8_t* u, const uint8_t* v, int T, int h0, int w0, long long yst, long long ysy,
                                 long long cst, long long csy, long long csx, const float* coef, int siting, uint8_t* out, hipStream_t s) {
  const YuvArgs a = yuv_args(y, u, v, h0, w0, yst, ysy, cst, csy, csx, coef, siting, out);
  const dim3 grid(cdiv(cdiv(w0, 4), IN_BLOCK), cdiv(h0, IN_ROWS), T);
  frames_yuv420_to_rgb8_kernel<<<grid, IN_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_frames_yuv420_to_rgb8");
  return FGVC_OK;
}

}  // namespace fgvc
