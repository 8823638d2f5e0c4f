// The input stage for planar and semi-planar Y'CbCr at 8 to 16 bits, subsampled 4:2:0, 4:2:2 or 4:4:4: input_yuv.hip's
// two kernels generalised over
//   * the sample type S (uint8_t | uint16_t; every stride is in SAMPLES): a sample is (word >> shift) & (2^depth - 1) -- P010's six low bits
//     and the bits above a low-aligned sample's depth never reach the arithmetic;
//   * the subsampling per axis (sub_x, sub_y in {1, 2}, wave-uniform arguments): a subsampled axis uses chroma_tap as it stands (vertically
//     between the rows, horizontally by the siting, edge clamped), a full-resolution axis the luma index itself with weight 0 -- the blend
//     (1 - 0) c + 0 c is c, exactly;
//   * the constants of the depth: seven coefficients by value, the chroma offset (2^(depth - 1)) among them.
// Samples are integers below 2^16 and the blend weights sixteenths: the interpolated chroma has at most 20 bits, exact in f32 in any order.
//   * fgvc_frames_yuvp_to_lab_f32: ... -> R'G'B' (0..255 scale, unclamped) -> input_lab.hpp's steps, ONE launch (datasets.preprocess_yuv_frames);
//   * fgvc_frames_yuvp_to_rgb8: rint(clamp(R'G'B', 0, 255)) as packed bytes (datasets.yuv_to_rgb8).
// A lane owns 4 consecutive columns, a workgroup IN_ROWS rows one after another; same size: the lane's 4 luma samples come as one 4- or
// 8-byte load where the address is aligned to it.  No workspace, no atomics, no LDS, nothing allocates or synchronises.
#include "input_lab.hpp"
#include "yuv_taps.hpp"

#pragma clang fp contract(off)

namespace fgvc {

namespace {

template <typename S>
struct YuvpArgs {
  const S *y, *u, *v;
  void* out;
  long long yst, ysy;              // luma: strides of frame and row, in samples
  long long cst, csy, csx;         // chroma: of frame, row and pixel
  float y_off, cy, c_off, crv, cgu, cgv, cbu;
  unsigned shift, mask;            // sample = (word >> shift) & mask
  int sub_x, sub_y;                // 1 | 2
  int center;                      // siting of a subsampled horizontal axis: 0 = left, 1 = center
  int h0, w0, ch, cw, h, w, left, top, hp, wp;
};

// the tap of one axis: chroma_tap where it is subsampled, else the luma index alone (weight 0: no arithmetic changes the sample)
__device__ __forceinline__ ChromaTap axis_tap(int p, int sub, int back, int n) {
  if (sub == 2) return chroma_tap(p, back, n);
  ChromaTap t;
  t.i0 = t.i1 = imin(p, n - 1);
  t.l = 0.0f;
  return t;
}

template <typename S>
__device__ __forceinline__ float sample_of(const YuvpArgs<S>& a, S word) {
  return (float)(((unsigned)word >> a.shift) & a.mask);
}

// (every weight a multiple of 1/4, every sample an integer < 2^16: exact whatever the order)
template <typename S>
__device__ __forceinline__ float chroma_at(const YuvpArgs<S>& a, const S* r0, const S* r1, long long o0, long long o1, float lx, float ly) {
  const float c00 = sample_of(a, r0[o0]), c01 = sample_of(a, r0[o1]), c10 = sample_of(a, r1[o0]), c11 = sample_of(a, r1[o1]);
  const float top = (1.0f - lx) * c00 + lx * c01, bot = (1.0f - lx) * c10 + lx * c11;
  return (1.0f - ly) * top + ly * bot;
}

// the two chroma rows of each plane around one luma row, and the lower one's weight
template <typename S>
struct ChromaRows {
  const S *u0, *u1, *v0, *v1;
  float l;
};

template <typename S>
__device__ __forceinline__ ChromaRows<S> chroma_rows(const YuvpArgs<S>& a, int t, int y) {
  const ChromaTap ty = axis_tap(y, a.sub_y, 1, a.ch);
  const long long f = (long long)t * a.cst, o0 = f + (long long)ty.i0 * a.csy, o1 = f + (long long)ty.i1 * a.csy;
  ChromaRows<S> r;
  r.u0 = a.u + o0; r.u1 = a.u + o1; r.v0 = a.v + o0; r.v1 = a.v + o1; r.l = ty.l;
  return r;
}

// one luma value and its chroma -> R'G'B' (0..255 scale, unclamped): every operation rounded, none contracted
template <typename S>
__device__ __forceinline__ void decode(const YuvpArgs<S>& a, float Y, const ChromaRows<S>& c, const ChromaTap& tx, float (&rgb)[3]) {
  const long long o0 = (long long)tx.i0 * a.csx, o1 = (long long)tx.i1 * a.csx;
  const float U = chroma_at(a, c.u0, c.u1, o0, o1, tx.l, c.l), V = chroma_at(a, c.v0, c.v1, o0, o1, tx.l, c.l);
  const float yy = a.cy * (Y - a.y_off), cb = U - a.c_off, cr = V - a.c_off;
  rgb[0] = yy + a.crv * cr;
  rgb[1] = (yy + a.cgu * cb) + a.cgv * cr;
  rgb[2] = yy + a.cbu * cb;
}

// the lane's 4 adjacent luma words as one load: a dword of bytes, two dwords of 16-bit words
__device__ __forceinline__ void load4(const uint8_t* p, unsigned (&w)[4]) {
  const uint32_t d = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = (d >> (8 * j)) & 255u;
}

__device__ __forceinline__ void load4(const uint16_t* p, unsigned (&w)[4]) {
  const uint2 d = *reinterpret_cast<const uint2*>(p);
  w[0] = d.x & 65535u; w[1] = d.x >> 16; w[2] = d.y & 65535u; w[3] = d.y >> 16;
}

// same size: the R'G'B' of the lane's 4 columns xi .. xi + 3 of luma row yi (columns off the frame keep 0)
template <typename S>
__device__ __forceinline__ void decode_row4(const YuvpArgs<S>& a, int t, int yi, int xi, const bool (&cin)[4], const ChromaTap (&tx)[4],
                                            float (&v)[4][3]) {
  const S* p = a.y + (long long)t * a.yst + (long long)yi * a.ysy;
  const ChromaRows<S> c = chroma_rows(a, t, yi);
  float Y[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (cin[0] && cin[3] && ((unsigned)reinterpret_cast<uintptr_t>(p + xi) & (4u * sizeof(S) - 1u)) == 0) {
    unsigned w[4];
    load4(p + xi, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) Y[j] = (float)((w[j] >> a.shift) & a.mask);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (cin[j]) Y[j] = sample_of(a, p[xi + j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (cin[j]) decode(a, Y[j], c, tx[j], v[j]);
}

}  // namespace

template <typename S, bool RESIZE>
__global__ __launch_bounds__(IN_BLOCK) void frames_yuvp_to_lab_kernel(const YuvpArgs<S> a) {
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
    for (int k = 0; k < NT; ++k) tx[j][k] = axis_tap(cx[j][k], a.sub_x, a.center, a.cw);
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
        const S* p0 = a.y + (long long)t * a.yst + (long long)y0 * a.ysy;
        const S* p1 = a.y + (long long)t * a.yst + (long long)y1 * a.ysy;
        const ChromaRows<S> c0 = chroma_rows(a, t, y0), c1 = chroma_rows(a, t, y1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!cin[j]) continue;
          float v00[3], v01[3], v10[3], v11[3];
          decode(a, sample_of(a, p0[cx[j][0]]), c0, tx[j][0], v00);
          decode(a, sample_of(a, p0[cx[j][NT - 1]]), c0, tx[j][NT - 1], v01);
          decode(a, sample_of(a, p1[cx[j][0]]), c1, tx[j][0], v10);
          decode(a, sample_of(a, p1[cx[j][NT - 1]]), c1, tx[j][NT - 1], v11);
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
template <typename S>
__global__ __launch_bounds__(IN_BLOCK) void frames_yuvp_to_rgb8_kernel(const YuvpArgs<S> a) {
  const int xi = (blockIdx.x * IN_BLOCK + threadIdx.x) * 4;
  if (xi >= a.w0) return;
  const int t = blockIdx.z;
  bool cin[4];
  ChromaTap tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cin[j] = xi + j < a.w0;
    tx[j] = axis_tap(cin[j] ? xi + j : 0, a.sub_x, a.center, a.cw);
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

template <typename S>
YuvpArgs<S> yuvp_args(const void* y, const void* u, const void* v, int depth, int shift, int sub_x, int sub_y, int h0, int w0, long long yst,
                      long long ysy, long long cst, long long csy, long long csx, const float* coef, int siting, void* out) {
  YuvpArgs<S> a;
  a.y = static_cast<const S*>(y); a.u = static_cast<const S*>(u); a.v = static_cast<const S*>(v); a.out = out;
  a.yst = yst; a.ysy = ysy; a.cst = cst; a.csy = csy; a.csx = csx;
  a.y_off = coef[0]; a.cy = coef[1]; a.c_off = coef[2]; a.crv = coef[3]; a.cgu = coef[4]; a.cgv = coef[5]; a.cbu = coef[6];
  a.shift = (unsigned)shift; a.mask = (1u << depth) - 1u;
  a.sub_x = sub_x; a.sub_y = sub_y;
  a.center = siting;
  a.h0 = h0; a.w0 = w0; a.ch = (h0 + sub_y - 1) / sub_y; a.cw = (w0 + sub_x - 1) / sub_x;
  a.h = h0; a.w = w0; a.left = 0; a.top = 0; a.hp = h0; a.wp = w0;
  return a;
}

template <typename S>
void lab_launch(YuvpArgs<S> a, int T, int h, int w, int left, int right, int top, int bottom, hipStream_t s) {
  const bool resize = h != a.h0 || w != a.w0;
  a.h = h; a.w = w; a.left = left; a.top = top;
  a.hp = top + h + bottom; a.wp = left + w + right;
  const dim3 grid(cdiv(cdiv(a.wp, 4), IN_BLOCK), cdiv(a.hp, IN_ROWS), T);
  if (resize) frames_yuvp_to_lab_kernel<S, true><<<grid, IN_BLOCK, 0, s>>>(a);
  else frames_yuvp_to_lab_kernel<S, false><<<grid, IN_BLOCK, 0, s>>>(a);
}

}  // namespace

int frames_yuvp_to_lab_launch(const void* y, const void* u, const void* v, int sample_bytes, int depth, int shift, int sub_x, int sub_y, int T,
                              int h0, int w0, long long yst, long long ysy, long long cst, long long csy, long long csx, const float* coef,
                              int siting, int h, int w, int left, int right, int top, int bottom, float* out, hipStream_t s) {
  if (sample_bytes == 2)
    lab_launch(yuvp_args<uint16_t>(y, u, v, depth, shift, sub_x, sub_y, h0, w0, yst, ysy, cst, csy, csx, coef, siting, out), T, h, w, left,
               right, top, bottom, s);
  else
    lab_launch(yuvp_args<uint8_t>(y, u, v, depth, shift, sub_x, sub_y, h0, w0, yst, ysy, cst, csy, csx, coef, siting, out), T, h, w, left,
               right, top, bottom, s);
  FGVC_CHECK_LAUNCH("fgvc_frames_yuvp_to_lab_f32");
  return FGVC_OK;
}

int frames_yuvp_to_rgb8_launch(const void* y, const void* u, const void* v, int sample_bytes, int depth, int shift, int sub_x, int sub_y, int T,
                               int h0, int w0, long long yst, long long ysy, long long cst, long long csy, long long csx, const float* coef,
                               int siting, uint8_t* out, hipStream_t s) {
  const dim3 grid(cdiv(cdiv(w0, 4), IN_BLOCK), cdiv(h0, IN_ROWS), T);
  if (sample_bytes == 2)
    frames_yuvp_to_rgb8_kernel<uint16_t><<<grid, IN_BLOCK, 0, s>>>(
        yuvp_args<uint16_t>(y, u, v, depth, shift, sub_x, sub_y, h0, w0, yst, ysy, cst, csy, csx, coef, siting, out));
  else
    frames_yuvp_to_rgb8_kernel<uint8_t><<<grid, IN_BLOCK, 0, s>>>(
        yuvp_args<uint8_t>(y, u, v, depth, shift, sub_x, sub_y, h0, w0, yst, ysy, cst, csy, csx, coef, siting, out));
  FGVC_CHECK_LAUNCH("fgvc_frames_yuvp_to_rgb8");
  return FGVC_OK;
}

}  // namespace fgvc
