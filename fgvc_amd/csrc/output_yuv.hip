// The output stage for 8-bit YUV 4:2:0 video, the mirror image of input_yuv.hip: packed or planar RGB bytes ->
//   Y' at every pixel; the R, G, B bytes filtered to the chroma position ('left' or 'center' siting, edge clamped) -> Cb, Cr
// as bytes, rint (half to even) of the value clamped to [0, 255] -- what datasets.rgb8_to_yuv420 defines, byte for byte: every f32 operation
// rounded, none contracted, in its order.  One launch for all frames.
// The frames are read in place through frame, row, pixel and channel strides; luma is written by frame and row stride, chroma by frame, row
// and PIXEL stride (1: I420's planes, 2: NV12's interleaved pairs), the same for u and v.
//   * a lane owns one chroma row and 4 chroma columns = 2 luma rows x 8 luma columns: 48 source bytes, as 6 dwords a row where the pixels are
//     packed ('thwc') or 2 dwords a channel where they are planar ('tchw') and the address is aligned; bytes at a ragged right edge and in
//     unaligned views, with the column index clamped to the frame -- which IS the edge clamp of the chroma taps;
//   * 'left' siting reaches one column back (2 i - 1): a plain byte load per channel that the neighbouring lane's cache line serves;
//   * it stores 8 Y bytes per row as one 8-byte word, and 4 U + 4 V bytes as two dwords (planes) or 8 interleaved bytes as one word (pairs, in
//     either order: NV12 or NV21) where the address is aligned; bytes otherwise.
// No workspace, no atomics, no LDS, nothing allocates or synchronises.
#include "common.hpp"

// the host restatement is one rounded operation after another: a contracted multiply-add keeps the product's rounding error and flips bytes at
// exact ties (full-range saturated colours land on 128 +- 127.5)
#pragma clang fp contract(off)

namespace fgvc {

namespace {

constexpr int YO_LANES_X = 64;                  // lanes along a row: 64 x 8 = 512 luma columns per workgroup
constexpr int YO_LANES_Y = 4;                   // chroma rows per workgroup = 8 luma rows
constexpr int YO_BLOCK = YO_LANES_X * YO_LANES_Y;
constexpr int YO_COLS = YO_LANES_X * 8;
constexpr int YO_ROWS = YO_LANES_Y * 2;

typedef uint32_t u32x2u __attribute__((ext_vector_type(2), aligned(4)));

struct YuvOutArgs {
  const uint8_t* src;
  uint8_t *y, *u, *v;
  long long st, sy, sx, sc;         // source: byte strides of frame, row, pixel and channel
  long long yst, ysy;               // luma: of frame and row
  long long cst, csy, csx;          // chroma: of frame, row and pixel
  float kr, kg, kb, y_off, s_y, cu, cv;
  int h0, w0, ch, cw;
};

__device__ __forceinline__ bool aligned4(const void* p) { return ((unsigned)reinterpret_cast<uintptr_t>(p) & 3u) == 0; }

__device__ __forceinline__ float byte_of(const uint32_t* d, int i) { return (float)((d[i >> 2] >> (8 * (i & 3))) & 255u); }

__device__ __forceinline__ uint32_t to_byte(float x) { return (uint32_t)rintf(fminf(fmaxf(x, 0.0f), 255.0f)); }      // half to even

__device__ __forceinline__ uint32_t pack4(uint32_t b0, uint32_t b1, uint32_t b2, uint32_t b3) { return b0 | (b1 << 8) | (b2 << 16) | (b3 << 24); }

__device__ __forceinline__ float lum(const YuvOutArgs& a, float R, float G, float B) { return (a.kr * R + a.kg * G) + a.kb * B; }

// columns x0 - 1 (with LEFT) and x0 .. x0 + 7 of one source row -> px[0] and px[1 .. 8]; a column off the frame repeats the nearest one inside
template <bool LEFT>
__device__ __forceinline__ void load_row(const YuvOutArgs& a, const uint8_t* row, int x0, bool whole, float (&px)[9][3]) {
  const uint8_t* p = row + (long long)x0 * a.sx;
  if (whole && a.sx == 3 && a.sc == 1 && aligned4(p)) {
    uint32_t d[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) d[i] = reinterpret_cast<const uint32_t*>(p)[i];
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int c = 0; c < 3; ++c) px[1 + k][c] = byte_of(d, 3 * k + c);
  } else if (whole && a.sx == 1 && aligned4(p) && aligned4(p + a.sc) && aligned4(p + 2 * a.sc)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t d[2];
      d[0] = reinterpret_cast<const uint32_t*>(p + c * a.sc)[0];
      d[1] = reinterpret_cast<const uint32_t*>(p + c * a.sc)[1];
#pragma unroll
      for (int k = 0; k < 8; ++k) px[1 + k][c] = byte_of(d, k);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const uint8_t* q = row + (long long)imin(x0 + k, a.w0 - 1) * a.sx;
#pragma unroll
      for (int c = 0; c < 3; ++c) px[1 + k][c] = (float)q[c * a.sc];
    }
  }
  if constexpr (LEFT) {
    const uint8_t* q = row + (long long)imax(x0 - 1, 0) * a.sx;
#pragma unroll
    for (int c = 0; c < 3; ++c) px[0][c] = (float)q[c * a.sc];
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) px[0][c] = 0.0f;
  }
}

// the 8 Y' bytes of one luma row
__device__ __forceinline__ void store_luma(const YuvOutArgs& a, uint8_t* d, int x0, bool whole, const float (&px)[9][3]) {
  uint32_t b[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) b[k] = to_byte(a.y_off + a.s_y * lum(a, px[1 + k][0], px[1 + k][1], px[1 + k][2]));
  if (whole && aligned4(d)) {
    u32x2u w;
    w[0] = pack4(b[0], b[1], b[2], b[3]);
    w[1] = pack4(b[4], b[5], b[6], b[7]);
    *reinterpret_cast<u32x2u*>(d) = w;
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (x0 + k < a.w0) d[k] = (uint8_t)b[k];
  }
}

}  // namespace

template <bool CENTER>
__global__ __launch_bounds__(YO_BLOCK) void frames_rgb8_to_yuv420_kernel(const YuvOutArgs a) {
  const int lx = threadIdx.x % YO_LANES_X, ly = threadIdx.x / YO_LANES_X;
  const int i0 = (blockIdx.x * YO_LANES_X + lx) * 4;                 // the lane's first chroma column
  const int j = blockIdx.y * YO_LANES_Y + ly;                        // its chroma row
  const int x0 = 2 * i0;
  if (x0 >= a.w0 || j >= a.ch) return;
  const int t = blockIdx.z;
  const int r0 = 2 * j, r1 = imin(r0 + 1, a.h0 - 1);
  const bool whole = x0 + 7 < a.w0;
  const uint8_t* frame = a.src + (long long)t * a.st;

  float p0[9][3], p1[9][3];
  load_row<!CENTER>(a, frame + (long long)r0 * a.sy, x0, whole, p0);
  load_row<!CENTER>(a, frame + (long long)r1 * a.sy, x0, whole, p1);

  uint8_t* dy = a.y + (long long)t * a.yst + (long long)r0 * a.ysy + x0;
  store_luma(a, dy, x0, whole, p0);
  if (r0 + 1 < a.h0) store_luma(a, dy + a.ysy, x0, whole, p1);

  // chroma sample i0 + i: the bytes filtered first (eighths on bytes: exact), then the matrix
  uint32_t bu[4], bv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int k = 1 + 2 * i;                                          // px index of luma column 2 (i0 + i)
    float m[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if constexpr (CENTER) {
        m[c] = ((p0[k][c] + p0[k + 1][c]) + (p1[k][c] + p1[k + 1][c])) * 0.25f;
      } else {
        const float t0 = (p0[k - 1][c] + 2.0f * p0[k][c]) + p0[k + 1][c], t1 = (p1[k - 1][c] + 2.0f * p1[k][c]) + p1[k + 1][c];
        m[c] = (t0 + t1) * 0.125f;
      }
    }
    const float L = lum(a, m[0], m[1], m[2]);
    bu[i] = to_byte(128.0f + a.cu * (m[2] - L));
    bv[i] = to_byte(128.0f + a.cv * (m[0] - L));
  }
  const long long off = (long long)t * a.cst + (long long)j * a.csy + (long long)i0 * a.csx;
  uint8_t *du = a.u + off, *dv = a.v + off;
  const bool cwhole = i0 + 3 < a.cw;
  if (cwhole && a.csx == 1 && aligned4(du) && aligned4(dv)) {
    *reinterpret_cast<uint32_t*>(du) = pack4(bu[0], bu[1], bu[2], bu[3]);
    *reinterpret_cast<uint32_t*>(dv) = pack4(bv[0], bv[1], bv[2], bv[3]);
  } else if (cwhole && a.csx == 2 && dv == du + 1 && aligned4(du)) {  // NV12: (u, v) pairs
    u32x2u w;
    w[0] = pack4(bu[0], bv[0], bu[1], bv[1]);
    w[1] = pack4(bu[2], bv[2], bu[3], bv[3]);
    *reinterpret_cast<u32x2u*>(du) = w;
  } else if (cwhole && a.csx == 2 && du == dv + 1 && aligned4(dv)) {  // NV21: (v, u) pairs
    u32x2u w;
    w[0] = pack4(bv[0], bu[0], bv[1], bu[1]);
    w[1] = pack4(bv[2], bu[2], bv[3], bu[3]);
    *reinterpret_cast<u32x2u*>(dv) = w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i0 + i < a.cw) {
        du[(long long)i * a.csx] = (uint8_t)bu[i];
        dv[(long long)i * a.csx] = (uint8_t)bv[i];
      }
  }
}

void yuv_out_tile(int* rows, int* cols) {
  *rows = YO_ROWS;
  *cols = YO_COLS;
}

int frames_rgb8_to_yuv420_launch(const uint8_t* frames, int T, int h0, int w0, long long st, long long sy, long long sx, long long sc, uint8_t* y,
                                 long long yst, long long ysy, uint8_t* u, uint8_t* v, long long cst, long long csy, long long csx,
                                 const float* coef, int siting, hipStream_t s) {
  YuvOutArgs a;
  a.src = frames; a.y = y; a.u = u; a.v = v;
  a.st = st; a.sy = sy; a.sx = sx; a.sc = sc;
  a.yst = yst; a.ysy = ysy; a.cst = cst; a.csy = csy; a.csx = csx;
  a.kr = coef[0]; a.kg = coef[1]; a.kb = coef[2]; a.y_off = coef[3]; a.s_y = coef[4]; a.cu = coef[5]; a.cv = coef[6];
  a.h0 = h0; a.w0 = w0; a.ch = (h0 + 1) / 2; a.cw = (w0 + 1) / 2;
  const dim3 grid(cdiv(w0, YO_COLS), cdiv(a.ch, YO_LANES_Y), T);
  if (siting == FGVC_YUV_SITING_CENTER) frames_rgb8_to_yuv420_kernel<true><<<grid, YO_BLOCK, 0, s>>>(a);
  else frames_rgb8_to_yuv420_kernel<false><<<grid, YO_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_frames_rgb8_to_yuv420");
  return FGVC_OK;
}

}  // namespace fgvc
