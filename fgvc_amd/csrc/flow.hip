// Dense optical flow between frames and its forward-backward check.
//   * fgvc_flow_from_lists_f32: every row's single-slot window lists (run_local_affinity) -> a full-resolution flow field and its validity
//     mask in one launch.  A workgroup owns a FLOW_TW x FLOW_TH tile of output pixels: it reduces the lists of the feature cells the tile
//     touches to displacements in LDS once (a cell's k entries read as 8-byte vectors where k is even), then every lane interpolates its
//     pixels from LDS and a wave stores 64 consecutive floats of one output row.
//   * fgvc_flow_consistency_f32: both directions of the reference's occlusion_estimation (occlusion_estimation.py:95-177) in one launch.
//   * fgvc_warp_f32: the reference's Warp.forward (warp.py:55-82), on the device function the consistency kernel samples with.
// Plain vector loads and stores; no atomics, no workspace.
#include <math.h>

#include "common.hpp"

namespace fgvc {

constexpr int FLOW_TW = 64, FLOW_TH = 16;                        // the output tile of one workgroup (256 lanes: 64 columns x 4 rows, four times)
constexpr int FLOW_CELLS = (FLOW_TW + 1) * (FLOW_TH + 1);        // scale = 1: a tile touches TW + 1 by TH + 1 cells, fewer at any larger scale

// One feature cell's displacement from its k list entries: S = sum w_r and C = sum w_r (kx, ky) scale over the non-empty taps inside the
// image -- topk_coord_rows_kernel's selection and order (cycle.hip) -- then C / S - q scale (renorm) or C - q scale (get_coord's own sum,
// vanilla_tracker.py:445-488).  S == 0: no displacement, invalid.
template <int VEC>
__device__ __forceinline__ void cell_displacement(const int32_t* __restrict__ ip, const float* __restrict__ wp, int topk, int qx, int qy,
                                                  int H, int W, int R, int scale, int renorm, float& dx, float& dy, int& ok) {
  const int L = 2 * R + 1, LL = L * L;
  float ax = 0.f, ay = 0.f, s = 0.f;
  auto tap = [&](int id, float wv) {
    if (id < 0) return;
    const int t = id % LL;
    const int ky = qy + t / L - R, kx = qx + t % L - R;
    if (ky < 0 || ky >= H || kx < 0 || kx >= W) return;
    s += wv;
    ax = fmaf(wv, (float)(kx * scale), ax);
    ay = fmaf(wv, (float)(ky * scale), ay);
  };
  if (VEC == 2) {
    const int2* ip2 = reinterpret_cast<const int2*>(ip);
    const fgvc_f32x2* wp2 = reinterpret_cast<const fgvc_f32x2*>(wp);
    for (int r = 0; r < topk / 2; ++r) {
      const int2 id = ip2[r];
      const fgvc_f32x2 wv = wp2[r];
      tap(id.x, wv.x);
      tap(id.y, wv.y);
    }
  } else {
    for (int r = 0; r < topk; ++r) tap(ip[r], wp[r]);
  }
  ok = s != 0.f;
  if (!ok) {
    dx = dy = 0.f;
    return;
  }
  const float px = (float)(qx * scale), py = (float)(qy * scale);
  dx = (renorm ? ax / s : ax) - px;
  dy = (renorm ? ay / s : ay) - py;
}

template <int VEC>
__global__ __launch_bounds__(256) void flow_from_lists_kernel(const int32_t* __restrict__ idx, const float* __restrict__ weight, int H, int W,
                                                               int R, int topk, int scale, int renorm, int h, int w, int pad_left,
                                                               int pad_top, float* __restrict__ flow, uint8_t* __restrict__ valid) {
  __shared__ float sdx[FLOW_CELLS], sdy[FLOW_CELLS];
  __shared__ int sok[FLOW_CELLS];
  const size_t row = blockIdx.z;
  const int HW = H * W;
  const int x0 = blockIdx.x * FLOW_TW, y0 = blockIdx.y * FLOW_TH;                     // the tile's first output pixel
  // the cells the tile's padded pixels (x + pad_left, y + pad_top) touch: floor(X / scale) and the one after it, both held inside the grid
  const int cx_first = imin((x0 + pad_left) / scale, W - 1), cx_last = imin((x0 + FLOW_TW - 1 + pad_left) / scale + 1, W - 1);
  const int cy_first = imin((y0 + pad_top) / scale, H - 1), cy_last = imin((y0 + FLOW_TH - 1 + pad_top) / scale + 1, H - 1);
  const int ncx = cx_last - cx_first + 1, ncy = cy_last - cy_first + 1;                // <= TW + 1, TH + 1
  for (int c = threadIdx.x; c < ncx * ncy; c += 256) {
    const int qy = cy_first + c / ncx, qx = cx_first + c % ncx;
    const size_t at = (row * HW + (size_t)qy * W + qx) * topk;
    float dx, dy;
    int ok;
    cell_displacement<VEC>(idx + at, weight + at, topk, qx, qy, H, W, R, scale, renorm, dx, dy, ok);
    sdx[c] = dx;
    sdy[c] = dy;
    sok[c] = ok;
  }
  __syncthreads();
  const int x = x0 + (threadIdx.x & (FLOW_TW - 1));
  if (x >= w) return;
  const int X = x + pad_left;
  const int cx0 = imin(X / scale, W - 1), cx1 = imin(cx0 + 1, W - 1);                  // the upper neighbour is clamped to the last cell
  const float fx = (float)(X - cx0 * scale) / (float)scale;
  const int lx0 = cx0 - cx_first, lx1 = cx1 - cx_first;
  const size_t plane = (size_t)h * w;
  float* fo = flow + row * 2 * plane;
  uint8_t* vo = valid + row * plane;
#pragma unroll
  for (int j = 0; j < FLOW_TH / 4; ++j) {
    const int y = y0 + (threadIdx.x >> 6) + 4 * j;
    if (y >= h) break;
    const int Y = y + pad_top;
    const int cy0 = imin(Y / scale, H - 1), cy1 = imin(cy0 + 1, H - 1);
    const float fy = (float)(Y - cy0 * scale) / (float)scale;
    const int a = (cy0 - cy_first) * ncx, b = (cy1 - cy_first) * ncx;
    const int i00 = a + lx0, i01 = a + lx1, i10 = b + lx0, i11 = b + lx1;
    const float tx = sdx[i00] + fx * (sdx[i01] - sdx[i00]), bx = sdx[i10] + fx * (sdx[i11] - sdx[i10]);
    const float ty = sdy[i00] + fx * (sdy[i01] - sdy[i00]), by = sdy[i10] + fx * (sdy[i11] - sdy[i10]);
    const size_t o = (size_t)y * w + x;
    fo[o] = tx + fy * (bx - tx);
    fo[plane + o] = ty + fy * (by - ty);
    vo[o] = (uint8_t)(sok[i00] & sok[i01] & sok[i10] & sok[i11]);
  }
}

// What F.grid_sample(src, coords_grid_warp(flow), 'bilinear', 'zeros', align_corners) reads at output pixel (x, y) whose flow is (u, v): the
// four taps, their weights and which of them lie inside the (H, W) plane.  The reference's arithmetic, step by step in f32 without
// contraction:
//   warp.py:22-24          grid = (x + u) * 2. / max(W - 1, 1) - 1.   -- normalised by W - 1 whatever align_corners is
//   grid_sample            align_corners: ((g + 1) / 2) (W - 1);  otherwise ((g + 1) W - 1) / 2
//   weights                (x1 - ix)(y1 - iy), (ix - x0)(y1 - iy), (x1 - ix)(iy - y0), (ix - x0)(iy - y0); a tap outside the plane adds 0.
// The bounds are tested on the floats, so a NaN or a huge coordinate reads nothing.
struct WarpTaps {
  float w[4];
  int at[4];       // y * W + x of the tap, or -1
};

__device__ __forceinline__ WarpTaps warp_taps(int x, int y, float u, float v, int H, int W, int align_corners) {
#pragma clang fp contract(off)
  const float dw = (float)imax(W - 1, 1), dh = (float)imax(H - 1, 1);
  const float gx = ((float)x + u) * 2.0f / dw - 1.0f, gy = ((float)y + v) * 2.0f / dh - 1.0f;
  const float ix = align_corners ? ((gx + 1.0f) / 2.0f) * (float)(W - 1) : ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;
  const float iy = align_corners ? ((gy + 1.0f) / 2.0f) * (float)(H - 1) : ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
  const float xa = floorf(ix), ya = floorf(iy), xb = xa + 1.0f, yb = ya + 1.0f;
  const bool inxa = xa >= 0.f && xa <= (float)(W - 1), inxb = xb >= 0.f && xb <= (float)(W - 1);
  const bool inya = ya >= 0.f && ya <= (float)(H - 1), inyb = yb >= 0.f && yb <= (float)(H - 1);
  WarpTaps t;
  t.w[0] = (xb - ix) * (yb - iy);
  t.w[1] = (ix - xa) * (yb - iy);
  t.w[2] = (xb - ix) * (iy - ya);
  t.w[3] = (ix - xa) * (iy - ya);
  t.at[0] = (inxa && inya) ? (int)ya * W + (int)xa : -1;
  t.at[1] = (inxb && inya) ? (int)ya * W + (int)xb : -1;
  t.at[2] = (inxa && inyb) ? (int)yb * W + (int)xa : -1;
  t.at[3] = (inxb && inyb) ? (int)yb * W + (int)xb : -1;
  return t;
}

// grid_sample of one plane: the in-plane taps summed in the order nw, ne, sw, se
__device__ __forceinline__ float warp_sample(const float* __restrict__ src, const WarpTaps& t) {
#pragma clang fp contract(off)
  float v[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = t.at[i] >= 0 ? src[t.at[i]] : 0.f;      // four independent loads, one wait
  float o = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (t.at[i] >= 0) o += v[i] * t.w[i];
  return o;
}

// warp.py:73-81: the same sampling of a plane of ones, then (mask > 0.9999); 1 without use_mask
__device__ __forceinline__ float warp_mask(const WarpTaps& t, int use_mask) {
#pragma clang fp contract(off)
  if (!use_mask) return 1.0f;
  float o = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (t.at[i] >= 0) o += t.w[i];
  return o > 0.9999f ? 1.0f : 0.f;
}

// One direction of the check at one pixel: a = the flow at the pixel, `other` = the opposite flow's two planes.
//   occlusion_estimation.py:108, :135   warp = Warp(): the default align_corners=False and use_mask=True; `warp_cfg` (whose default asks
//                                       for align_corners=True) is never read
//   :112-113, :139-140                  sq_diff = sum_c (a_c + warped_c)^2
//   :114-115                            sum_sq = sum_c (a_c * 2 + warped_c^2)   -- a product by two, not a square
//   :117-118                            consistency: sq_diff < sum_sq * 0.01 + 0.5
//   :142                                fb_abs: sq_diff ** 0.5 < diff
__device__ __forceinline__ float fb_check(const float* __restrict__ other, size_t plane, int x, int y, float ax, float ay, int H, int W,
                                          int mode, float diff) {
#pragma clang fp contract(off)
  const WarpTaps t = warp_taps(x, y, ax, ay, H, W, 0);
  const float m = warp_mask(t, 1);
  const float wx = warp_sample(other, t) * m, wy = warp_sample(other + plane, t) * m;
  const float sx = ax + wx, sy = ay + wy;
  const float sq_diff = sx * sx + sy * sy;
  if (mode == FGVC_FLOW_FB_ABS) return sqrtf(sq_diff) < diff ? 1.0f : 0.f;
  const float sum_sq = (ax * 2.0f + wx * wx) + (ay * 2.0f + wy * wy);
  return sq_diff < sum_sq * 0.01f + 0.5f ? 1.0f : 0.f;
}

__global__ __launch_bounds__(256) void flow_consistency_kernel(const float* __restrict__ fw, const float* __restrict__ bw, int H, int W,
                                                                int mode, float diff, float* __restrict__ occ_fw,
                                                                float* __restrict__ occ_bw) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = (size_t)H * W;
  if ((size_t)p >= plane) return;
  const size_t n = blockIdx.y;
  const int y = p / W, x = p - y * W;
  const float* f = fw + n * 2 * plane;
  const float* b = bw + n * 2 * plane;
  const float fx = f[p], fy = f[plane + p], bx = b[p], by = b[plane + p];
  occ_fw[n * plane + p] = fb_check(b, plane, x, y, fx, fy, H, W, mode, diff);
  occ_bw[n * plane + p] = fb_check(f, plane, x, y, bx, by, H, W, mode, diff);
}

__global__ __launch_bounds__(256) void warp_kernel(const float* __restrict__ feat, const float* __restrict__ flow, int C, int H, int W,
                                                    int align_corners, int use_mask, float* __restrict__ out) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * 256 + threadIdx.x;
  const size_t plane = (size_t)H * W;
  if ((size_t)p >= plane) return;
  const size_t n = blockIdx.y;
  const int y = p / W, x = p - y * W;
  const float* fl = flow + n * 2 * plane;
  const WarpTaps t = warp_taps(x, y, fl[p], fl[plane + p], H, W, align_corners);
  const float m = warp_mask(t, use_mask);
  for (int c = 0; c < C; ++c) {
    const size_t o = (n * C + c) * plane;
    out[o + p] = warp_sample(feat + o, t) * m;
  }
}

int flow_from_lists_launch(const int32_t* idx, const float* weight, int rows, int H, int W, int R, int topk, int scale, int renorm, int h,
                           int w, int pad_left, int pad_top, float* flow, uint8_t* valid, hipStream_t s) {
  const dim3 grid(cdiv(w, FLOW_TW), cdiv(h, FLOW_TH), rows);
  const bool vec = topk % 2 == 0 && ((reinterpret_cast<uintptr_t>(idx) | reinterpret_cast<uintptr_t>(weight)) & 7u) == 0;
  if (vec)
    flow_from_lists_kernel<2><<<grid, 256, 0, s>>>(idx, weight, H, W, R, topk, scale, renorm, h, w, pad_left, pad_top, flow, valid);
  else
    flow_from_lists_kernel<1><<<grid, 256, 0, s>>>(idx, weight, H, W, R, topk, scale, renorm, h, w, pad_left, pad_top, flow, valid);
  FGVC_CHECK_LAUNCH("fgvc_flow_from_lists_f32");
  return FGVC_OK;
}

int flow_consistency_launch(const float* fw, const float* bw, int n, int h, int w, int mode, float diff, float* occ_fw, float* occ_bw,
                            hipStream_t s) {
  const dim3 grid(cdiv(h * w, 256), n);
  flow_consistency_kernel<<<grid, 256, 0, s>>>(fw, bw, h, w, mode, diff, occ_fw, occ_bw);
  FGVC_CHECK_LAUNCH("fgvc_flow_consistency_f32");
  return FGVC_OK;
}

int warp_launch(const float* feat, const float* flow, int N, int C, int H, int W, int align_corners, int use_mask, float* out, hipStream_t s) {
  const dim3 grid(cdiv(H * W, 256), N);
  warp_kernel<<<grid, 256, 0, s>>>(feat, flow, C, H, W, align_corners, use_mask, out);
  FGVC_CHECK_LAUNCH("fgvc_warp_f32");
  return FGVC_OK;
}

}  // namespace fgvc
