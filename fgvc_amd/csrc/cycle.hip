// Forward-backward cycle check of predicted point tracks.
//   * fgvc_topk_coord_rows_f32: topk_coord_kernel (local.hip, A7 get_coord, vanilla_tracker.py:445-488) for every row of a planned clip in
//     one launch: row r's single-slot window lists -> its coordinate field, (x, y) interleaved so that one bilinear tap is one 8-byte load.
//   * fgvc_cycle_chase_f32: one thread per (frame, point) walks its predicted position back to the query frame through the chain of
//     fields, one bilinear sample per hop (HRVanillaTracker.forward_test_forward's step, vanilla_tracker.py:639: corr_lookup.py:31-65
//     bilinear_sample with align_corners=True and zero padding), and writes where it lands and how far that is from the query point.
// Plain vector loads and stores; no atomics, no LDS, no workspace.
#include <math.h>

#include "common.hpp"

namespace fgvc {

__global__ __launch_bounds__(256) void topk_coord_rows_kernel(const int32_t* __restrict__ idx, const float* __restrict__ weight, int H,
                                                               int W, int R, int topk, int scale, fgvc_f32x2* __restrict__ out) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  const int HW = H * W;
  if (q >= HW) return;
  const size_t row = blockIdx.y;
  const int L = 2 * R + 1, qy = q / W, qx = q - qy * W;
  const int32_t* ip = idx + (row * HW + q) * topk;
  const float* wp = weight + (row * HW + q) * topk;
  float ax = 0.f, ay = 0.f;
  for (int r = 0; r < topk; ++r) {              // the same sum in the same order as topk_coord_kernel: a row equals its output bit for bit
    const int id = ip[r];
    if (id < 0) continue;
    const int tap = id % (L * L);
    const int ky = qy + tap / L - R, kx = qx + tap % L - R;
    if (ky < 0 || ky >= H || kx < 0 || kx >= W) continue;
    const float wv = wp[r];
    ax = fmaf(wv, (float)(kx * scale), ax);
    ay = fmaf(wv, (float)(ky * scale), ay);
  }
  out[row * HW + q] = fgvc_f32x2{ax, ay};
}

// F.grid_sample(field, grid, 'bilinear', 'zeros', align_corners=True) at the pixel coordinate (px, py) of an (H, W) field of (x, y) pairs,
// through the normalised grid the reference builds first (corr_lookup.py:61-63): g = p * 2 / (size - 1) - 1, then ((g + 1) / 2) * (size - 1).
// A tap outside the field contributes 0; the bounds are tested on the floats, so a NaN or a huge coordinate reads nothing.
__device__ __forceinline__ fgvc_f32x2 grid_sample_xy(const fgvc_f32x2* __restrict__ f, float px, float py, int H, int W) {
  const float dw = (float)max(W - 1, 1), dh = (float)max(H - 1, 1);
  const float gx = px * 2.0f / dw - 1.0f, gy = py * 2.0f / dh - 1.0f;
  const float ix = ((gx + 1.0f) / 2.0f) * (float)(W - 1), iy = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
  const float x0 = floorf(ix), y0 = floorf(iy), x1 = x0 + 1.0f, y1 = y0 + 1.0f;
  const float wnw = (x1 - ix) * (y1 - iy), wne = (ix - x0) * (y1 - iy), wsw = (x1 - ix) * (iy - y0), wse = (ix - x0) * (iy - y0);
  const bool inx0 = x0 >= 0.f && x0 <= (float)(W - 1), inx1 = x1 >= 0.f && x1 <= (float)(W - 1);
  const bool iny0 = y0 >= 0.f && y0 <= (float)(H - 1), iny1 = y1 >= 0.f && y1 <= (float)(H - 1);
  const fgvc_f32x2 z = {0.f, 0.f};
  // the four loads are independent: issued together, one wait
  const fgvc_f32x2 nw = (inx0 && iny0) ? f[(int)y0 * W + (int)x0] : z;
  const fgvc_f32x2 ne = (inx1 && iny0) ? f[(int)y0 * W + (int)x1] : z;
  const fgvc_f32x2 sw = (inx0 && iny1) ? f[(int)y1 * W + (int)x0] : z;
  const fgvc_f32x2 se = (inx1 && iny1) ? f[(int)y1 * W + (int)x1] : z;
  float ox = 0.f, oy = 0.f;
  if (inx0 && iny0) { ox += nw.x * wnw; oy += nw.y * wnw; }
  if (inx1 && iny0) { ox += ne.x * wne; oy += ne.y * wne; }
  if (inx0 && iny1) { ox += sw.x * wsw; oy += sw.y * wsw; }
  if (inx1 && iny1) { ox += se.x * wse; oy += se.y * wse; }
  return fgvc_f32x2{ox, oy};
}

// fields [n][H*W] (x, y): fields[j] takes a position in frame s + 1 + j to frame s + j.  traj [n][P] = the predicted positions of frames
// s + 1 .. s + n, start [P] = the query points (frame s).  Thread (i, p): i + 1 dependent hops.  A non-finite position at any hop, or the
// (-1, -1) the read-out gives for an all-zero map, ends as back = NaN, err = +inf.
__global__ __launch_bounds__(256) void cycle_chase_kernel(const fgvc_f32x2* __restrict__ fields, const fgvc_f32x2* __restrict__ traj,
                                                           const fgvc_f32x2* __restrict__ start, int n, int P, int H, int W, float scale,
                                                           fgvc_f32x2* __restrict__ back, float* __restrict__ err) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n * P) return;
  const int i = t / P, p = t - i * P;
  const size_t HW = (size_t)H * W;
  fgvc_f32x2 y = traj[t];
  bool ok = isfinite(y.x) && isfinite(y.y) && !(y.x == -1.0f && y.y == -1.0f);
  for (int g = i; g >= 0 && ok; --g) {
    y = grid_sample_xy(fields + (size_t)g * HW, y.x / scale, y.y / scale, H, W);
    ok = isfinite(y.x) && isfinite(y.y);
  }
  const fgvc_f32x2 s0 = start[p];
  const float dx = y.x - s0.x, dy = y.y - s0.y;
  const float e = sqrtf(dx * dx + dy * dy);
  const bool fin = ok && isfinite(e);
  back[t] = fin ? y : fgvc_f32x2{NAN, NAN};
  err[t] = fin ? e : INFINITY;
}

int topk_coord_rows_launch(const int32_t* idx, const float* weight, int rows, int H, int W, int R, int topk, int scale, float* out,
                           hipStream_t s) {
  const dim3 grid(cdiv(H * W, 256), rows);
  topk_coord_rows_kernel<<<grid, 256, 0, s>>>(idx, weight, H, W, R, topk, scale, reinterpret_cast<fgvc_f32x2*>(out));
  FGVC_CHECK_LAUNCH("fgvc_topk_coord_rows_f32");
  return FGVC_OK;
}

int cycle_chase_launch(const float* fields, const float* traj, const float* start, int n, int P, int H, int W, int scale, float* back,
                       float* err, hipStream_t s) {
  cycle_chase_kernel<<<cdiv(n * P, 256), 256, 0, s>>>(reinterpret_cast<const fgvc_f32x2*>(fields), reinterpret_cast<const fgvc_f32x2*>(traj),
                                                      reinterpret_cast<const fgvc_f32x2*>(start), n, P, H, W, (float)scale,
                                                      reinterpret_cast<fgvc_f32x2*>(back), err);
  FGVC_CHECK_LAUNCH("fgvc_cycle_chase_f32");
  return FGVC_OK;
}

}  // namespace fgvc
