// Point tracks in both time directions by chaining the dense flow.
//   * fgvc_flow_chain_f32: the reference's TAP-Vid flow-chaining baseline (RAFT.forward_test, raft.py:247-289, on bilinear_sample2d,
//     samp.py:5-99) for a whole clip, every point and both directions in one launch.  A point has two lanes: blockIdx.y = 0 writes the query
//     frame and walks forward through flow_fw, blockIdx.y = 1 walks backward through flow_bw.  Both loop over the frames in step, so at
//     every frame a wave stores consecutive points: one 8-byte position and one visibility byte per lane.
// f32 arithmetic without contraction, in the reference's order: the result equals its float32 run bit for bit.
// Plain vector loads and stores; no atomics, no LDS, no workspace.
#include <math.h>

#include "common.hpp"

namespace fgvc {

constexpr int CHAIN_BLOCK = 128;
constexpr float CHAIN_LIMIT = 8388608.0f;                        // 2^23: below it floorf(x) and floorf(x) + 1 are exact ints

// a position that is never turned into an index: non-finite, or 2^23 and beyond (a NaN fails both comparisons)
__device__ __forceinline__ bool chain_bad(float x, float y) { return !(fabsf(x) < CHAIN_LIMIT && fabsf(y) < CHAIN_LIMIT); }

__device__ __forceinline__ bool chain_inside(float x, float y, int h, int w) { return x >= 0.f && y >= 0.f && x < (float)w && y < (float)h; }

// bilinear_sample2d of the two planes of one flow field at (x, y), |x|, |y| < 2^23: taps at the clamped floor and floor + 1, the weights
// from the unclamped ones, ((w00 i00 + w01 i01) + w10 i10) + w11 i11 with every product rounded.  `ok` (may be null): the hop is good when
// (x, y) is inside the frame and the mask is set at its nearest pixel.
__device__ __forceinline__ void chain_sample(const float* __restrict__ f, const uint8_t* __restrict__ ok, int h, int w, float x, float y,
                                             float& dx, float& dy, bool& good) {
#pragma clang fp contract(off)
  const float x0f = floorf(x), y0f = floorf(y), x1f = x0f + 1.0f, y1f = y0f + 1.0f;
  const int x0 = (int)x0f, y0 = (int)y0f;
  const int xa = imin(imax(x0, 0), w - 1), xb = imin(imax(x0 + 1, 0), w - 1);
  const int ya = imin(imax(y0, 0), h - 1), yb = imin(imax(y0 + 1, 0), h - 1);
  const size_t plane = (size_t)h * w;
  const float* ra = f + (size_t)ya * w;
  const float* rb = f + (size_t)yb * w;
  // eight independent loads (and the mask byte), one wait
  const float u00 = ra[xa], u01 = ra[xb], u10 = rb[xa], u11 = rb[xb];
  const float v00 = ra[plane + xa], v01 = ra[plane + xb], v10 = rb[plane + xa], v11 = rb[plane + xb];
  if (ok) {
    const int xn = imin(imax((int)floorf(x + 0.5f), 0), w - 1), yn = imin(imax((int)floorf(y + 0.5f), 0), h - 1);
    good = chain_inside(x, y, h, w) && ok[(size_t)yn * w + xn] != 0;
  } else {
    good = true;
  }
  const float w00 = (x1f - x) * (y1f - y), w01 = (x - x0f) * (y1f - y), w10 = (x1f - x) * (y - y0f), w11 = (x - x0f) * (y - y0f);
  dx = ((w00 * u00 + w01 * u01) + w10 * u10) + w11 * u11;
  dy = ((w00 * v00 + w01 * v01) + w10 * v10) + w11 * v11;
}

// flow_fw / flow_bw [T-1][2][h][w], ok_fw / ok_bw [T-1][h][w] or null, query [P][3] = (t, x, y); traj [T][P] (x, y), vis [T][P].
// A query time that is no integer of [0, T) is never turned into an index either: every frame of that point is NaN and invisible.
__global__ __launch_bounds__(CHAIN_BLOCK) void flow_chain_kernel(const float* __restrict__ fw, const float* __restrict__ bw,
                                                                  const uint8_t* __restrict__ okfw, const uint8_t* __restrict__ okbw,
                                                                  const float* __restrict__ query, int T, int P, int h, int w, int sticky,
                                                                  fgvc_f32x2* __restrict__ traj, uint8_t* __restrict__ vis) {
#pragma clang fp contract(off)
  const int p = blockIdx.x * CHAIN_BLOCK + threadIdx.x;
  if (p >= P) return;
  const bool backward = blockIdx.y != 0;
  const float qt = query[3 * (size_t)p], qx = query[3 * (size_t)p + 1], qy = query[3 * (size_t)p + 2];
  const bool timed = qt >= 0.f && qt < (float)T && floorf(qt) == qt;
  const int tq = timed ? (int)qt : 0;
  const size_t plane = (size_t)h * w;
  const fgvc_f32x2 nan2 = {NAN, NAN};
  float x = qx, y = qy;
  bool dead = !timed || chain_bad(x, y), all_good = true;
  // both loops run over the frames in step in every lane (a lane outside its own range idles): a wave's stores go to one frame
  if (!backward) {
    for (int t = 0; t < T; ++t) {
      if (t < tq) continue;
      fgvc_f32x2 out = {qx, qy};
      if (t > tq) {
        if (!dead) {
          float dx, dy;
          bool good;
          chain_sample(fw + (size_t)(t - 1) * 2 * plane, okfw ? okfw + (size_t)(t - 1) * plane : nullptr, h, w, x, y, dx, dy, good);
          all_good = all_good && good;
          x = x + dx;
          y = y + dy;
          dead = chain_bad(x, y);
        }
        out = dead ? nan2 : fgvc_f32x2{x, y};
      } else if (!timed) {
        out = nan2;
      }
      const size_t o = (size_t)t * P + p;
      traj[o] = out;
      vis[o] = (uint8_t)((t == tq ? timed : !dead) && chain_inside(out.x, out.y, h, w) && (!sticky || all_good));
    }
  } else {
    for (int t = T - 2; t >= 0; --t) {
      if (t >= tq) continue;
      if (!dead) {
        float dx, dy;
        bool good;
        chain_sample(bw + (size_t)t * 2 * plane, okbw ? okbw + (size_t)t * plane : nullptr, h, w, x, y, dx, dy, good);
        all_good = all_good && good;
        x = x + dx;
        y = y + dy;
        dead = chain_bad(x, y);
      }
      const size_t o = (size_t)t * P + p;
      traj[o] = dead ? nan2 : fgvc_f32x2{x, y};
      vis[o] = (uint8_t)(!dead && chain_inside(x, y, h, w) && (!sticky || all_good));
    }
  }
}

int flow_chain_launch(const float* fw, const float* bw, const uint8_t* okfw, const uint8_t* okbw, const float* query, int T, int P, int h,
                      int w, int sticky, float* traj, uint8_t* vis, hipStream_t s) {
  const dim3 grid(cdiv(P, CHAIN_BLOCK), 2);
  flow_chain_kernel<<<grid, CHAIN_BLOCK, 0, s>>>(fw, bw, okfw, okbw, query, T, P, h, w, sticky, reinterpret_cast<fgvc_f32x2*>(traj), vis);
  FGVC_CHECK_LAUNCH("fgvc_flow_chain_f32");
  return FGVC_OK;
}

}  // namespace fgvc
