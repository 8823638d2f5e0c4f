// The renderer's shared pieces (DESIGN.md sections 16, 21 and 23): the tile, the 12-byte load and store, and the body of the one-launch
// kernel -- load, overlay, [a stage of the including file], points, store.  render.hip instantiates it with no stage
// (fgvc_render_frames_u8), trails.hip with the trail stage between the overlay and the points (fgvc_render_trails_u8), pose.hip with the
// heat maps and limbs there (fgvc_render_pose_u8).  At the end, the host side the three launchers share: the fill of RenderArgs from
// render_host.hpp's RenderCall and the launch loop over the frames.
//   * a workgroup owns RN_ROWS rows x RN_COLS columns of one frame; a lane owns 4 consecutive pixels (12 bytes) of RN_ROWS / 4 rows and keeps
//     them in registers from its one load to its one store, so `out` may be `frames`;
//   * the 12 bytes of a lane start at any address (W * 3 is generally no multiple of 4, and a cropped view starts anywhere): they are moved as
//     the aligned pieces that address allows -- dword dword dword | half dword dword half | byte half dword dword byte | byte dword dword half
//     byte -- never a byte of another lane, never an access across its own alignment.  A wave lies in one row, so the choice is uniform;
//   * overlay: integer only.  A lane whose four ids are 0 is done after one compare; the others read the ids around them for the contour;
//   * points: the workgroup scans the frame's P points RN_BLOCK at a time, and compacts IN INDEX ORDER (ballot + prefix count per wave, wave
//     totals through LDS) those that are visible, finite and whose (2 r + 2)^2 window meets the tile into an LDS list; every lane then walks
//     the list for its pixels, truncating to uint8 after every point as the reference's assignment into its uint8 image does.  As many
//     rounds as P needs: the list holds one round.  A tile no window meets costs the scan and nothing per pixel.
// The point arithmetic is float64 with contraction off: the gather form of the reference's scatter of patches into a padded image
// (flyingthingsplus/utils/visualize.py:126-154), each product left to right, the four terms summed left to right.
// No atomics, no second launch, no temporary image, no workspace.
#pragma once

#include <math.h>

#include "common.hpp"
#include "render_host.hpp"

#pragma clang fp contract(off)

namespace fgvc {

constexpr int RN_BLOCK = 256;
constexpr int RN_PX = 4;                          // pixels per lane and row
constexpr int RN_COLS = WAVE * RN_PX;             // 256 columns: one wave spans a tile's row
constexpr int RN_WAVES = RN_BLOCK / WAVE;
constexpr int RN_LANE_ROWS = 2;                   // rows per lane
constexpr int RN_ROWS = RN_WAVES * RN_LANE_ROWS;  // 8 rows per workgroup (exported as fgvc_render_tile(): the tests put points on the corners)

typedef unsigned __int128 u128;

struct RenderArgs {
  const uint8_t* frames;
  uint8_t* out;
  const uint8_t* ids;          // null: no overlay
  const uint8_t* palette;      // [256][3]
  const double* tracks;        // null: no points; (x, y) of point i on frame t at tracks[i * trk_sp + t * trk_st + {0, 1}]
  const uint8_t* visibles;     // null: all visible; visibles[i * vis_sp + t * vis_st] != 0
  const uint8_t* colors;       // [P][3]
  const double* icon;          // [2 r + 1][2 r + 1]
  long long f_st, f_sy, o_st, o_sy, i_st, i_sy, trk_sp, trk_st, vis_sp, vis_st;
  int t0, h, w, xtiles, alpha, contour, P, radius;
};

__device__ __forceinline__ u128 ld1(const uint8_t* q) { return (u128)*q; }
__device__ __forceinline__ u128 ld2(const uint8_t* q) { return (u128)*reinterpret_cast<const uint16_t*>(q); }
__device__ __forceinline__ u128 ld4(const uint8_t* q) { return (u128)*reinterpret_cast<const uint32_t*>(q); }
__device__ __forceinline__ void st1(uint8_t* q, u128 v) { *q = (uint8_t)v; }
__device__ __forceinline__ void st2(uint8_t* q, u128 v) { *reinterpret_cast<uint16_t*>(q) = (uint16_t)v; }
__device__ __forceinline__ void st4(uint8_t* q, u128 v) { *reinterpret_cast<uint32_t*>(q) = (uint32_t)v; }

// 12 bytes at any address, as the aligned pieces the address allows
__device__ __forceinline__ u128 load12(const uint8_t* q) {
  switch ((unsigned)reinterpret_cast<uintptr_t>(q) & 3u) {
    case 0: return ld4(q) | ld4(q + 4) << 32 | ld4(q + 8) << 64;
    case 2: return ld2(q) | ld4(q + 2) << 16 | ld4(q + 6) << 48 | ld2(q + 10) << 80;
    case 1: return ld1(q) | ld2(q + 1) << 8 | ld4(q + 3) << 24 | ld4(q + 7) << 56 | ld1(q + 11) << 88;
    default: return ld1(q) | ld4(q + 1) << 8 | ld4(q + 5) << 40 | ld2(q + 9) << 72 | ld1(q + 11) << 88;
  }
}

__device__ __forceinline__ void store12(uint8_t* q, u128 v) {
  switch ((unsigned)reinterpret_cast<uintptr_t>(q) & 3u) {
    case 0: st4(q, v); st4(q + 4, v >> 32); st4(q + 8, v >> 64); break;
    case 2: st2(q, v); st4(q + 2, v >> 16); st4(q + 6, v >> 48); st2(q + 10, v >> 80); break;
    case 1: st1(q, v); st2(q + 1, v >> 8); st4(q + 3, v >> 24); st4(q + 7, v >> 56); st1(q + 11, v >> 88); break;
    default: st1(q, v); st4(q + 1, v >> 8); st4(q + 5, v >> 40); st2(q + 9, v >> 72); st1(q + 11, v >> 88); break;
  }
}

// 4 id bytes at any address
__device__ __forceinline__ uint32_t load4(const uint8_t* q) {
  const unsigned m = (unsigned)reinterpret_cast<uintptr_t>(q) & 3u;
  if (m == 0) return *reinterpret_cast<const uint32_t*>(q);
  if (m == 2) return (uint32_t)*reinterpret_cast<const uint16_t*>(q) | (uint32_t)*reinterpret_cast<const uint16_t*>(q + 2) << 16;
  return (uint32_t)q[0] | (uint32_t)*reinterpret_cast<const uint16_t*>(q + 1) << 8 | (uint32_t)q[3] << 24;
}

// where a lane stands: handed to the stage
struct RenderLane {
  int t, tx0, ty0, tid, lane, wave;
};

// the stage of fgvc_render_frames_u8: none
struct NoStage {
  __device__ __forceinline__ void operator()(unsigned (&)[RN_LANE_ROWS][RN_PX * 3], const RenderLane&) const {}
};

template <class Stage>
__device__ __forceinline__ void render_body(const RenderArgs& a, const Stage& stage) {
  __shared__ uint8_t pal[256 * 3];
  __shared__ int l_x1[RN_BLOCK], l_y1[RN_BLOCK];
  __shared__ double l_wx0[RN_BLOCK], l_wx1[RN_BLOCK], l_wy0[RN_BLOCK], l_wy1[RN_BLOCK];
  __shared__ uint32_t l_col[RN_BLOCK];
  __shared__ int wave_n[RN_WAVES];

  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int t = a.t0 + blockIdx.y;
  const int tx0 = (blockIdx.x % a.xtiles) * RN_COLS, ty0 = (blockIdx.x / a.xtiles) * RN_ROWS;
  const int x0 = tx0 + lane * RN_PX;                                  // the lane's first column
  const int npx = imin(RN_PX, a.w - x0);                              // its columns inside the image (<= 0: none)

  if (a.ids) {
    for (int i = tid; i < 256 * 3; i += RN_BLOCK) pal[i] = a.palette[i];
    __syncthreads();
  }

  // ---- load, overlay ----
  unsigned v[RN_LANE_ROWS][RN_PX * 3];                                // 0 .. 255 per pixel and channel
#pragma unroll
  for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
    const int y = ty0 + wave * RN_LANE_ROWS + rr;
#pragma unroll
    for (int k = 0; k < RN_PX * 3; ++k) v[rr][k] = 0;
    if (y >= a.h || npx <= 0) continue;
    const uint8_t* q = a.frames + (long long)t * a.f_st + (long long)y * a.f_sy + (long long)x0 * 3;
    if (npx == RN_PX) {
      const u128 d = load12(q);
#pragma unroll
      for (int k = 0; k < RN_PX * 3; ++k) v[rr][k] = (unsigned)(d >> (8 * k)) & 255u;
    } else {
#pragma unroll
      for (int k = 0; k < RN_PX * 3; ++k)
        if (k < npx * 3) v[rr][k] = q[k];
    }
    if (!a.ids) continue;
    const uint8_t* m = a.ids + (long long)t * a.i_st + (long long)y * a.i_sy + x0;
    uint32_t own = 0;
    if (npx == RN_PX) {
      own = load4(m);
    } else {
#pragma unroll
      for (int j = 0; j < RN_PX; ++j)
        if (j < npx) own |= (uint32_t)m[j] << (8 * j);
    }
    if (own == 0) continue;                                           // background: the frame's pixels
    // the ids around the four: a missing neighbour counts as equal
    const bool up = y > 0, down = y + 1 < a.h;
    const uint32_t left = x0 > 0 ? m[-1] : (own & 255u);
#pragma unroll
    for (int j = 0; j < RN_PX; ++j) {
      if (j >= npx) continue;
      const uint32_t k = (own >> (8 * j)) & 255u;
      if (k == 0) continue;
      bool edge = false;
      if (a.contour) {
        const uint32_t l = j == 0 ? left : (own >> (8 * (j - 1))) & 255u;
        const uint32_t r = x0 + j + 1 < a.w ? (j + 1 < npx ? (own >> (8 * ((j + 1) & 3))) & 255u : m[j + 1]) : k;
        const uint32_t u = up ? m[j - a.i_sy] : k, d = down ? m[j + a.i_sy] : k;
        edge = l != k || r != k || u != k || d != k;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned p = pal[k * 3 + c];
        v[rr][3 * j + c] = edge ? p : (v[rr][3 * j + c] * (unsigned)(256 - a.alpha) + p * (unsigned)a.alpha + 128u) >> 8;
      }
    }
  }

  // ---- between the overlay and the points ----
  stage(v, RenderLane{t, tx0, ty0, tid, lane, wave});

  // ---- points ----
  if (a.tracks) {
    const int r = a.radius, D = 2 * r + 1;
    for (int base = 0; base < a.P; base += RN_BLOCK) {
      const int i = base + tid;
      bool take = false;
      int x1 = 0, y1 = 0;
      double x = 0.0, y = 0.0;
      if (i < a.P && (!a.visibles || a.visibles[(long long)i * a.vis_sp + (long long)t * a.vis_st] != 0)) {
        const double* p = a.tracks + (long long)i * a.trk_sp + (long long)t * a.trk_st;
        const double px = p[0], py = p[1];
        if (isfinite(px) && isfinite(py)) {
          x = fmin(fmax(px + 0.5, 0.0), (double)a.w);
          y = fmin(fmax(py + 0.5, 0.0), (double)a.h);
          x1 = (int)floor(x);
          y1 = (int)floor(y);
          // the window: columns x1 - r - 1 .. x1 + r, rows y1 - r - 1 .. y1 + r
          take = x1 + r >= tx0 && x1 - r - 1 < tx0 + RN_COLS && y1 + r >= ty0 && y1 - r - 1 < ty0 + RN_ROWS;
        }
      }
      const unsigned long long bal = __ballot(take);
      const int before = __popcll(bal & ((1ull << lane) - 1ull));
      if (lane == 0) wave_n[wave] = __popcll(bal);
      __syncthreads();
      int off = 0, n = 0;
#pragma unroll
      for (int wv = 0; wv < RN_WAVES; ++wv) {
        const int c = wave_n[wv];
        off += wv < wave ? c : 0;
        n += c;
      }
      if (take) {
        const int e = off + before;
        const int x2 = x1 + 1, y2 = y1 + 1;
        l_x1[e] = x1;
        l_y1[e] = y1;
        l_wx0[e] = (double)x2 - x;
        l_wx1[e] = x - (double)x1;
        l_wy0[e] = (double)y2 - y;
        l_wy1[e] = y - (double)y1;
        const uint8_t* c = a.colors + (long long)i * 3;
        l_col[e] = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
      }
      __syncthreads();
      for (int e = 0; e < n; ++e) {
        const int b0 = x0 + r + 1 - l_x1[e];                          // b of the lane's first pixel
        if (b0 + RN_PX - 1 < 0 || b0 > D) continue;
        const int a0 = ty0 + wave * RN_LANE_ROWS + r + 1 - l_y1[e];   // a of the lane's first row
        if (a0 + RN_LANE_ROWS - 1 < 0 || a0 > D) continue;
        const double wx0 = l_wx0[e], wx1 = l_wx1[e], wy0 = l_wy0[e], wy1 = l_wy1[e];
        const uint32_t col = l_col[e];
#pragma unroll
        for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
          const int aa = a0 + rr;
          if (aa < 0 || aa > D) continue;
#pragma unroll
          for (int j = 0; j < RN_PX; ++j) {
            const int bb = b0 + j;
            if (bb < 0 || bb > D) continue;
            const bool ra = aa < D, rb = bb < D, ra1 = aa >= 1, rb1 = bb >= 1;         // I(u, v) is zero outside 0 .. D - 1
            const double i00 = ra && rb ? a.icon[aa * D + bb] : 0.0;
            const double i10 = ra1 && rb ? a.icon[(aa - 1) * D + bb] : 0.0;
            const double i01 = ra && rb1 ? a.icon[aa * D + bb - 1] : 0.0;
            const double i11 = ra1 && rb1 ? a.icon[(aa - 1) * D + bb - 1] : 0.0;
            const double patch = ((i00 * wx0) * wy0 + (i10 * wx0) * wy1 + (i01 * wx1) * wy0) + (i11 * wx1) * wy1;
            const double keep = 1.0 - patch;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const double cv = (double)((col >> (8 * c)) & 255u);
              v[rr][3 * j + c] = (unsigned)(int)(keep * (double)v[rr][3 * j + c] + patch * cv);
            }
          }
        }
      }
      __syncthreads();                                                // the list is rewritten by the next round
    }
  }

  // ---- store ----
#pragma unroll
  for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
    const int y = ty0 + wave * RN_LANE_ROWS + rr;
    if (y >= a.h || npx <= 0) continue;
    uint8_t* q = a.out + (long long)t * a.o_st + (long long)y * a.o_sy + (long long)x0 * 3;
    if (npx == RN_PX) {
      u128 d = 0;
#pragma unroll
      for (int k = 0; k < RN_PX * 3; ++k) d |= (u128)(v[rr][k] & 255u) << (8 * k);
      store12(q, d);
    } else {
#pragma unroll
      for (int k = 0; k < RN_PX * 3; ++k)
        if (k < npx * 3) q[k] = (uint8_t)v[rr][k];
    }
  }
}

// ---- host: what the three launchers share ----
// the kernel's arguments of a call; dots_need_icon (trails, pose): no icon, no point stage.  t0 is the launch loop's
inline RenderArgs render_args(const RenderCall& c, bool dots_need_icon) {
  RenderArgs a;
  a.frames = c.frames; a.out = c.out; a.ids = c.ids; a.palette = c.palette;
  a.tracks = c.P > 0 && (c.icon || !dots_need_icon) ? c.tracks : nullptr; a.visibles = c.visibles; a.colors = c.colors; a.icon = c.icon;
  a.f_st = c.f_st; a.f_sy = c.f_sy; a.o_st = c.o_st; a.o_sy = c.o_sy; a.i_st = c.i_st; a.i_sy = c.i_sy;
  a.trk_sp = c.trk_sp; a.trk_st = c.trk_st; a.vis_sp = c.vis_sp; a.vis_st = c.vis_st;
  a.t0 = 0; a.h = c.h; a.w = c.w; a.xtiles = cdiv(c.w, RN_COLS); a.alpha = c.alpha; a.contour = c.contour; a.P = c.P; a.radius = c.radius;
  return a;
}

// launch(grid) enqueues the entry's kernel on `a`: once per 65535 frames (grid.y is 16-bit), a.t0 set; `entry` names a failure
template <class Launch>
int render_launches(const char* entry, RenderArgs& a, int T, const Launch& launch) {
  if (a.h == 0 || a.w == 0) return FGVC_OK;
  for (int t0 = 0; t0 < T; t0 += 65535) {
    a.t0 = t0;
    launch(dim3(a.xtiles * cdiv(a.h, RN_ROWS), imin(T - t0, 65535)));
    FGVC_CHECK_LAUNCH(entry);
  }
  return FGVC_OK;
}

}  // namespace fgvc
