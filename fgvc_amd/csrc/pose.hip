// Pose: overlay, then the joints' heat maps blended in, then the skeleton's limbs as anti-aliased line segments,
// then the dots, onto uint8 RGB video, all T frames in ONE launch -- fgvc_amd/viz.py's host backend, bit for bit.  The load, overlay,
// points and store are render_body.hpp's, and so are the fill of the shared arguments and the launch loop; the limbs are segments.hpp's
// stage (the trail's compaction and per-pixel rule) with an item source of its own; this file adds that source, the heat loop, its
// stage's arguments and the launch lines.
//   * heat: for k = 0 .. K - 1 in order a lane reads its 4 x 2 values of map k (f32 or f64, through the maps' frame, channel and row
//     strides; 16-byte loads where the row's address allows them) and blends colour k in:
//       a = min(max(v gain, 0), 1) alpha with v widened to double;  not a > 0 (zero, negative, NaN): the pixel keeps its value;
//       v_c = (1 - a) v_c + a colour_c, truncated to uint8 after every map;
//   * limbs: on frame t item e is edge (a, b) of the skeleton, from tracks[a][t] + 0.5 to tracks[b][t] + 0.5, seen when both ends are
//     visible on t, of opacity cov limb_alpha and colour limb_colors[e].  An end outside 0 .. P - 1 is not drawn (the host refuses it).
// Float64 with contraction off, every product and sum left to right.  No atomics, no second launch, no workspace.
#include "segments.hpp"

#pragma clang fp contract(off)

namespace fgvc {

namespace {

// what the stage needs beside RenderArgs (whose visibles, strides, P, h and w it reads: the joints are the points)
struct PoseArgs {
  const double* tracks;        // the joints, also when RenderArgs' tracks is null (no dots); null only when E == 0
  const int32_t* skeleton;     // [E][2]
  const uint8_t* limb_colors;  // [E][3]
  const void* heat;            // null: no maps; element (t, k, y, x) at heat[t * h_st + k * h_sk + y * h_sy + x]
  const uint8_t* heat_colors;  // [K][3]
  long long h_st, h_sk, h_sy;
  double ro2, g, limb_alpha, heat_gain, heat_alpha;
  int E, K, reach;
};

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

// the lane's RN_PX values of one row, widened; n of them lie inside the image
__device__ __forceinline__ void load_heat(const float* q, int n, double (&o)[RN_PX]) {
  if (n == RN_PX && (reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
    const f32x4 d = *reinterpret_cast<const f32x4*>(q);
    o[0] = (double)d.x; o[1] = (double)d.y; o[2] = (double)d.z; o[3] = (double)d.w;
    return;
  }
#pragma unroll
  for (int j = 0; j < RN_PX; ++j) o[j] = j < n ? (double)q[j] : 0.0;
}

__device__ __forceinline__ void load_heat(const double* q, int n, double (&o)[RN_PX]) {
  if (n == RN_PX && (reinterpret_cast<uintptr_t>(q) & 15u) == 0) {
    const f64x2 d0 = *reinterpret_cast<const f64x2*>(q), d1 = *reinterpret_cast<const f64x2*>(q + 2);
    o[0] = d0.x; o[1] = d0.y; o[2] = d1.x; o[3] = d1.y;
    return;
  }
#pragma unroll
  for (int j = 0; j < RN_PX; ++j) o[j] = j < n ? q[j] : 0.0;
}

// the item source of segments.hpp: item e of frame t is edge e of the skeleton
struct LimbItems {
  const RenderArgs& a;
  const PoseArgs& b;
  struct Item {
    int e;
  };

  __device__ __forceinline__ void locate(int c, const RenderLane& k, int reach, Item& it, SegmentGeom& sg) const {
    it.e = c;
    const int ja = b.skeleton[2 * c], jb = b.skeleton[2 * c + 1];
    bool seen = (unsigned)ja < (unsigned)a.P && (unsigned)jb < (unsigned)a.P;
    if (seen && a.visibles) {
      const uint8_t* q = a.visibles + (long long)k.t * a.vis_st;
      seen = q[(long long)ja * a.vis_sp] != 0 && q[(long long)jb * a.vis_sp] != 0;
    }
    if (seen) {
      const double* p = b.tracks + (long long)k.t * a.trk_st;
      const double* pa = p + (long long)ja * a.trk_sp;
      const double* pb = p + (long long)jb * a.trk_sp;
      segment_ends(pa[0], pa[1], pb[0], pb[1], reach, k, sg);
    }
  }

  __device__ __forceinline__ double factor(const Item&, const RenderLane&) const { return b.limb_alpha; }

  __device__ __forceinline__ uint32_t colour(const Item& it, const RenderLane&) const {
    const uint8_t* col = b.limb_colors + (long long)it.e * 3;
    return (uint32_t)col[0] | (uint32_t)col[1] << 8 | (uint32_t)col[2] << 16;
  }
};

template <typename HT>
struct PoseStage {
  const RenderArgs& a;
  const PoseArgs& b;

  __device__ __forceinline__ void operator()(unsigned (&v)[RN_LANE_ROWS][RN_PX * 3], const RenderLane& k) const {
    if (b.heat) {
      const int x0 = k.tx0 + k.lane * RN_PX, y0 = k.ty0 + k.wave * RN_LANE_ROWS;
      const int npx = imin(RN_PX, a.w - x0);                          // the lane's columns inside the image (<= 0: none)
      if (npx > 0 && y0 < a.h) {
        const HT* base = static_cast<const HT*>(b.heat) + (long long)k.t * b.h_st + (long long)y0 * b.h_sy + x0;
        for (int m = 0; m < b.K; ++m) {
          const uint8_t* hc = b.heat_colors + m * 3;
          const double c0 = (double)hc[0], c1 = (double)hc[1], c2 = (double)hc[2];
          const HT* q = base + (long long)m * b.h_sk;
#pragma unroll
          for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
            if (y0 + rr >= a.h) continue;
            double hv[RN_PX];
            load_heat(q + (long long)rr * b.h_sy, npx, hv);
#pragma unroll
            for (int j = 0; j < RN_PX; ++j) {
              const double a = fmin(fmax(hv[j] * b.heat_gain, 0.0), 1.0) * b.heat_alpha;
              if (!(a > 0.0)) continue;                               // zero, negative, NaN, and the columns outside: the pixel keeps its value
              const double keep = 1.0 - a;
              v[rr][3 * j + 0] = (unsigned)(int)(keep * (double)v[rr][3 * j + 0] + a * c0);
              v[rr][3 * j + 1] = (unsigned)(int)(keep * (double)v[rr][3 * j + 1] + a * c1);
              v[rr][3 * j + 2] = (unsigned)(int)(keep * (double)v[rr][3 * j + 2] + a * c2);
            }
          }
        }
      }
    }
    if (b.E > 0) segment_stage(v, k, LimbItems{a, b}, b.E, b.ro2, b.g, b.reach);
  }
};

}  // namespace

template <typename HT>
__global__ __launch_bounds__(RN_BLOCK) void render_pose_kernel(const RenderArgs a, const PoseArgs b) { render_body(a, PoseStage<HT>{a, b}); }

// icon == null: no dots; heat == null: no maps; E == 0: no limbs
int render_pose_launch(const RenderCall& c, const int32_t* skeleton, int E, const uint8_t* limb_colors, int reach, double ro2, double g,
                       double limb_alpha, const void* heat, int heat_f64, int K, long long h_st, long long h_sk, long long h_sy,
                       const uint8_t* heat_colors, double heat_gain, double heat_alpha, hipStream_t s) {
  RenderArgs a = render_args(c, true);
  PoseArgs b;
  b.tracks = c.tracks; b.skeleton = skeleton; b.limb_colors = limb_colors;
  b.heat = K > 0 ? heat : nullptr; b.heat_colors = heat_colors;
  b.h_st = h_st; b.h_sk = h_sk; b.h_sy = h_sy;
  b.ro2 = ro2; b.g = g; b.limb_alpha = limb_alpha; b.heat_gain = heat_gain; b.heat_alpha = heat_alpha;
  b.E = c.P > 0 && c.tracks ? E : 0; b.K = K; b.reach = reach;
  return render_launches("fgvc_render_pose_u8", a, c.T, [&](dim3 grid) {
    if (heat_f64)
      render_pose_kernel<double><<<grid, RN_BLOCK, 0, s>>>(a, b);
    else
      render_pose_kernel<float><<<grid, RN_BLOCK, 0, s>>>(a, b);
  });
}

}  // namespace fgvc
