// Motion trails: overlay, then every point's last L steps as anti-aliased line segments, then the dots, onto uint8
// RGB video, all T frames in ONE launch -- fgvc_amd/viz.py's host backend, bit for bit.  The load, overlay, points and store are
// render_body.hpp's, and so are the fill of the shared arguments and the launch loop; the stage between the overlay and the points is segments.hpp's (the compaction and the per-pixel rule, shared with
// pose.hip's limbs); this file adds where a trail's items come from, its stage's arguments and the launch line.
//   * on frame t a point has n = min(t, L) segments, s = t - n .. t - 1, segment s from tracks[i][s] + 0.5 to tracks[i][s + 1] + 0.5: the
//     frame's P n candidate items (item = i n + k, s = t - n + k: point order, oldest first), each with the fade factor of its age;
//   * the list is 14 KB beside the point stage's 12 KB: 26.4 KB, six workgroups of 4 waves in a compute unit's 160 KB, which is also what
//     its 79 VGPRs admit (six waves per SIMD).
// Float64 with contraction off, every product and sum left to right.  No atomics, no second launch, no workspace.
#include "segments.hpp"

#pragma clang fp contract(off)

namespace fgvc {

namespace {

struct TrailArgs {
  const double* tracks;        // never null here
  const uint8_t* visibles;     // null: all visible
  const uint8_t* colors;       // [P][3]: colour of point i (used when time_colors is null)
  const uint8_t* time_colors;  // [T - 1][3]: colour of segment s, or null
  const double* fade;          // [L]: by age t - 1 - s
  long long trk_sp, trk_st, vis_sp, vis_st;
  double ro2, g;
  int P, L, reach;             // reach = ceil(ro)
};

// the item source of segments.hpp: item c of frame t is step s = s0 + c % n of point i = c / n
struct TrailItems {
  const TrailArgs& b;
  int n, s0;
  struct Item {
    int i, s;
  };

  __device__ __forceinline__ void locate(int c, const RenderLane& k, int reach, Item& it, SegmentGeom& sg) const {
    const int i = (int)((unsigned)c / (unsigned)n);
    const int s = s0 + (c - i * n);
    it.i = i;
    it.s = s;
    bool seen = true;
    if (b.visibles) {
      const uint8_t* q = b.visibles + (long long)i * b.vis_sp + (long long)s * b.vis_st;
      seen = q[0] != 0 && q[b.vis_st] != 0;
    }
    if (seen) {
      const double* p = b.tracks + (long long)i * b.trk_sp + (long long)s * b.trk_st;
      segment_ends(p[0], p[1], p[b.trk_st], p[b.trk_st + 1], reach, k, sg);
    }
  }

  __device__ __forceinline__ double factor(const Item& it, const RenderLane& k) const { return b.fade[k.t - 1 - it.s]; }

  __device__ __forceinline__ uint32_t colour(const Item& it, const RenderLane&) const {
    const uint8_t* col = b.time_colors ? b.time_colors + (long long)it.s * 3 : b.colors + (long long)it.i * 3;
    return (uint32_t)col[0] | (uint32_t)col[1] << 8 | (uint32_t)col[2] << 16;
  }
};

struct TrailStage {
  TrailArgs b;

  __device__ __forceinline__ void operator()(unsigned (&v)[RN_LANE_ROWS][RN_PX * 3], const RenderLane& k) const {
    const int n = imin(k.t, b.L);                                     // segments per point on this frame (uniform in the workgroup)
    if (n <= 0) return;
    segment_stage(v, k, TrailItems{b, n, k.t - n}, b.P * n, b.ro2, b.g, b.reach);   // P L < 2^31 (checked on the host)
  }
};

}  // namespace

__global__ __launch_bounds__(RN_BLOCK) void render_trails_kernel(const RenderArgs a, const TrailArgs b) { render_body(a, TrailStage{b}); }

// icon == null: no dots (the trails alone)
int render_trails_launch(const RenderCall& c, int trail, int reach, double ro2, double g, const double* fade, const uint8_t* time_colors,
                         hipStream_t s) {
  RenderArgs a = render_args(c, true);
  TrailArgs b;
  b.tracks = c.tracks; b.visibles = c.visibles; b.colors = c.colors; b.time_colors = time_colors; b.fade = fade;
  b.trk_sp = c.trk_sp; b.trk_st = c.trk_st; b.vis_sp = c.vis_sp; b.vis_st = c.vis_st;
  b.ro2 = ro2; b.g = g; b.P = c.P; b.L = c.P > 0 ? trail : 0; b.reach = reach;
  return render_launches("fgvc_render_trails_u8", a, c.T, [&](dim3 grid) { render_trails_kernel<<<grid, RN_BLOCK, 0, s>>>(a, b); });
}

}  // namespace fgvc
