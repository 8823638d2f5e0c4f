// Anti-aliased line segments as a stage of render_body (DESIGN.md sections 21 and 23): the compaction and the per-pixel rule that the trail
// stage (trails.hip) and the limb stage (pose.hip) share.  What differs between the two is where an item's two ends, its opacity and its
// colour come from: the item source, a template argument.
//   * the workgroup walks the frame's `items` candidates RN_BLOCK at a time and compacts IN ITEM ORDER (ballot + prefix count per wave, wave
//     totals through LDS) those the source shows (both ends visible), whose four coordinates are below 2^20 in magnitude (which NaN and the
//     infinities are not) and whose box, grown by ceil(ro), meets the tile, into an LDS list: ax, ay, dx, dy, L2, the opacity factor, the
//     packed colour and the box cut to the tile (4 bytes).  56 bytes per item, 14 KB;
//   * every lane then walks the list for its 8 pixels: one integer compare of its 4 x 2 block against the item's box before any double,
//     then per pixel the distance to the segment without a square root and with ONE division (correctly rounded: no fast-math),
//       u = clamp(((px - ax) dx + (py - ay) dy) / L2, 0, 1) (0 when L2 == 0),  d2 = |p - (a + u d)|^2,  cov = clamp((ro2 - d2) g, 0, 1),
//       v_c = (1 - cov f) v_c + cov f colour_c, truncated to uint8 after every segment;
//     a pixel outside the box (floor of the smaller end - ceil(ro) .. ceil of the larger end + ceil(ro)) is ceil(ro) + 1 or more away from
//     the segment in x or in y, so d2 - ro2 >= 2 ceil(ro) + 1 against a rounding error below 2^-10 at the 2^20 limit: its cov is exactly 0,
//     it would keep its value, and leaving it out changes nothing.
// A source has
//     struct Item;                                                          what locate() found, handed on to paint()
//     void locate(int c, const RenderLane&, int reach, Item&, SegmentGeom&) const;      an item that is seen hands its ends to segment_ends()
//     double factor(const Item&, const RenderLane&) const;  uint32_t colour(const Item&, const RenderLane&) const;   of an item that is kept
// Float64 with contraction off, every product and sum left to right.
#pragma once

#include "render_body.hpp"

#pragma clang fp contract(off)

namespace fgvc {

constexpr double SEGMENT_LIMIT = 1048576.0;        // 2^20: beyond it a coordinate is not drawn (and every integer below is exact)

// what the list keeps of a segment's geometry; `take` of an item that is not kept stays false
struct SegmentGeom {
  double ax = 0.0, ay = 0.0, dx = 0.0, dy = 0.0;
  uint32_t box = 0;
  bool take = false;
};

// the two ends of a segment that its source has seen -> the geometry, and whether the segment is drawn on this tile: called by a source's locate()
__device__ __forceinline__ void segment_ends(double x0, double y0, double x1, double y1, int reach, const RenderLane& k, SegmentGeom& s) {
  if (fabs(x0) < SEGMENT_LIMIT && fabs(y0) < SEGMENT_LIMIT && fabs(x1) < SEGMENT_LIMIT && fabs(y1) < SEGMENT_LIMIT) {   // false for NaN
    s.ax = x0 + 0.5;
    s.ay = y0 + 0.5;
    const double bx = x1 + 0.5, by = y1 + 0.5;
    s.dx = bx - s.ax;
    s.dy = by - s.ay;
    const int xlo = (int)floor(fmin(s.ax, bx)) - reach - k.tx0, xhi = (int)ceil(fmax(s.ax, bx)) + reach - k.tx0;   // in the tile's frame
    const int ylo = (int)floor(fmin(s.ay, by)) - reach - k.ty0, yhi = (int)ceil(fmax(s.ay, by)) + reach - k.ty0;
    s.take = xhi >= 0 && xlo < RN_COLS && yhi >= 0 && ylo < RN_ROWS;
    s.box = (uint32_t)imax(xlo, 0) | (uint32_t)imin(xhi, RN_COLS - 1) << 8 | (uint32_t)imax(ylo, 0) << 16 |
            (uint32_t)imin(yhi, RN_ROWS - 1) << 24;
  }
}

template <class Source>
__device__ __forceinline__ void segment_stage(unsigned (&v)[RN_LANE_ROWS][RN_PX * 3], const RenderLane& k, const Source& src, int items,
                                              double ro2, double g, int reach) {
  __shared__ double l_ax[RN_BLOCK], l_ay[RN_BLOCK], l_dx[RN_BLOCK], l_dy[RN_BLOCK], l_l2[RN_BLOCK], l_fade[RN_BLOCK];
  __shared__ uint32_t l_col[RN_BLOCK], l_box[RN_BLOCK];
  __shared__ int wave_n[RN_WAVES];
  const int lx = k.lane * RN_PX, ly = k.wave * RN_LANE_ROWS;          // the lane's block inside the tile
  for (int base = 0; base < items; base += RN_BLOCK) {
    const int c = base + k.tid;
    SegmentGeom sg;
    typename Source::Item it{};
    if (c < items) src.locate(c, k, reach, it, sg);
    const bool take = sg.take;
    const double ax = sg.ax, ay = sg.ay, dx = sg.dx, dy = sg.dy;
    const uint32_t box = sg.box;
    const unsigned long long bal = __ballot(take);
    const int before = __popcll(bal & ((1ull << k.lane) - 1ull));
    if (k.lane == 0) wave_n[k.wave] = __popcll(bal);
    __syncthreads();
    int off = 0, kept = 0;
#pragma unroll
    for (int wv = 0; wv < RN_WAVES; ++wv) {
      const int cnt = wave_n[wv];
      off += wv < k.wave ? cnt : 0;
      kept += cnt;
    }
    if (take) {
      const int e = off + before;
      l_ax[e] = ax;
      l_ay[e] = ay;
      l_dx[e] = dx;
      l_dy[e] = dy;
      l_l2[e] = dx * dx + dy * dy;
      l_fade[e] = src.factor(it, k);
      l_col[e] = src.colour(it, k);
      l_box[e] = box;
    }
    __syncthreads();
    for (int e = 0; e < kept; ++e) {
      const uint32_t bb = l_box[e];
      const int bx0 = (int)(bb & 255u), bx1 = (int)((bb >> 8) & 255u), by0 = (int)((bb >> 16) & 255u), by1 = (int)(bb >> 24);
      if (lx + RN_PX - 1 < bx0 || lx > bx1 || ly + RN_LANE_ROWS - 1 < by0 || ly > by1) continue;
      const double sax = l_ax[e], say = l_ay[e], sdx = l_dx[e], sdy = l_dy[e], l2 = l_l2[e], fd = l_fade[e];
      const uint32_t col = l_col[e];
#pragma unroll
      for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
        if (ly + rr < by0 || ly + rr > by1) continue;
        const double py = (double)(k.ty0 + ly + rr);
#pragma unroll
        for (int j = 0; j < RN_PX; ++j) {
          if (lx + j < bx0 || lx + j > bx1) continue;
          const double px = (double)(k.tx0 + lx + j);
          const double q = ((px - sax) * sdx + (py - say) * sdy) / l2;
          const double u = l2 == 0.0 ? 0.0 : fmin(fmax(q, 0.0), 1.0);
          const double ex = px - (sax + u * sdx), ey = py - (say + u * sdy);
          const double d2 = ex * ex + ey * ey;
          const double cov = fmin(fmax((ro2 - d2) * g, 0.0), 1.0);
          if (!(cov > 0.0)) continue;                               // the pixel keeps its value
          const double op = cov * fd, keep = 1.0 - op;
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            const double cv = (double)((col >> (8 * ch)) & 255u);
            v[rr][3 * j + ch] = (unsigned)(int)(keep * (double)v[rr][3 * j + ch] + op * cv);
          }
        }
      }
    }
    __syncthreads();                                                // the list is rewritten by the next round
  }
}

}  // namespace fgvc
