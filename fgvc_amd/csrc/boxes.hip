// Boxes and id tags: overlay, then every object's box as a ring outside the box with an optional tag of decimal
// digits on top of it, then the dots, onto uint8 RGB video, all T frames in ONE launch -- fgvc_amd/viz.py's host backend, bit for bit.  The
// load, overlay, points and store are render_body.hpp's, and so are the fill of the shared arguments and the launch loop; this file adds the
// stage between the overlay and the points and the launch line.
//   * thread i of a workgroup turns box i of the frame into a record in LDS (ring, tag, colour, label; 14 words, N <= 255: 14 KB beside the
//     body's 12 KB) and marks it when it draws nothing or misses the workgroup's tile;
//   * every lane then walks the N records in index order (a uniform loop) and tests its RN_LANE_ROWS x RN_PX pixels with integer
//     compares -- ring, then tag, then digits, as the host draws them; a marked record costs one compare.
// Integer arithmetic only: the ring and the tag blend with the overlay's formula, the digits are opaque.
#include "render_body.hpp"

namespace fgvc {

namespace {

constexpr int BOX_LIMIT = 1 << 20;               // a box with a coordinate at or beyond it is not drawn (the host refuses it)

struct BoxArgs {
  const int32_t* boxes;        // [T][N][4] (x0, y0, x1, y1) half-open; frame t at boxes + t * b_st
  const uint8_t* visibles;     // [T][N], frame t at visibles + t * v_st; null: all
  const uint8_t* colors;       // [N][3]
  const int32_t* labels;       // [N] in 0 .. 999, or null: no tags
  const uint8_t* digits;       // [10][7]: bit 4 - c of digits[g][r] is column c of row r of glyph g
  long long b_st, v_st;
  int N, bw, alpha, scale, w;
};

constexpr int BOX_MAX = 255;
constexpr int BOX_FIELDS = 14;     // ring outer 4, box 4, tag 4, style, label

struct BoxStage {
  BoxArgs b;

  // Two steps.  First thread i works out box i of the frame -- its ring, its tag, its colour -- and whether it meets the workgroup's tile at
  // all, and leaves the record in LDS: per-thread work, so every value is a vector register, and the box tables' pointers are dead after
  // it.  Then every lane walks the N records in index order.  (Walking the tables themselves in a uniform loop kept each box's dozen
  // coordinates in scalar registers beside the body's own arguments: 42 of them were spilled.)
  __device__ __forceinline__ void operator()(unsigned (&v)[RN_LANE_ROWS][RN_PX * 3], const RenderLane& k) const {
    __shared__ int rec[BOX_FIELDS][BOX_MAX + 1];
    if (b.N <= 0) return;                                               // (uniform: the barrier below is reached by all or by none)
    if (k.tid < b.N) {
      const int i = k.tid;
      const int32_t* q = b.boxes + (long long)k.t * b.b_st + (long long)i * 4;
      const int x0 = q[0], y0 = q[1], x1 = q[2], y1 = q[3];
      bool draw = x1 > x0 && y1 > y0 && x0 > -BOX_LIMIT && y0 > -BOX_LIMIT && x1 < BOX_LIMIT && y1 < BOX_LIMIT;
      if (draw && b.visibles) draw = b.visibles[(long long)k.t * b.v_st + i] != 0;
      const int ox0 = x0 - b.bw, oy0 = y0 - b.bw, ox1 = x1 + b.bw, oy1 = y1 + b.bw;
      // the tag: (6 d + 1) s x 9 s on top of the ring, inside the box's first rows where it would start above row 0, moved left where it would
      // end beyond the frame
      int tx0 = 0, ty0 = 0, tx1 = 0, ty1 = 0, label = 0, nd = 0;
      if (draw && b.labels) {
        label = b.labels[i];
        if ((unsigned)label <= 999u) {
          nd = label < 10 ? 1 : label < 100 ? 2 : 3;
          const int tw = (6 * nd + 1) * b.scale, th = 9 * b.scale;
          ty0 = oy0 - th < 0 ? y0 : oy0 - th;
          tx0 = ox0 + tw > b.w ? imax(b.w - tw, 0) : ox0;
          tx1 = tx0 + tw;
          ty1 = ty0 + th;
        }
      }
      // what the box touches at all, against the tile
      const int ux0 = nd ? imin(ox0, tx0) : ox0, uy0 = nd ? imin(oy0, ty0) : oy0;
      const int ux1 = nd ? imax(ox1, tx1) : ox1, uy1 = nd ? imax(oy1, ty1) : oy1;
      draw = draw && ux1 > k.tx0 && ux0 < k.tx0 + RN_COLS && uy1 > k.ty0 && uy0 < k.ty0 + RN_ROWS;
      unsigned style = 0;
      if (draw) {
        const uint8_t* c = b.colors + (long long)i * 3;
        const unsigned ink = 299u * c[0] + 587u * c[1] + 114u * c[2] < 128000u ? 1u : 0u;
        style = (unsigned)c[0] | (unsigned)c[1] << 8 | (unsigned)c[2] << 16 | ink << 24 | (unsigned)nd << 25 | 1u << 31;
      }
      rec[0][i] = ox0; rec[1][i] = oy0; rec[2][i] = ox1; rec[3][i] = oy1;
      rec[4][i] = x0; rec[5][i] = y0; rec[6][i] = x1; rec[7][i] = y1;
      rec[8][i] = tx0; rec[9][i] = ty0; rec[10][i] = tx1; rec[11][i] = ty1;
      rec[12][i] = (int)style; rec[13][i] = label;
    }
    __syncthreads();

    const int lx0 = k.tx0 + k.lane * RN_PX, ly0 = k.ty0 + k.wave * RN_LANE_ROWS;     // the lane's first pixel
    const unsigned al = (unsigned)b.alpha, keep = 256u - al;
    const int inv = 65536 / b.scale + 1;                                 // d / scale == (d inv) >> 16 for 0 <= d < 76, scale 1 .. 4
    for (int i = 0; i < b.N; ++i) {
      const unsigned style = (unsigned)rec[12][i];
      if (!(style >> 31)) continue;                                     // draws nothing, or misses the tile (the same in every lane)
      const int ox0 = rec[0][i], oy0 = rec[1][i], ox1 = rec[2][i], oy1 = rec[3][i];
      const int nd = (int)((style >> 25) & 3u);
      const int tx0 = rec[8][i], ty0 = rec[9][i], tx1 = rec[10][i], ty1 = rec[11][i];
      // ... and against the lane's own pixels
      const bool ring_near = ox1 > lx0 && ox0 < lx0 + RN_PX && oy1 > ly0 && oy0 < ly0 + RN_LANE_ROWS;
      const bool tag_near = nd && tx1 > lx0 && tx0 < lx0 + RN_PX && ty1 > ly0 && ty0 < ly0 + RN_LANE_ROWS;
      if (!ring_near && !tag_near) continue;
      const int x0 = rec[4][i], y0 = rec[5][i], x1 = rec[6][i], y1 = rec[7][i], label = rec[13][i];
      const unsigned add[3] = {(style & 255u) * al + 128u, ((style >> 8) & 255u) * al + 128u, ((style >> 16) & 255u) * al + 128u};
      const unsigned ink = (style >> 24) & 1u ? 255u : 0u;
      // Inside-tests as integers, -1 or 0, from sign bits: a compare would leave each of the 18 row and column tests of a lane's eight
      // pixels in a pair of scalar registers (they were what was spilled); |coordinate| < 2^20 + 16, so no difference overflows.
      int row_o[RN_LANE_ROWS], row_i[RN_LANE_ROWS], row_t[RN_LANE_ROWS], col_o[RN_PX], col_i[RN_PX], col_t[RN_PX];   // -1: outside
      const int has_tag = nd ? -1 : 0;
#pragma unroll
      for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
        const int py = ly0 + rr;
        row_o[rr] = ((py - oy0) | (oy1 - 1 - py)) >> 31;
        row_i[rr] = ((py - y0) | (y1 - 1 - py)) >> 31;
        row_t[rr] = ((py - ty0) | (ty1 - 1 - py)) >> 31;
      }
#pragma unroll
      for (int j = 0; j < RN_PX; ++j) {
        const int px = lx0 + j;
        col_o[j] = ((px - ox0) | (ox1 - 1 - px)) >> 31;
        col_i[j] = ((px - x0) | (x1 - 1 - px)) >> 31;
        col_t[j] = ((px - tx0) | (tx1 - 1 - px)) >> 31;
      }
#pragma unroll
      for (int rr = 0; rr < RN_LANE_ROWS; ++rr) {
        const int py = ly0 + rr;
#pragma unroll
        for (int j = 0; j < RN_PX; ++j) {
          const int px = lx0 + j;
          const unsigned ring = (unsigned)(~(row_o[rr] | col_o[j]) & (row_i[rr] | col_i[j]));      // in the outer rectangle, not in the box
          const unsigned tag = (unsigned)(~(row_t[rr] | col_t[j]) & has_tag);
          unsigned lit = 0;
          if (tag) {
            const int u = ((px - tx0) * inv) >> 16, r = ((py - ty0) * inv) >> 16;     // the tag's own pixel: 0 .. 6 d, 0 .. 8
            const int g = (u + 5) / 6 - 1, cc = u - 1 - 6 * g;                      // glyph g = 0 .. d - 1 from the left, its column 0 .. 5
            const int digit = g == nd - 1 ? label % 10 : g == nd - 2 ? (label / 10) % 10 : label / 100;
            const int row = imin(imax(r - 1, 0), 6);
            const unsigned bits = b.digits[digit * 7 + row];
            lit = r >= 1 && r <= 7 && u >= 1 && cc < 5 && ((bits >> (4 - cc)) & 1u) ? ~0u : 0u;
          }
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) {
            unsigned x = v[rr][3 * j + ch];
            x ^= (x ^ ((x * keep + add[ch]) >> 8)) & ring;
            x ^= (x ^ ((x * keep + add[ch]) >> 8)) & tag;
            v[rr][3 * j + ch] = x ^ ((x ^ ink) & lit);
          }
        }
      }
    }
  }
};

}  // namespace

__global__ __launch_bounds__(RN_BLOCK) void render_boxes_kernel(const RenderArgs a, const BoxArgs b) { render_body(a, BoxStage{b}); }

int render_boxes_launch(const RenderCall& c, const int32_t* boxes, long long b_st, const uint8_t* box_visibles, long long v_st,
                        const uint8_t* box_colors, int N, int box_width, int box_alpha, const int32_t* labels, int label_scale,
                        const uint8_t* digits, hipStream_t s) {
  RenderArgs a = render_args(c, false);
  BoxArgs b;
  b.boxes = boxes; b.visibles = box_visibles; b.colors = box_colors; b.labels = labels; b.digits = digits;
  b.b_st = b_st; b.v_st = v_st;
  b.N = boxes ? N : 0; b.bw = box_width; b.alpha = box_alpha; b.scale = label_scale; b.w = c.w;
  return render_launches("fgvc_render_boxes_u8", a, c.T, [&](dim3 grid) { render_boxes_kernel<<<grid, RN_BLOCK, 0, s>>>(a, b); });
}

}  // namespace fgvc
