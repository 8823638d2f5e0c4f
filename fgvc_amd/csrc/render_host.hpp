// The host side the render entries share (fgvc_render_frames_u8, _trails_u8, _pose_u8, _boxes_u8: DESIGN.md sections 16, 21, 23 and 27): the
// arguments they have in common, in the order of include/fgvc_hip.h, and the launchers capi.hip hands them to.  No device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace fgvc {

struct RenderCall {
  const uint8_t* frames;
  long long f_st, f_sy;
  uint8_t* out;
  long long o_st, o_sy;
  int T, h, w;
  const uint8_t* ids;          // null: no overlay
  long long i_st, i_sy;
  const uint8_t* palette;
  int alpha, contour;
  const double* tracks;        // null: no points
  long long trk_sp, trk_st;
  const uint8_t* visibles;     // null: all visible
  long long vis_sp, vis_st;
  const uint8_t* colors;
  int P, radius;
  const double* icon;          // trails and pose: null for no dots
};

void render_tile(int* rows, int* cols);
int render_frames_launch(const RenderCall& c, hipStream_t s);
int render_trails_launch(const RenderCall& c, int trail, int reach, double ro2, double g, const double* fade, const uint8_t* time_colors,
                         hipStream_t s);
int render_pose_launch(const RenderCall& c, const int32_t* skeleton, int E, const uint8_t* limb_colors, int reach, double ro2, double g,
                       double limb_alpha, const void* heat, int heat_f64, int K, long long h_st, long long h_sk, long long h_sy,
                       const uint8_t* heat_colors, double heat_gain, double heat_alpha, hipStream_t s);
int render_boxes_launch(const RenderCall& c, const int32_t* boxes, long long b_st, const uint8_t* box_visibles, long long v_st,
                        const uint8_t* box_colors, int N, int box_width, int box_alpha, const int32_t* labels, int label_scale,
                        const uint8_t* digits, hipStream_t s);

}  // namespace fgvc
