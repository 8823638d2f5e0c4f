// Render: mask overlay and point icons onto uint8 RGB video, all T frames in ONE launch -- fgvc_amd/viz.py's host
// backend, bit for bit.  The kernel's body and the tile are render_body.hpp's (shared with trails.hip); this file instantiates it with no
// stage between the overlay and the points.
#include "render_body.hpp"

namespace fgvc {

__global__ __launch_bounds__(RN_BLOCK) void render_frames_kernel(const RenderArgs a) { render_body(a, NoStage{}); }

void render_tile(int* rows, int* cols) {
  *rows = RN_ROWS;
  *cols = RN_COLS;
}

int render_frames_launch(const uint8_t* frames, long long f_st, long long f_sy, uint8_t* out, long long o_st, long long o_sy, int T, int h, int w,
                         const uint8_t* ids, long long i_st, long long i_sy, const uint8_t* palette, int alpha, int contour,
                         const double* tracks, long long trk_sp, long long trk_st, const uint8_t* visibles, long long vis_sp, long long vis_st,
                         const uint8_t* colors, int P, int radius, const double* icon, hipStream_t s) {
  if (T == 0 || h == 0 || w == 0) return FGVC_OK;
  RenderArgs a;
  a.frames = frames; a.out = out; a.ids = ids; a.palette = palette;
  a.tracks = P > 0 ? tracks : nullptr; a.visibles = visibles; a.colors = colors; a.icon = icon;
  a.f_st = f_st; a.f_sy = f_sy; a.o_st = o_st; a.o_sy = o_sy; a.i_st = i_st; a.i_sy = i_sy;
  a.trk_sp = trk_sp; a.trk_st = trk_st; a.vis_sp = vis_sp; a.vis_st = vis_st;
  a.h = h; a.w = w; a.xtiles = cdiv(w, RN_COLS); a.alpha = alpha; a.contour = contour; a.P = P; a.radius = radius;
  for (int t0 = 0; t0 < T; t0 += 65535) {                             // grid.y is 16-bit
    a.t0 = t0;
    const dim3 grid(a.xtiles * cdiv(h, RN_ROWS), imin(T - t0, 65535));
    render_frames_kernel<<<grid, RN_BLOCK, 0, s>>>(a);
    FGVC_CHECK_LAUNCH("fgvc_render_frames_u8");
  }
  return FGVC_OK;
}

}  // namespace fgvc
