// Render: mask overlay and point icons onto uint8 RGB video, all T frames in ONE launch -- fgvc_amd/viz.py's host
// backend, bit for bit.  The kernel's body, the tile, the fill of its arguments and the launch loop are render_body.hpp's (shared with
// trails.hip and pose.hip); this file instantiates the body with no stage between the overlay and the points and has the launch line.
#include "render_body.hpp"

namespace fgvc {

__global__ __launch_bounds__(RN_BLOCK) void render_frames_kernel(const RenderArgs a) { render_body(a, NoStage{}); }

void render_tile(int* rows, int* cols) {
  *rows = RN_ROWS;
  *cols = RN_COLS;
}

int render_frames_launch(const RenderCall& c, hipStream_t s) {
  RenderArgs a = render_args(c, false);
  return render_launches("fgvc_render_frames_u8", a, c.T, [&](dim3 grid) { render_frames_kernel<<<grid, RN_BLOCK, 0, s>>>(a); });
}

}  // namespace fgvc
