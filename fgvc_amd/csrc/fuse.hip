// Fusing the forward and the backward label sweep between two annotated frames (test_cfg.refs fuse='linear'; engine.fuse_refs_host is
// the rule in float64).  One launch for every between-annotation frame of a call: item i names a forward row block, a backward row block
// and an output row block [HW][C] f32 by frame indices into their stacks, and a weight w.  Per cell the kernel takes the arg-maximum of
// the forward and of the backward row (the first maximum wins), counts the cells where the two differ, and writes w x + (1 - w) y.
#include "common.hpp"

namespace fgvc {

namespace {

constexpr int FUSE_BLOCK = 256;
constexpr int FUSE_MAX_GRID_X = 1024;

// (value, channel) of the better of two candidates: the larger value, the lower channel among equals
__device__ __forceinline__ void fuse_take(float& v, int& i, float ov, int oi) {
  const bool b = ov > v || (ov == v && oi < i);
  v = b ? ov : v;
  i = b ? oi : i;
}

}  // namespace

// Grid (x, n_items).  A cell's row is shared by G = 2^lg lanes of one wave (G the smallest power of two >= min(C, 64), chosen by the host):
// lane g of the group takes channels g, g + G, ..: consecutive lanes read consecutive floats for every C from 1 to 256, and no lane keeps
// a row in registers.  Each lane blends the elements it loaded and writes them to the same offsets of the output block, so `out` may be
// the forward block itself (no __restrict__ on either).  The groups' (value, channel) pairs are folded with log2(G) wave shuffles; every
// lane of a wave runs them (the loop bound is the same for the whole workgroup), lanes without a cell carry (-inf, IDX_EMPTY).
// Mismatches: per lane in a register, then one LDS atomic per lane that saw any, then ONE 64-bit integer atomic per workgroup into
// counts[item] (zeroed by the launcher): integer sums, the same on every run.
// An item whose frame indices do not lie inside their stacks writes nothing (the wrapper refuses it before the launch).
__global__ __launch_bounds__(FUSE_BLOCK) void seg_fuse_rows_kernel(const float* fw, const float* __restrict__ bw, float* out,
                                                                   const int32_t* __restrict__ items, int n_fw, int n_bw, int n_out,
                                                                   int HW, int C, int lg, unsigned long long* __restrict__ counts) {
  __shared__ unsigned int wg_count;
  const int item = blockIdx.y;
  const int fi = items[4 * item], bi = items[4 * item + 1], oi = items[4 * item + 2];
  if (fi < 0 || fi >= n_fw || bi < 0 || bi >= n_bw || oi < 0 || oi >= n_out) return;   // the same for the whole workgroup
  const float w = __int_as_float(items[4 * item + 3]);
  const float v = 1.f - w;                                                               // rounded once
  const size_t block = (size_t)HW * C;
  const float* x = fw + (size_t)fi * block;
  const float* y = bw + (size_t)bi * block;
  float* o = out + (size_t)oi * block;
  if (threadIdx.x == 0) wg_count = 0u;
  __syncthreads();

  const int G = 1 << lg, g = threadIdx.x & (G - 1);
  const int per_wg = FUSE_BLOCK >> lg;                                                   // cells per workgroup and iteration
  unsigned int mine = 0u;
  for (long long base = (long long)blockIdx.x * per_wg; base < HW; base += (long long)gridDim.x * per_wg) {
    const long long cell = base + (threadIdx.x >> lg);
    const bool live = cell < HW;
    float bx = -INFINITY, by = -INFINITY;
    int ix = IDX_EMPTY, iy = IDX_EMPTY;
    if (live) {
      const size_t row = (size_t)cell * C;
      for (int c = g; c < C; c += G) {
        const float xv = x[row + c], yv = y[row + c];
        if (xv > bx || ix == IDX_EMPTY) { bx = xv; ix = c; }                             // ascending c: the first maximum stays
        if (yv > by || iy == IDX_EMPTY) { by = yv; iy = c; }
        o[row + c] = fmaf(w, xv, __fmul_rn(v, yv));
      }
    }
    for (int s = G >> 1; s >= 1; s >>= 1) {
      fuse_take(bx, ix, __shfl_xor(bx, s, 64), __shfl_xor(ix, s, 64));
      fuse_take(by, iy, __shfl_xor(by, s, 64), __shfl_xor(iy, s, 64));
    }
    mine += (live && g == 0 && ix != iy) ? 1u : 0u;
  }
  if (mine) atomicAdd(&wg_count, mine);
  __syncthreads();
  if (threadIdx.x == 0 && wg_count) atomicAdd(&counts[item], (unsigned long long)wg_count);
}

}  // namespace fgvc

using namespace fgvc;

extern "C" {

int fgvc_seg_fuse_rows_f32(const float* fw, const float* bw, float* out, const int32_t* items, int n_items, int n_fw, int n_bw, int n_out,
                           int HW, int C, int64_t* counts, void* stream) {
  FGVC_REQUIRE(fw && bw && out && items && counts, FGVC_ERR_INVALID_ARG, "fgvc_seg_fuse_rows_f32: null pointer");
  FGVC_REQUIRE(n_items >= 0 && n_items <= 65535 && n_fw > 0 && n_bw > 0 && n_out > 0 && HW > 0 && C >= 1 && C <= 256, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_fuse_rows_f32: bad shape (1 <= C <= 256, n_items <= 65535)");
  if (n_items == 0) return FGVC_OK;
  int lg = 0;
  while ((1 << lg) < C && lg < 6) ++lg;
  const int per_wg = FUSE_BLOCK >> lg;
  const int gx = (int)((HW + (long long)per_wg - 1) / per_wg < FUSE_MAX_GRID_X ? (HW + (long long)per_wg - 1) / per_wg : FUSE_MAX_GRID_X);
  hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_items * sizeof(int64_t), (hipStream_t)stream);
  FGVC_REQUIRE(e == hipSuccess, FGVC_ERR_LAUNCH, "fgvc_seg_fuse_rows_f32: clearing the counts failed: %s", hipGetErrorString(e));
  seg_fuse_rows_kernel<<<dim3(gx, n_items), FUSE_BLOCK, 0, (hipStream_t)stream>>>(fw, bw, out, items, n_fw, n_bw, n_out, HW, C, lg,
                                                                                 (unsigned long long*)counts);
  FGVC_CHECK_LAUNCH("fgvc_seg_fuse_rows_f32");
  return FGVC_OK;
}

}  // extern "C"
