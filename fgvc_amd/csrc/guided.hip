// Edge-aware mask read-out (test_cfg.readout = dict(type='guided')): joint bilateral upsampling of the label grid,
// guided by the padded Lab frames the encoder read.  engine.guided_readout_host states the rule in float64; this file runs it in f32.
//
//   pre-pass    guide_cells_kernel       cell colours [n][Hf*Wf][3]: the mean of the guide over each cell's (hp / Hf) x (wp / Wf) block
//               guided_extremes_kernel   per (frame, channel) min / max of the labels over the FEATURE GRID, as order-preserving keys
//   main        guided_readout_kernel    one launch for all frames: ids, and under CONF confidence bytes and per-id statistics
//
// Geometry is integer: with N = clamp((2 o + 1) n_unpad, n_out, (2 n_unpad - 1) n_out) + 2 n_out off, the padded-frame coordinate of output
// o is p + 0.5 = N / (2 n_out), so the centre cell floor((p + 0.5) / s), the offset of the grid coordinate from it and the bilinear taps of
// the guide come from one integer division each.  No rounding can move a pixel that lies exactly half-way between two cells to the
// other window, and the only f32 roundings of a spatial offset are one division and one subtraction.
#include "common.hpp"

namespace fgvc {

namespace {

constexpr int GD_BLOCK = 256;
constexpr int GD_TW = 32, GD_TH = 8;            // output tile of a workgroup: one pixel per lane, a wave = two tile rows
constexpr int GD_CH = 16;                       // label channels staged in LDS at a time
constexpr int GD_LDS_MAX = 64 * 1024;
constexpr int GD_CELLS_MAX_WP = (GD_LDS_MAX / 4) / 3;   // guide_cells_kernel keeps 3 rows of column sums in LDS

struct GdAxis {
  int n_out, n_unpad, n_pad, off, s, n_cells;   // s = n_pad / n_cells pixels per cell
};

// output coordinate o -> centre cell, t = (grid coordinate - centre cell) in [-0.5, 0.5), and the guide's bilinear taps p0, p1 with weight l of p1
__host__ __device__ __forceinline__ int gd_units(const GdAxis& a, int o) {
  int N = (2 * o + 1) * a.n_unpad;
  const int lo = a.n_out, hi = (2 * a.n_unpad - 1) * a.n_out;
  N = N < lo ? lo : (N > hi ? hi : N);
  return N + 2 * a.n_out * a.off;
}
__host__ __device__ __forceinline__ int gd_cell(const GdAxis& a, int o) { return gd_units(a, o) / (2 * a.n_out * a.s); }
__device__ __forceinline__ void gd_pos(const GdAxis& a, int o, int& cell, float& t, int& p0, int& p1, float& l) {
  const int N = gd_units(a, o), D = 2 * a.n_out * a.s, U = 2 * a.n_out;
  cell = N / D;
  t = (float)(N - cell * D) / (float)D - 0.5f;
  const int M = N - a.n_out;                    // (p) in units of 1 / U, >= 0
  p0 = M / U;
  l = (float)(M - p0 * U) / (float)U;
  p1 = imin(p0 + 1, a.n_pad - 1);
}

struct GdGeom {
  GdAxis y, x;
  int C, FW, plane;        // FW: row stride of a footprint plane in LDS (the widest footprint of any tile); plane: words per plane (odd)
  int norm;
  float inv2ss, inv2sr;    // 1 / (2 sigma_space^2), 1 / (2 sigma_range^2)
};

// order-preserving key of a float: a < b <=> key(a) < key(b); every key is > 0, so a cleared word is below all of them
__device__ __forceinline__ uint32_t gd_key(float v) {
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gd_unkey(uint32_t k) {
  return __builtin_bit_cast(float, (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

}  // namespace

// cell colours: grid (Hf, n).  Column sums over the cell row's sy pixel rows (coalesced reads), then sx of them per cell from LDS.  Both
// sums run in order, so a cell's value is within (sy + sx - 1) roundings of the exact mean.
__global__ __launch_bounds__(GD_BLOCK) void guide_cells_kernel(const float* __restrict__ guide, int hp, int wp, int Hf, int Wf,
                                                               float* __restrict__ cells) {
  extern __shared__ float col[];  // [3][wp]
  const int i = blockIdx.x, f = blockIdx.y, sy = hp / Hf, sx = wp / Wf;
  for (int idx = threadIdx.x; idx < 3 * wp; idx += GD_BLOCK) {
    const int ch = idx / wp, x = idx - ch * wp;
    const float* p = guide + ((size_t)(f * 3 + ch) * hp + (size_t)i * sy) * wp + x;
    float s = p[0];
    for (int r = 1; r < sy; ++r) s += p[(size_t)r * wp];
    col[idx] = s;
  }
  __syncthreads();
  const float inv = (float)(sy * sx);
  for (int idx = threadIdx.x; idx < 3 * Wf; idx += GD_BLOCK) {
    const int j = idx / 3, ch = idx - 3 * j;
    const float* q = col + ch * wp + j * sx;
    float s = q[0];
    for (int k = 1; k < sx; ++k) s += q[k];
    cells[((size_t)(f * Hf + i) * Wf + j) * 3 + ch] = s / inv;
  }
}

// grid extremes: grid (NB, n).  A lane keeps one channel (its stride is a multiple of C); the workgroup folds in LDS, then adds its C pairs
// to mm [n][C][2] = key(max), key(-min) with integer atomic maxima: order-independent.  mm is zero on entry.
__global__ __launch_bounds__(GD_BLOCK) void guided_extremes_kernel(const float* __restrict__ labels, int HW, int C, uint32_t* __restrict__ mm) {
  __shared__ uint32_t red[2 * 256];
  const int f = blockIdx.y, step = (GD_BLOCK / C) * C;
  for (int c = threadIdx.x; c < 2 * C; c += GD_BLOCK) red[c] = 0u;
  __syncthreads();
  if ((int)threadIdx.x < step) {
    const int c = threadIdx.x % C;
    const long long total = (long long)HW * C;
    const float* lab = labels + (size_t)f * total;
    float mn = INFINITY, mx = -INFINITY;
    for (long long idx = (long long)blockIdx.x * step + threadIdx.x; idx < total; idx += (long long)gridDim.x * step) {
      const float v = lab[idx];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    if (mx >= mn) {
      atomicMax(&red[2 * c], gd_key(mx));
      atomicMax(&red[2 * c + 1], gd_key(-mn));
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < 2 * C; c += GD_BLOCK)
    if (red[c] != 0u) atomicMax(&mm[(size_t)f * 2 * C + c], red[c]);
}

// The read-out: grid (tiles x, tiles y, n), one output pixel per lane.
//   1  stage the cell colours of the tile's footprint (its centre cells +- R, inside the grid) in LDS, planar: gc [3][plane];
//   2  per lane: the guide sampled bilinearly at the pixel, the (2 R + 1)^2 exponents, their minimum, w = exp(-(e - e_min)) in registers
//      (a tap outside the grid has e = inf, w = 0; the centre cell is always inside, so the sum of the weights is >= 1);
//   3  per chunk of GD_CH channels: stage the normalised labels of the footprint, planar: lab [GD_CH][plane]; every lane forms
//      sum(w L) / sum(w) per channel and keeps a running best, second and argmax (the first maximum wins);
//   4  ids (CONF: and confidence bytes, and (count, conf sum) per id through LDS counters and 64-bit integer atomics).
// Planes are `plane` words apart with plane odd: the staging writes (lanes run over channels first) spread over the banks, and the
// tap reads of a wave are consecutive cells of one plane (or one cell, broadcast).
template <int R, bool CONF>
__global__ __launch_bounds__(GD_BLOCK) void guided_readout_kernel(const float* __restrict__ labels, const float* __restrict__ guide,
                                                                  const float* __restrict__ cells, const uint32_t* __restrict__ mm,
                                                                  GdGeom g, uint8_t* __restrict__ masks, uint8_t* __restrict__ conf,
                                                                  unsigned long long* __restrict__ stats) {
  constexpr int D = 2 * R + 1;
  extern __shared__ float lds[];
  float* gc = lds;                       // [3][plane]
  float* lab = lds + 3 * g.plane;        // [GD_CH][plane]
  [[maybe_unused]] uint32_t* cnt = reinterpret_cast<uint32_t*>(lab + GD_CH * g.plane);   // CONF: cnt [C] | sum [C]
  const int f = blockIdx.z, C = g.C, Hf = g.y.n_cells, Wf = g.x.n_cells;
  const int ty0 = blockIdx.y * GD_TH, tx0 = blockIdx.x * GD_TW;
  const int lx = threadIdx.x & (GD_TW - 1), ly = threadIdx.x / GD_TW;
  const bool live = ty0 + ly < g.y.n_out && tx0 + lx < g.x.n_out;
  const int oy = imin(ty0 + ly, g.y.n_out - 1), ox = imin(tx0 + lx, g.x.n_out - 1);
  // the tile's footprint on the grid (gd_cell is monotonic in the output coordinate)
  const int fy0 = imax(gd_cell(g.y, ty0) - R, 0), fy1 = imin(gd_cell(g.y, imin(ty0 + GD_TH, g.y.n_out) - 1) + R, Hf - 1);
  const int fx0 = imax(gd_cell(g.x, tx0) - R, 0), fx1 = imin(gd_cell(g.x, imin(tx0 + GD_TW, g.x.n_out) - 1) + R, Wf - 1);
  const int FH = fy1 - fy0 + 1, FWb = fx1 - fx0 + 1;

  for (int idx = threadIdx.x; idx < FH * FWb * 3; idx += GD_BLOCK) {
    const int cell = idx / 3, ch = idx - 3 * cell;
    const int i = cell / FWb, j = cell - i * FWb;
    gc[ch * g.plane + i * g.FW + j] = cells[((size_t)(f * Hf + fy0 + i) * Wf + fx0 + j) * 3 + ch];
  }
  if constexpr (CONF)
    for (int c = threadIdx.x; c < 2 * C; c += GD_BLOCK) cnt[c] = 0u;

  int cy, cx, y0, y1, x0, x1;
  float ty, tx, wy, wx;
  gd_pos(g.y, oy, cy, ty, y0, y1, wy);
  gd_pos(g.x, ox, cx, tx, x0, x1, wx);
  float I[3];
  {
    const size_t hw = (size_t)g.y.n_pad * g.x.n_pad;
    const float* gf = guide + (size_t)f * 3 * hw;
    const size_t r0 = (size_t)y0 * g.x.n_pad, r1 = (size_t)y1 * g.x.n_pad;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const float* p = gf + ch * hw;
      const float a = p[r0 + x0], b = p[r0 + x1], c = p[r1 + x0], d = p[r1 + x1];
      const float top = fmaf(wx, b - a, a), bot = fmaf(wx, d - c, c);
      I[ch] = fmaf(wy, bot - top, top);
    }
  }
  // clamped tap rows (times the row stride) and columns, relative to the footprint: a clamped tap reads a staged cell and has weight 0
  int ri[D], cj[D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    ri[a] = (imin(imax(cy + a - R, 0), Hf - 1) - fy0) * g.FW;
    cj[a] = imin(imax(cx + a - R, 0), Wf - 1) - fx0;
  }
  __syncthreads();
  float w[D * D];
  float emin = INFINITY;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    const float dy = (float)(a - R) - ty;
    const bool iny = (unsigned)(cy + a - R) < (unsigned)Hf;
#pragma unroll
    for (int b = 0; b < D; ++b) {
      const float dx = (float)(b - R) - tx;
      const bool in = iny && (unsigned)(cx + b - R) < (unsigned)Wf;
      const int cs = ri[a] + cj[b];
      const float d0 = I[0] - gc[cs], d1 = I[1] - gc[g.plane + cs], d2 = I[2] - gc[2 * g.plane + cs];
      float e = (dy * dy + dx * dx) * g.inv2ss + (d0 * d0 + d1 * d1 + d2 * d2) * g.inv2sr;
      e = in ? e : INFINITY;
      w[a * D + b] = e;
      emin = fminf(emin, e);
    }
  }
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < D * D; ++k) {
    w[k] = expf(-(w[k] - emin));
    den += w[k];
  }
  const float rden = 1.f / den;

  float best = -INFINITY, second = -INFINITY;
  int bi = 0;
  for (int c0 = 0; c0 < C; c0 += GD_CH) {
    const int nc = imin(GD_CH, C - c0);
    if (c0 > 0) __syncthreads();          // the previous chunk has been read
    for (int idx = threadIdx.x; idx < FH * FWb * nc; idx += GD_BLOCK) {
      const int cell = idx / nc, c = idx - cell * nc;
      const int i = cell / FWb, j = cell - i * FWb;
      float v = labels[((size_t)(f * Hf + fy0 + i) * Wf + fx0 + j) * C + c0 + c];
      if (g.norm) {
        // torch.where(max > 0, (x - min) / (max - min + 1e-12), x), the extremes taken over the feature grid
        const uint32_t* k = mm + ((size_t)f * C + c0 + c) * 2;
        const float mx = gd_unkey(k[0]), mn = -gd_unkey(k[1]);
        if (mx > 0.f) v = (v - mn) / ((mx - mn) + 1e-12f);
      }
      lab[c * g.plane + i * g.FW + j] = v;
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      const float* lp = lab + c * g.plane;
      float num = 0.f;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) num = fmaf(w[a * D + b], lp[ri[a] + cj[b]], num);
      const float v = num * rden;
      const bool first = c0 + c == 0;
      if constexpr (CONF) second = (first || v > best) ? best : fmaxf(second, v);
      if (first || v > best) {
        best = v;
        bi = c0 + c;
      }
    }
  }
  const size_t o = ((size_t)f * g.y.n_out + oy) * g.x.n_out + ox;
  if (live) masks[o] = (uint8_t)bi;
  if constexpr (CONF) {
    if (live) {
      const float gap = fminf(fmaxf(best - second, 0.f), 1.f);    // C == 1: second is -inf, the byte is 255
      const uint32_t cb = (uint32_t)rintf(255.f * gap);
      conf[o] = (uint8_t)cb;
      atomicAdd(&cnt[bi], 1u);
      atomicAdd(&cnt[C + bi], cb);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += GD_BLOCK)
      if (cnt[c] != 0u) {
        unsigned long long* dst = stats + ((size_t)f * C + c) * 2;
        atomicAdd(dst, (unsigned long long)cnt[c]);
        atomicAdd(dst + 1, (unsigned long long)cnt[C + c]);
      }
  }
}

namespace {

// the widest and tallest footprint of any tile along one axis
int gd_max_footprint(const GdAxis& a, int tile, int R) {
  int m = 0;
  for (int t0 = 0; t0 < a.n_out; t0 += tile) {
    const int lo = imax(gd_cell(a, t0) - R, 0), hi = imin(gd_cell(a, imin(t0 + tile, a.n_out) - 1) + R, a.n_cells - 1);
    m = imax(m, hi - lo + 1);
  }
  return m;
}

template <bool CONF>
void gd_launch(int radius, dim3 grid, size_t lds, hipStream_t s, const float* labels, const float* guide, const float* cells,
               const uint32_t* mm, const GdGeom& g, uint8_t* masks, uint8_t* conf, unsigned long long* stats) {
  if (radius == 1)
    guided_readout_kernel<1, CONF><<<grid, GD_BLOCK, lds, s>>>(labels, guide, cells, mm, g, masks, conf, stats);
  else if (radius == 2)
    guided_readout_kernel<2, CONF><<<grid, GD_BLOCK, lds, s>>>(labels, guide, cells, mm, g, masks, conf, stats);
  else
    guided_readout_kernel<3, CONF><<<grid, GD_BLOCK, lds, s>>>(labels, guide, cells, mm, g, masks, conf, stats);
}

int gd_readout(const char* name, bool with_conf, const float* labels, const float* guide, const float* cells, int n, int Hf, int Wf, int C,
               int hp, int wp, int top, int left, int h, int w, int h0, int w0, int norm, int radius, double sigma_space,
               double sigma_range, uint8_t* masks, uint8_t* conf, int64_t* stats, void* workspace, void* stream) {
  FGVC_REQUIRE(labels && guide && cells && masks, FGVC_ERR_INVALID_ARG, "%s: null pointer", name);
  FGVC_REQUIRE(!with_conf || (conf && stats), FGVC_ERR_INVALID_ARG, "%s: null conf / stats buffer", name);
  FGVC_REQUIRE(!with_conf || (conf != masks), FGVC_ERR_INVALID_ARG, "%s: conf and masks are one buffer", name);
  FGVC_REQUIRE(C >= 1 && C <= 256, FGVC_ERR_INVALID_ARG, "%s: C = %d outside 1..256", name, C);
  FGVC_REQUIRE(radius >= 1 && radius <= 3, FGVC_ERR_INVALID_ARG, "%s: radius = %d outside 1..3", name, radius);
  FGVC_REQUIRE(isfinite(sigma_space) && sigma_space > 0.0, FGVC_ERR_INVALID_ARG, "%s: sigma_space must be positive and finite", name);
  FGVC_REQUIRE(isfinite(sigma_range) && sigma_range > 0.0, FGVC_ERR_INVALID_ARG, "%s: sigma_range must be positive and finite", name);
  FGVC_REQUIRE(n >= 0 && n <= 65535 && Hf > 0 && Wf > 0 && hp > 0 && wp > 0 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG,
               "%s: bad shape (n <= 65535)", name);
  FGVC_REQUIRE(hp % Hf == 0 && wp % Wf == 0, FGVC_ERR_INVALID_ARG,
               "%s: the feature grid %d x %d does not divide the padded frame %d x %d", name, Hf, Wf, hp, wp);
  FGVC_REQUIRE(h > 0 && w > 0 && top >= 0 && left >= 0 && top + h <= hp && left + w <= wp, FGVC_ERR_INVALID_ARG,
               "%s: the unpadded window must lie inside the padded frame", name);
  // the integer geometry: N < 2 n_out (n_pad + 1) must fit an int, and a remainder below 2 n_out s must be exact in f32
  FGVC_REQUIRE((long long)h0 * (hp + 1) < (1ll << 29) && (long long)w0 * (wp + 1) < (1ll << 29) && (long long)h0 * (hp / Hf) <= (1ll << 23) &&
                   (long long)w0 * (wp / Wf) <= (1ll << 23) && (long long)n * Hf * Wf < (1ll << 31),
               FGVC_ERR_UNSUPPORTED, "%s: frame or output size out of range", name);
  FGVC_REQUIRE(workspace != nullptr || n == 0, FGVC_ERR_INVALID_ARG,
               "%s: workspace of fgvc_seg_readout_guided_workspace_bytes() bytes required", name);
  if (n == 0) return FGVC_OK;
  GdGeom g;
  g.y = GdAxis{h0, h, hp, top, hp / Hf, Hf};
  g.x = GdAxis{w0, w, wp, left, wp / Wf, Wf};
  g.C = C;
  g.norm = norm != 0;
  g.inv2ss = (float)(1.0 / (2.0 * sigma_space * sigma_space));
  g.inv2sr = (float)(1.0 / (2.0 * sigma_range * sigma_range));
  const int FH = gd_max_footprint(g.y, GD_TH, radius);
  g.FW = gd_max_footprint(g.x, GD_TW, radius);
  g.plane = (FH * g.FW) | 1;
  const size_t lds = ((size_t)(3 + GD_CH) * g.plane + (with_conf ? 2 * C : 0)) * sizeof(float);
  FGVC_REQUIRE(lds <= (size_t)GD_LDS_MAX, FGVC_ERR_UNSUPPORTED,
               "%s: a tile's footprint of %d x %d cells does not fit the LDS (an output much smaller than the frame)", name, FH, g.FW);
  hipStream_t s = (hipStream_t)stream;
  uint32_t* mm = static_cast<uint32_t*>(workspace);
  if (g.norm) {
    FGVC_REQUIRE(hipMemsetAsync(mm, 0, (size_t)n * C * 2 * sizeof(uint32_t), s) == hipSuccess, FGVC_ERR_LAUNCH,
                 "%s: clearing the extremes failed", name);
    const int step = (GD_BLOCK / C) * C;
    const long long total = (long long)Hf * Wf * C;
    const int nb = (int)imax(1, imin(64, (int)((total + 4ll * step - 1) / (4ll * step))));
    guided_extremes_kernel<<<dim3(nb, n), GD_BLOCK, 0, s>>>(labels, Hf * Wf, C, mm);
  }
  const dim3 grid(cdiv(w0, GD_TW), cdiv(h0, GD_TH), n);
  FGVC_REQUIRE(grid.y <= 65535u, FGVC_ERR_UNSUPPORTED, "%s: h0 out of range", name);
  if (with_conf) {
    FGVC_REQUIRE(hipMemsetAsync(stats, 0, (size_t)n * C * 2 * sizeof(int64_t), s) == hipSuccess, FGVC_ERR_LAUNCH,
                 "%s: clearing the statistics failed", name);
    gd_launch<true>(radius, grid, lds, s, labels, guide, cells, mm, g, masks, conf, reinterpret_cast<unsigned long long*>(stats));
  } else {
    gd_launch<false>(radius, grid, lds, s, labels, guide, cells, mm, g, masks, nullptr, nullptr);
  }
  FGVC_CHECK_LAUNCH(name);
  return FGVC_OK;
}

}  // namespace

}  // namespace fgvc

using namespace fgvc;

extern "C" {

int fgvc_guided_channel_chunk(void) { return GD_CH; }
int fgvc_guided_tile_rows(void) { return GD_TH; }
int fgvc_guided_tile_cols(void) { return GD_TW; }

int fgvc_guide_cells_f32(const float* guide, int n, int hp, int wp, int Hf, int Wf, float* cells, void* stream) {
  FGVC_REQUIRE(guide && cells, FGVC_ERR_INVALID_ARG, "fgvc_guide_cells_f32: null pointer");
  FGVC_REQUIRE(n >= 0 && n <= 65535 && Hf > 0 && Hf <= 65535 && Wf > 0 && hp > 0 && wp > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_guide_cells_f32: bad shape (n, Hf <= 65535)");
  FGVC_REQUIRE(hp % Hf == 0 && wp % Wf == 0, FGVC_ERR_INVALID_ARG,
               "fgvc_guide_cells_f32: the feature grid %d x %d does not divide the padded frame %d x %d", Hf, Wf, hp, wp);
  FGVC_REQUIRE(wp <= GD_CELLS_MAX_WP && (long long)n * 3 * hp < (1ll << 31) && (long long)n * Hf * Wf < (1ll << 31), FGVC_ERR_UNSUPPORTED,
               "fgvc_guide_cells_f32: frame size out of range (wp <= %d)", GD_CELLS_MAX_WP);
  if (n == 0) return FGVC_OK;
  guide_cells_kernel<<<dim3(Hf, n), GD_BLOCK, (size_t)3 * wp * sizeof(float), (hipStream_t)stream>>>(guide, hp, wp, Hf, Wf, cells);
  FGVC_CHECK_LAUNCH("fgvc_guide_cells_f32");
  return FGVC_OK;
}

size_t fgvc_seg_readout_guided_workspace_bytes(int n, int C) {
  if (n < 0 || C < 1) return 0;
  return (size_t)n * C * 2 * sizeof(uint32_t);
}

int fgvc_seg_readout_guided_u8(const float* labels, const float* guide, const float* cells, int n, int Hf, int Wf, int C, int hp, int wp,
                               int top, int left, int h, int w, int h0, int w0, int norm, int radius, double sigma_space,
                               double sigma_range, uint8_t* masks, void* workspace, void* stream) {
  return gd_readout("fgvc_seg_readout_guided_u8", false, labels, guide, cells, n, Hf, Wf, C, hp, wp, top, left, h, w, h0, w0, norm, radius,
                    sigma_space, sigma_range, masks, nullptr, nullptr, workspace, stream);
}

int fgvc_seg_readout_guided_conf_u8(const float* labels, const float* guide, const float* cells, int n, int Hf, int Wf, int C, int hp,
                                    int wp, int top, int left, int h, int w, int h0, int w0, int norm, int radius, double sigma_space,
                                    double sigma_range, uint8_t* masks, uint8_t* conf, int64_t* stats, void* workspace, void* stream) {
  return gd_readout("fgvc_seg_readout_guided_conf_u8", true, labels, guide, cells, n, Hf, Wf, C, hp, wp, top, left, h, w, h0, w0, norm,
                    radius, sigma_space, sigma_range, masks, conf, stats, workspace, stream);
}

}  // extern "C"
