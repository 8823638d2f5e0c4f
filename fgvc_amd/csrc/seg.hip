// Segmentation-mask ends of the label-propagation path (semi-supervised VOS, vanilla_tracker.py:663-830): first-frame index map ->
// one-hot labels on the feature grid, hard propagation (argmax -> one-hot of a bank row), and the read-out of C-channel logits to a
// full-resolution index mask.  The middle of the path (pair top-k, merge, fgvc_propagate_topk_f32) is the points path's, with P = C.
#include "common.hpp"

namespace fgvc {

namespace {

// Pillow's NEAREST resize (ImagingScaleAffine, Geometry.c): the source coordinate of output o is a running double sum
// a/2 + a + ... + a with a = in/out, truncated.  The running sum is not floor((o + 0.5) * in / out): at sizes such as 100 -> 27 the
// two differ where the exact value is an integer.  Sequential by construction, so one lane builds each table.
__device__ void pil_nearest_table(int n_in, int n_out, int* __restrict__ tab) {
  const double a = (double)n_in / (double)n_out;
  double xo = a * 0.5;
  for (int o = 0; o < n_out; ++o) {
    const int xi = (int)xo;
    tab[o] = xi < n_in - 1 ? xi : n_in - 1;
    xo += a;
  }
}

// PyTorch area_pixel_compute_source_index (align_corners=False) in f32, as the points read-out evaluates it (post.hip src_index)
__device__ __forceinline__ void seg_src_index(int d, float scale, int in_size, int& i0, int& i1, float& l1) {
  float s = scale * ((float)d + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = imin((int)s, in_size - 1);
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// Taps of one output coordinate through bilinear(in -> padded size), crop at `off`, bilinear(unpadded -> out): feature-grid
// indices t[0..3] and weights w[0..3].  COMPOSED = false: the second resize is the identity (out size == unpadded size), t[2..3]
// and w[2..3] are unused.
template <bool COMPOSED>
struct Taps {
  int t[4];
  float w[4];
  __device__ __forceinline__ void make(int o, float s2, int n_unpad, int off, float s1, int n_feat) {
    int a0, a1, f0, f1;
    float la, lf;
    if constexpr (COMPOSED) {
      seg_src_index(o, s2, n_unpad, a0, a1, la);
      seg_src_index(a0 + off, s1, n_feat, f0, f1, lf);
      t[0] = f0; t[1] = f1; w[0] = (1.f - la) * (1.f - lf); w[1] = (1.f - la) * lf;
      seg_src_index(a1 + off, s1, n_feat, f0, f1, lf);
      t[2] = f0; t[3] = f1; w[2] = la * (1.f - lf); w[3] = la * lf;
    } else {
      seg_src_index(o + off, s1, n_feat, f0, f1, lf);
      t[0] = f0; t[1] = f1; w[0] = 1.f - lf; w[1] = lf;
    }
  }
};

// one pixel of the composed field in channel c: rows y.t (offsets already multiplied by Wf * C), columns x.t (by C)
template <bool COMPOSED>
__device__ __forceinline__ float field_value(const float* __restrict__ lab, const Taps<COMPOSED>& y, const Taps<COMPOSED>& x) {
  constexpr int N = COMPOSED ? 4 : 2;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float row = 0.f;
#pragma unroll
    for (int j = 0; j < N; ++j) row = fmaf(x.w[j], lab[y.t[i] + x.t[j]], row);
    acc = fmaf(y.w[i], row, acc);
  }
  return acc;
}

constexpr int SEG_BLOCK = 256;
constexpr int SEG_PX = 4;                       // output pixels per lane (one 4-byte store)
constexpr int SEG_CHUNK = SEG_BLOCK * SEG_PX;   // pixels per workgroup iteration
constexpr int SEG_NB = 32;                      // phase-1 workgroups per frame (= rows of the partials slab)
// the label kernels' dynamic LDS holds the Hf + Wf source tables (4 B each) beside seg_max_label_kernel's 16 B of static LDS: within 64 KiB
constexpr int SEG_MAX_TABLE = (65536 - 16) / 4;

struct ReadoutGeom {
  int Hf, Wf, C, h, w, h0, w0, top, left;
  float s1y, s1x, s2y, s2x;  // feature / padded and unpadded / output scales
};

// the taps of one lane's SEG_PX pixels starting at p (pixels past HW get clamped coordinates: their values are never used)
template <bool COMPOSED>
__device__ __forceinline__ void lane_taps(const ReadoutGeom& g, int p, int HW, Taps<COMPOSED> (&ty)[SEG_PX],
                                          Taps<COMPOSED> (&tx)[SEG_PX]) {
#pragma unroll
  for (int k = 0; k < SEG_PX; ++k) {
    const int q = imin(p + k, HW - 1);
    const int oy = q / g.w0, ox = q - oy * g.w0;
    ty[k].make(oy, g.s2y, g.h, g.top, g.s1y, g.Hf);
    tx[k].make(ox, g.s2x, g.w, g.left, g.s1x, g.Wf);
#pragma unroll
    for (int i = 0; i < (COMPOSED ? 4 : 2); ++i) {   // Taps<false>::make fills t[0..1] only
      ty[k].t[i] *= g.Wf * g.C;
      tx[k].t[i] *= g.C;
    }
  }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace

// ------------------------------------------------------------------------------------------
// frame-0 labels: Pillow-nearest sample of the padded index map to (Hf, Wf), then one-hot with C channels
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_max_label_kernel(const uint8_t* __restrict__ map, int hp, int wp, int Hf, int Wf,
                                                            int32_t* __restrict__ out) {
  extern __shared__ int tab[];  // [Hf] rows | [Wf] columns
  __shared__ int wmax[4];
  int* ry = tab;
  int* rx = tab + Hf;
  if (threadIdx.x == 0) pil_nearest_table(hp, Hf, ry);
  if (threadIdx.x == 64) pil_nearest_table(wp, Wf, rx);
  __syncthreads();
  int m = 0;
  for (int i = threadIdx.x; i < Hf * Wf; i += 256) {
    const int y = i / Wf, x = i - y * Wf;
    m = max(m, (int)map[(size_t)ry[y] * wp + rx[x]]);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

__global__ __launch_bounds__(256) void seg_onehot_kernel(const uint8_t* __restrict__ map, int hp, int wp, int Hf, int Wf, int C,
                                                         float* __restrict__ out) {
  extern __shared__ int tab[];
  int* ry = tab;
  int* rx = tab + Hf;
  if (threadIdx.x == 0) pil_nearest_table(hp, Hf, ry);
  if (threadIdx.x == 64) pil_nearest_table(wp, Wf, rx);
  __syncthreads();
  const long long n = (long long)Hf * Wf * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int pix = (int)(i / C), c = (int)(i - (long long)pix * C);
    const int y = pix / Wf, x = pix - y * Wf;
    out[i] = (int)map[(size_t)ry[y] * wp + rx[x]] == c ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// annotations at any frame: the 256-bit presence set of a map sampled to the feature grid (bit id of word id / 32), and the injection of
// the cells whose sampled id is in a given set into a (HfWf, C) row block, in place
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_label_set_kernel(const uint8_t* __restrict__ map, int hp, int wp, int Hf, int Wf,
                                                            uint32_t* __restrict__ out) {
  extern __shared__ int tab[];  // [Hf] rows | [Wf] columns
  __shared__ uint32_t bits[8];
  int* ry = tab;
  int* rx = tab + Hf;
  if (threadIdx.x == 0) pil_nearest_table(hp, Hf, ry);
  if (threadIdx.x == 64) pil_nearest_table(wp, Wf, rx);
  if (threadIdx.x >= 128 && threadIdx.x < 136) bits[threadIdx.x - 128] = 0u;
  __syncthreads();
  for (int i = threadIdx.x; i < Hf * Wf; i += 256) {
    const int y = i / Wf, x = i - y * Wf;
    const uint32_t id = map[(size_t)ry[y] * wp + rx[x]];
    const uint32_t bit = 1u << (id & 31);
    if (!(bits[id >> 5] & bit)) atomicOr(&bits[id >> 5], bit);
  }
  __syncthreads();
  if (threadIdx.x < 8) out[threadIdx.x] = bits[threadIdx.x];
}

// rows [Hf*Wf][C]: a cell whose sampled id is in `set` becomes one_hot(id, C) (an id >= C: a zero row, as seg_onehot_kernel); every
// other cell is left alone
__global__ __launch_bounds__(256) void seg_inject_kernel(const uint8_t* __restrict__ map, int hp, int wp, int Hf, int Wf, int C,
                                                         const uint32_t* __restrict__ set, float* __restrict__ rows) {
  extern __shared__ int tab[];
  __shared__ uint32_t bits[8];
  int* ry = tab;
  int* rx = tab + Hf;
  if (threadIdx.x == 0) pil_nearest_table(hp, Hf, ry);
  if (threadIdx.x == 64) pil_nearest_table(wp, Wf, rx);
  if (threadIdx.x >= 128 && threadIdx.x < 136) bits[threadIdx.x - 128] = set[threadIdx.x - 128];
  __syncthreads();
  const long long n = (long long)Hf * Wf * C;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int pix = (int)(i / C), c = (int)(i - (long long)pix * C);
    const int y = pix / Wf, x = pix - y * Wf;
    const int id = (int)map[(size_t)ry[y] * wp + rx[x]];
    if ((bits[id >> 5] >> (id & 31)) & 1u) rows[i] = id == c ? 1.f : 0.f;
  }
}

// ------------------------------------------------------------------------------------------
// hard propagation: row r of `in` (rows, C) -> one_hot(argmax) in `out` (may alias `in`); the first maximum wins
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void seg_hard_onehot_kernel(const float* in, int rows, int C, float* out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float* src = in + (size_t)r * C;
  float best = src[0];
  int bi = 0;
  for (int c = 1; c < C; ++c) {
    const float v = src[c];
    if (v > best) { best = v; bi = c; }
  }
  float* dst = out + (size_t)r * C;
  for (int c = 0; c < C; ++c) dst[c] = c == bi ? 1.f : 0.f;
}

// ------------------------------------------------------------------------------------------
// read-out phase 1: per (frame, channel) min / max of the composed field over the whole output frame.
// Grid (SEG_NB, n): each workgroup strides over the frame's pixel chunks; per channel the lanes reduce their SEG_PX values, the
// wave reduces with shuffles and lane 0 folds it into its wave's LDS slot; the workgroup's partial goes to row blockIdx.x of the
// slab part[n][SEG_NB][C][2] (no atomics: deterministic, and no buffer to clear first).
// ------------------------------------------------------------------------------------------
template <bool COMPOSED>
__global__ __launch_bounds__(SEG_BLOCK) void seg_minmax_kernel(const float* __restrict__ labels, ReadoutGeom g,
                                                               float* __restrict__ part) {
  extern __shared__ float red[];  // [4 waves][C][2]
  const int f = blockIdx.y, C = g.C, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int HW = g.h0 * g.w0;
  const float* lab = labels + (size_t)f * g.Hf * g.Wf * C;
  for (int i = threadIdx.x; i < 4 * C; i += SEG_BLOCK) {
    red[2 * i] = INFINITY;
    red[2 * i + 1] = -INFINITY;
  }
  __syncthreads();
  for (int p0 = blockIdx.x * SEG_CHUNK; p0 < HW; p0 += SEG_NB * SEG_CHUNK) {
    const int p = p0 + threadIdx.x * SEG_PX;
    Taps<COMPOSED> ty[SEG_PX], tx[SEG_PX];
    lane_taps<COMPOSED>(g, p, HW, ty, tx);
    const int nvalid = imin(SEG_PX, HW - p);   // may be <= 0 for the last chunk's tail lanes
    for (int c = 0; c < C; ++c) {
      float mn = INFINITY, mx = -INFINITY;
#pragma unroll
      for (int k = 0; k < SEG_PX; ++k) {
        const float v = field_value<COMPOSED>(lab + c, ty[k], tx[k]);
        if (k < nvalid) {
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
        }
      }
      mn = wave_min(mn);
      mx = wave_max(mx);
      if (lane == 0) {
        float* s = red + 2 * (wave * C + c);
        s[0] = fminf(s[0], mn);
        s[1] = fmaxf(s[1], mx);
      }
    }
  }
  __syncthreads();
  float* dst = part + ((size_t)f * SEG_NB + blockIdx.x) * C * 2;
  for (int c = threadIdx.x; c < C; c += SEG_BLOCK) {
    float mn = red[2 * c], mx = red[2 * c + 1];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      mn = fminf(mn, red[2 * (w * C + c)]);
      mx = fmaxf(mx, red[2 * (w * C + c) + 1]);
    }
    dst[2 * c] = mn;
    dst[2 * c + 1] = mx;
  }
}

// read-out phase 2 (seg_argmax_body.inc): fold the slab into per-channel (min, max) in LDS, then per pixel normalise, argmax (first
// maximum wins) and store SEG_PX index bytes per lane in one 4-byte store where the destination is aligned.
// seg_readout_conf_kernel is the same body with CONF: the runner-up value rides along in a second register per pixel, conf = rint(255 *
// clamp(best - second, 0, 1)) goes out as a second byte plane (C == 1: second stays -inf, the byte is 255), each pixel adds (1, conf) to
// its winner's slot of the LDS counters cnt[C] | sum[C] behind mm, and the workgroup adds its non-zero slots to stats [n][C][2] (zero on
// entry) with 64-bit integer atomics: integer sums, so the result does not depend on the order.
struct SegConfOut {
  uint8_t* conf;
  unsigned long long* stats;
};

template <bool COMPOSED>
__global__ __launch_bounds__(SEG_BLOCK) void seg_argmax_kernel(const float* __restrict__ labels, ReadoutGeom g,
                                                               const float* __restrict__ part, int norm,
                                                               uint8_t* __restrict__ masks) {
  constexpr bool CONF = false;
  [[maybe_unused]] const SegConfOut extra{nullptr, nullptr};
#include "seg_argmax_body.inc"
}

template <bool COMPOSED>
__global__ __launch_bounds__(SEG_BLOCK) void seg_readout_conf_kernel(const float* __restrict__ labels, ReadoutGeom g,
                                                                     const float* __restrict__ part, int norm,
                                                                     uint8_t* __restrict__ masks, SegConfOut extra) {
  constexpr bool CONF = true;
#include "seg_argmax_body.inc"
}

size_t seg_readout_workspace_bytes(int n, int C) { return (size_t)n * SEG_NB * C * 2 * sizeof(float); }

// ------------------------------------------------------------------------------------------
// Soft first-frame labels (the JHMDB / BADJA heat-map form, vanilla_tracker.py:700-716 with a 4-D map) and their read-out to joint
// coordinates (img2coord, :172-191, :814-818).  The map (K, hm, wm) is padded by its own pad_divide_by to (hp, wp) with the content at
// (top, left); the padding is applied implicitly (zeros), no padded copy exists.
// ------------------------------------------------------------------------------------------
namespace {

__device__ __forceinline__ float fma_t(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_t(double a, double b, double c) { return __builtin_fma(a, b, c); }

// bilinear (align_corners=False) of the zero-padded map at output pixel (oy, ox), in the map's dtype T as F.interpolate computes it
// (area_pixel_compute_scale / _source_index in accscalar_t = T; the padded grid is the interpolation's input).
// The rounding sequence is part of the source: every kernel that calls this (bank row 0, the coordinate read-out's frame 0, the map
// read-out's frame 0) must produce the same bits for the same pixel, and with contraction left to the compiler each instance fused
// a * b + c differently.  Contraction is off in this body and the fused operations are written out: the source coordinate and each
// of the three interpolations are one multiply and one fma.
template <typename T>
__device__ __forceinline__ T padded_bilinear(const T* __restrict__ m, int hm, int wm, int top, int left, int hp, int wp, T sy, T sx,
                                             int oy, int ox) {
#pragma clang fp contract(off)
  T ry = fma_t(sy, (T)oy + (T)0.5, (T)-0.5), rx = fma_t(sx, (T)ox + (T)0.5, (T)-0.5);
  ry = ry < (T)0 ? (T)0 : ry;
  rx = rx < (T)0 ? (T)0 : rx;
  const int y0 = imin((int)ry, hp - 1), x0 = imin((int)rx, wp - 1);
  const int y1 = y0 + (y0 < hp - 1 ? 1 : 0), x1 = x0 + (x0 < wp - 1 ? 1 : 0);
  const T ly = ry - (T)y0, lx = rx - (T)x0;
  const T hy = (T)1 - ly, hx = (T)1 - lx;
  auto at = [&](int y, int x) -> T {
    const int yy = y - top, xx = x - left;
    return (yy >= 0 && yy < hm && xx >= 0 && xx < wm) ? m[(size_t)yy * wm + xx] : (T)0;
  };
  const T r0 = fma_t(hx, at(y0, x0), lx * at(y0, x1));
  const T r1 = fma_t(hx, at(y1, x0), lx * at(y1, x1));
  return fma_t(hy, r0, ly * r1);
}

// top-5 of a band: value descending, the higher flat index first among equal values (post.hip TopKHi, np.argsort's tail)
constexpr int HM_K = 5;
constexpr int HM_BLOCK = 256;
constexpr int HM_BANDS = 8;

struct Top5 {
  double v[HM_K];
  int ix[HM_K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < HM_K; ++j) {
      v[j] = -INFINITY;
      ix[j] = -1;
    }
  }
  __device__ __forceinline__ bool accepts(double s, int id) const {
    return s > v[HM_K - 1] || (s == v[HM_K - 1] && id > ix[HM_K - 1]);
  }
  __device__ __forceinline__ void insert(double s, int id) {
#pragma unroll
    for (int j = 0; j < HM_K; ++j) {
      const bool b = s > v[j] || (s == v[j] && id > ix[j]);
      const double tv = v[j];
      const int ti = ix[j];
      v[j] = b ? s : tv;
      ix[j] = b ? id : ti;
      s = b ? tv : s;
      id = b ? ti : id;
    }
  }
};

struct HeatGeom {
  int K, Hf, Wf, hm, wm, hp, wp, top, left, h0, w0, nbands;
  float s1y, s1x, s2y, s2x;   // the composed taps' scales, as ReadoutGeom's
};

// the workgroup's candidates and partial sum -> slot (map, band) of the partials: a tree over the LDS lists, then thread 0 stores
__device__ __forceinline__ void band_reduce_store(Top5& top, double sum, size_t o, double* __restrict__ part_v,
                                                  int* __restrict__ part_i, double* __restrict__ part_sum) {
  __shared__ double sv[HM_BLOCK * HM_K];
  __shared__ int si[HM_BLOCK * HM_K];
  __shared__ double ssum[HM_BLOCK];
  const int tid = threadIdx.x;
#pragma unroll
  for (int j = 0; j < HM_K; ++j) {
    sv[tid * HM_K + j] = top.v[j];
    si[tid * HM_K + j] = top.ix[j];
  }
  ssum[tid] = sum;
  __syncthreads();
  for (int stride = HM_BLOCK / 2; stride >= 1; stride >>= 1) {
    if (tid < stride) {
#pragma unroll
      for (int j = 0; j < HM_K; ++j) {
        const double v = sv[(tid + stride) * HM_K + j];
        const int id = si[(tid + stride) * HM_K + j];
        if (id >= 0 && top.accepts(v, id)) top.insert(v, id);
      }
#pragma unroll
      for (int j = 0; j < HM_K; ++j) {
        sv[tid * HM_K + j] = top.v[j];
        si[tid * HM_K + j] = top.ix[j];
      }
      ssum[tid] += ssum[tid + stride];
    }
    __syncthreads();
  }
  if (tid == 0) {
#pragma unroll
    for (int j = 0; j < HM_K; ++j) {
      part_v[o * HM_K + j] = top.v[j];
      part_i[o * HM_K + j] = top.ix[j];
    }
    part_sum[o] = ssum[0];
  }
}

}  // namespace

// bank row 0: bilinear(padded map -> (Hf, Wf)) in the map's dtype, rounded once to f32; out [Hf*Wf][K], one thread per value
template <typename T>
__global__ __launch_bounds__(256) void seg_soft_labels_kernel(const T* __restrict__ map, int K, int hm, int wm, int hp, int wp, int top,
                                                              int left, int Hf, int Wf, float* __restrict__ out) {
  const T sy = (T)hp / (T)Hf, sx = (T)wp / (T)Wf;
  const long long n = (long long)Hf * Wf * K;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int pix = (int)(i / K), k = (int)(i - (long long)pix * K);
    const int y = pix / Wf, x = pix - y * Wf;
    out[i] = (float)padded_bilinear<T>(map + (size_t)k * hm * wm, hm, wm, top, left, hp, wp, sy, sx, y, x);
  }
}

// Read-out stage 1, frames >= 1: one workgroup per (joint, frame, row band) scans the composed field (fgvc_seg_readout_u8's Taps /
// field_value, unchanged) over its rows, one pixel per lane per step: a top-5 list and the band's sum (f64, lane-strided then a tree).
template <bool COMPOSED>
__global__ __launch_bounds__(HM_BLOCK) void heatmap_band_kernel(const float* __restrict__ bank, HeatGeom g, double* __restrict__ part_v,
                                                                int* __restrict__ part_i, double* __restrict__ part_sum) {
  const int k = blockIdx.x, f = blockIdx.y + 1, band = blockIdx.z;
  const float* lab = bank + (size_t)f * g.Hf * g.Wf * g.K + k;
  const int rows = cdiv(g.h0, g.nbands);
  const int y_lo = band * rows, y_hi = imin(g.h0, y_lo + rows);
  Top5 top;
  top.init();
  double sum = 0.0;
  for (int y = y_lo; y < y_hi; ++y) {
    Taps<COMPOSED> ty;
    ty.make(y, g.s2y, g.hm, g.top, g.s1y, g.Hf);
#pragma unroll
    for (int i = 0; i < (COMPOSED ? 4 : 2); ++i) ty.t[i] *= g.Wf * g.K;
    for (int x = threadIdx.x; x < g.w0; x += HM_BLOCK) {
      Taps<COMPOSED> tx;
      tx.make(x, g.s2x, g.wm, g.left, g.s1x, g.Wf);
#pragma unroll
      for (int i = 0; i < (COMPOSED ? 4 : 2); ++i) tx.t[i] *= g.K;
      const double v = (double)field_value<COMPOSED>(lab, ty, tx);
      const int id = y * g.w0 + x;
      sum += v;
      if (top.accepts(v, id)) top.insert(v, id);
    }
  }
  band_reduce_store(top, sum, ((size_t)f * g.K + k) * g.nbands + band, part_v, part_i, part_sum);
}

// Read-out stage 1, frame 0: bilinear of the zero-padded input map straight to (h0, w0) in its own dtype -- no crop (:712-716)
template <typename T>
__global__ __launch_bounds__(HM_BLOCK) void heatmap_band0_kernel(const T* __restrict__ map, HeatGeom g, double* __restrict__ part_v,
                                                                 int* __restrict__ part_i, double* __restrict__ part_sum) {
  const int k = blockIdx.x, band = blockIdx.z;
  const T* m = map + (size_t)k * g.hm * g.wm;
  const T sy = (T)g.hp / (T)g.h0, sx = (T)g.wp / (T)g.w0;
  const int rows = cdiv(g.h0, g.nbands);
  const int y_lo = band * rows, y_hi = imin(g.h0, y_lo + rows);
  Top5 top;
  top.init();
  double sum = 0.0;
  for (int y = y_lo; y < y_hi; ++y)
    for (int x = threadIdx.x; x < g.w0; x += HM_BLOCK) {
      const double v = (double)padded_bilinear<T>(m, g.hm, g.wm, g.top, g.left, g.hp, g.wp, sy, sx, y, x);
      const int id = y * g.w0 + x;
      sum += v;
      if (top.accepts(v, id)) top.insert(v, id);
    }
  band_reduce_store(top, sum, (size_t)k * g.nbands + band, part_v, part_i, part_sum);
}

// Read-out stage 2: one thread per (frame, joint) map merges its bands and writes x to coords[0][k][f], y to coords[1][k][f].
// f64 != 0: img2coord on a float64 stack (the map was float64): top-5 normalisation in f64.  Else every value is an f32 and the
// normalisation is f32, as post.hip's merge.  Sums in the ascending order of np.sum over argsort[-5:].
// (heatmap_merge_body.inc: shared with heatmap_peak_merge_kernel, which also stores every map's largest value)
__global__ __launch_bounds__(64) void heatmap_merge_kernel(const double* __restrict__ part_v, const int* __restrict__ part_i,
                                                           const double* __restrict__ part_sum, int nbands, int K, int T, int w0, int f64,
                                                           double* __restrict__ coords) {
  constexpr bool PEAK = false;
  [[maybe_unused]] double* const peak = nullptr;
#include "heatmap_merge_body.inc"
}

__global__ __launch_bounds__(64) void heatmap_peak_merge_kernel(const double* __restrict__ part_v, const int* __restrict__ part_i,
                                                                const double* __restrict__ part_sum, int nbands, int K, int T, int w0,
                                                                int f64, double* __restrict__ coords, double* __restrict__ peak) {
  constexpr bool PEAK = true;
#include "heatmap_merge_body.inc"
}

size_t heatmap_workspace_bytes(int T, int K) {
  return (size_t)T * K * HM_BANDS * (HM_K * sizeof(double) + HM_K * sizeof(int) + sizeof(double));
}

// ------------------------------------------------------------------------------------------
// The propagated soft maps themselves (coords=False with a 4-D map, :770-784, :803): the field the coordinate read-out scans, written
// channel-first.  A transpose: the bank is channel-last, the output has w0 contiguous.  A workgroup owns SM_TY rows x SM_TX columns of
// one frame for a group of up to SM_KG channels.  It stages the feature-grid footprint of that tile in LDS, one plane per channel
// ([kg][rows][cols], plane stride odd), from channel-contiguous loads (16 B where K, the group and the pointer allow it); then lane
// (q, cl) evaluates 4 consecutive x (quad q of the tile's 16) of one (row, channel) per step, cl-strided over the tile's rows x channels,
// with field_value on its channel's plane: the same taps, weights and fmaf chain as heatmap_band_kernel.  16 lanes write one 256-byte
// run of a row.  A footprint beyond SM_CAP floats (an output much smaller than the feature grid) is read from the bank directly.
// ------------------------------------------------------------------------------------------
namespace {

constexpr int SM_BLOCK = 256;
constexpr int SM_TX = 64;       // tile columns: 16 quads of 4
constexpr int SM_TY = 8;        // tile rows
constexpr int SM_KG = 16;       // channels per group
constexpr int SM_CAP = 6144;    // floats of LDS for the footprint (24 KiB)

// native vectors: one store instruction each (a struct of four floats is split into scalars and merged across the branches below)
typedef float sm_f32x4 __attribute__((ext_vector_type(4)));
typedef float sm_f32x2 __attribute__((ext_vector_type(2)));
typedef double sm_f64x2 __attribute__((ext_vector_type(2)));

// 4 consecutive values at dst (n < 4 at the end of a row): the widest stores the address allows
__device__ __forceinline__ void store_quad(float* __restrict__ dst, const float (&v)[4], int n) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
  if (n == 4 && (a & 15) == 0) {
    *reinterpret_cast<sm_f32x4*>(dst) = sm_f32x4{v[0], v[1], v[2], v[3]};
  } else if (n == 4 && (a & 7) == 0) {
    *reinterpret_cast<sm_f32x2*>(dst) = sm_f32x2{v[0], v[1]};
    *reinterpret_cast<sm_f32x2*>(dst + 2) = sm_f32x2{v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) dst[j] = v[j];
  }
}
__device__ __forceinline__ void store_quad(double* __restrict__ dst, const double (&v)[4], int n) {
  if (n == 4 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    *reinterpret_cast<sm_f64x2*>(dst) = sm_f64x2{v[0], v[1]};
    *reinterpret_cast<sm_f64x2*>(dst + 2) = sm_f64x2{v[2], v[3]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) dst[j] = v[j];
  }
}

}  // namespace

// frames >= 1.  grid (x tiles * y tiles, channel groups, frames); out points at the first of the frames written
template <bool COMPOSED, typename OUT>
__global__ __launch_bounds__(SM_BLOCK) void softmap_kernel(const float* __restrict__ bank, HeatGeom g, int f_first, int xtiles,
                                                           OUT* __restrict__ out) {
  constexpr int N = COMPOSED ? 4 : 2;
  __shared__ __attribute__((aligned(16))) float foot[SM_CAP];
  __shared__ Taps<COMPOSED> sty[SM_TY];
  const int tid = threadIdx.x;
  const int tile_y = blockIdx.x / xtiles, tile_x = blockIdx.x - tile_y * xtiles;
  const int y0 = tile_y * SM_TY, x0 = tile_x * SM_TX;
  const int ny = imin(SM_TY, g.h0 - y0), x_last = imin(x0 + SM_TX, g.w0) - 1;
  const int k0 = blockIdx.y * SM_KG, kg = imin(SM_KG, g.K - k0);
  const int f = f_first + blockIdx.z;
  const float* lab = bank + (size_t)f * g.Hf * g.Wf * g.K + k0;
  // the footprint: seg_src_index is monotone in its output coordinate, so the first tap of the first row / column and the last tap of
  // the last bound every tap of the tile
  Taps<COMPOSED> lo, hi;
  lo.make(y0, g.s2y, g.hm, g.top, g.s1y, g.Hf);
  hi.make(y0 + ny - 1, g.s2y, g.hm, g.top, g.s1y, g.Hf);
  const int fy0 = lo.t[0], nrows = hi.t[N - 1] - fy0 + 1;
  lo.make(x0, g.s2x, g.wm, g.left, g.s1x, g.Wf);
  hi.make(x_last, g.s2x, g.wm, g.left, g.s1x, g.Wf);
  const int fx0 = lo.t[0], ncols = hi.t[N - 1] - fx0 + 1;
  const int plane = (nrows * ncols) | 1;
  const bool staged = plane * kg <= SM_CAP;   // the same in every lane
  if (staged) {
    const int npix = nrows * ncols;
    if ((g.K & 3) == 0 && (kg & 3) == 0 && (reinterpret_cast<uintptr_t>(bank) & 15) == 0) {
      const int c4n = kg >> 2;
      for (int e = tid; e < npix * c4n; e += SM_BLOCK) {
        const int pix = e / c4n, c4 = e - pix * c4n;
        const int r = pix / ncols, c = pix - r * ncols;
        const float4 v = *reinterpret_cast<const float4*>(lab + ((size_t)(fy0 + r) * g.Wf + fx0 + c) * g.K + 4 * c4);
        float* d = foot + (4 * c4) * plane + pix;
        d[0] = v.x; d[plane] = v.y; d[2 * plane] = v.z; d[3 * plane] = v.w;
      }
    } else {
      for (int e = tid; e < npix * kg; e += SM_BLOCK) {
        const int pix = e / kg, c = e - pix * kg;
        const int r = pix / ncols, cc = pix - r * ncols;
        foot[c * plane + pix] = lab[((size_t)(fy0 + r) * g.Wf + fx0 + cc) * g.K + c];
      }
    }
  }
  // row taps of the tile, offsets as field_value wants them: LDS rows of ncols, or bank rows of Wf * K
  if (tid < ny) {
    Taps<COMPOSED> t;
    t.make(y0 + tid, g.s2y, g.hm, g.top, g.s1y, g.Hf);
#pragma unroll
    for (int i = 0; i < N; ++i) t.t[i] = staged ? (t.t[i] - fy0) * ncols : t.t[i] * g.Wf * g.K;
    sty[tid] = t;
  }
  const int q = tid & 15, cl = tid >> 4;
  const int x = x0 + 4 * q;
  Taps<COMPOSED> tx[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    tx[j].make(imin(x + j, g.w0 - 1), g.s2x, g.wm, g.left, g.s1x, g.Wf);
#pragma unroll
    for (int i = 0; i < N; ++i) tx[j].t[i] = staged ? tx[j].t[i] - fx0 : tx[j].t[i] * g.K;
  }
  __syncthreads();
  const int n = imin(4, g.w0 - x);
  if (n <= 0) return;
  OUT* dst_f = out + ((size_t)blockIdx.z * g.K + k0) * g.h0 * g.w0 + x;
  // one call per source so that the staged instance reads LDS with LDS instructions
  auto run = [&](const float* __restrict__ base, int kstride) __attribute__((always_inline)) {
    for (int c = cl; c < ny * kg; c += SM_BLOCK / 16) {
      const int r = c / kg, k = c - r * kg;
      const Taps<COMPOSED> ty = sty[r];
      OUT v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = (OUT)field_value<COMPOSED>(base + k * kstride, ty, tx[j]);
      store_quad(dst_f + ((size_t)k * g.h0 + y0 + r) * g.w0, v, n);
    }
  };
  if (staged)
    run(foot, plane);
  else
    run(lab, 1);
}

// frame 0: bilinear of the zero-padded input map straight to (h0, w0) in its own dtype, then rounded or widened to the output's.
// The value is padded_bilinear's, whose rounding sequence is fixed in its source: the bits heatmap_band0_kernel scans.  The loop is that
// kernel's (rows of a band, one pixel per lane, 256 consecutive x per step), the output dtype a run-time flag: one instance per map
// dtype.  Frame 0 is 1 / T of the stack: dword stores.
// grid (K, 1, nbands): one row per band up to 16384 rows, so that every lane has a few pixels only (the map is gathered through the caches)
constexpr int SM_MAX_BANDS0 = 16384;
template <typename T>
__global__ __launch_bounds__(SM_BLOCK) void softmap0_kernel(const T* __restrict__ map, HeatGeom g, int out_f64, void* __restrict__ out) {
  const int k = blockIdx.x, band = blockIdx.z;
  const T* m = map + (size_t)k * g.hm * g.wm;
  const T sy = (T)g.hp / (T)g.h0, sx = (T)g.wp / (T)g.w0;
  const int rows = cdiv(g.h0, g.nbands);
  const int y_lo = band * rows, y_hi = imin(g.h0, y_lo + rows);
  const size_t base = (size_t)k * g.h0 * g.w0;
  for (int y = y_lo; y < y_hi; ++y)
    for (int x = threadIdx.x; x < g.w0; x += SM_BLOCK) {
      const T v = padded_bilinear<T>(m, g.hm, g.wm, g.top, g.left, g.hp, g.wp, sy, sx, y, x);
      const size_t o = base + (size_t)y * g.w0 + x;
      if (out_f64)
        static_cast<double*>(out)[o] = (double)v;
      else
        static_cast<float*>(out)[o] = (float)v;
    }
}

template <typename OUT>
static void softmap_launch(const float* bank, const void* map0, int map0_f64, const HeatGeom& g, int f_begin, int f_end, OUT* out,
                           hipStream_t s) {
  const size_t frame = (size_t)g.K * g.h0 * g.w0;
  const int xtiles = cdiv(g.w0, SM_TX);
  if (f_begin == 0) {
    const dim3 grid0(g.K, 1, g.nbands);
    const int f64 = sizeof(OUT) == 8;
    if (map0_f64)
      softmap0_kernel<double><<<grid0, SM_BLOCK, 0, s>>>(static_cast<const double*>(map0), g, f64, out);
    else
      softmap0_kernel<float><<<grid0, SM_BLOCK, 0, s>>>(static_cast<const float*>(map0), g, f64, out);
  }
  const int f_first = imax(f_begin, 1);
  if (f_end > f_first) {
    const dim3 grid(xtiles * cdiv(g.h0, SM_TY), cdiv(g.K, SM_KG), f_end - f_first);
    OUT* dst = out + (size_t)(f_first - f_begin) * frame;
    if (g.hm == g.h0 && g.wm == g.w0)
      softmap_kernel<false, OUT><<<grid, SM_BLOCK, 0, s>>>(bank, g, f_first, xtiles, dst);
    else
      softmap_kernel<true, OUT><<<grid, SM_BLOCK, 0, s>>>(bank, g, f_first, xtiles, dst);
  }
}

}  // namespace fgvc

using namespace fgvc;

extern "C" {

int fgvc_seg_max_label_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, int32_t* out, void* stream) {
  FGVC_REQUIRE(map && out, FGVC_ERR_INVALID_ARG, "fgvc_seg_max_label_u8: null pointer");
  FGVC_REQUIRE(hp > 0 && wp > 0 && Hf > 0 && Wf > 0, FGVC_ERR_INVALID_ARG, "fgvc_seg_max_label_u8: bad shape");
  FGVC_REQUIRE(Hf + Wf <= SEG_MAX_TABLE, FGVC_ERR_UNSUPPORTED, "fgvc_seg_max_label_u8: Hf + Wf > %d", SEG_MAX_TABLE);
  seg_max_label_kernel<<<1, 256, (Hf + Wf) * sizeof(int), (hipStream_t)stream>>>(map, hp, wp, Hf, Wf, out);
  FGVC_CHECK_LAUNCH("fgvc_seg_max_label_u8");
  return FGVC_OK;
}

int fgvc_seg_onehot_labels_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, int C, float* out, void* stream) {
  FGVC_REQUIRE(map && out, FGVC_ERR_INVALID_ARG, "fgvc_seg_onehot_labels_u8: null pointer");
  FGVC_REQUIRE(hp > 0 && wp > 0 && Hf > 0 && Wf > 0 && C >= 1 && C <= 256, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_onehot_labels_u8: bad shape (1 <= C <= 256)");
  FGVC_REQUIRE(Hf + Wf <= SEG_MAX_TABLE, FGVC_ERR_UNSUPPORTED, "fgvc_seg_onehot_labels_u8: Hf + Wf > %d", SEG_MAX_TABLE);
  const long long n = (long long)Hf * Wf * C;
  const int blocks = (int)(n < 256ll * 1024 ? (n + 255) / 256 : 1024);
  seg_onehot_kernel<<<blocks, 256, (Hf + Wf) * sizeof(int), (hipStream_t)stream>>>(map, hp, wp, Hf, Wf, C, out);
  FGVC_CHECK_LAUNCH("fgvc_seg_onehot_labels_u8");
  return FGVC_OK;
}

int fgvc_seg_label_set_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, uint32_t* out, void* stream) {
  FGVC_REQUIRE(map && out, FGVC_ERR_INVALID_ARG, "fgvc_seg_label_set_u8: null pointer");
  FGVC_REQUIRE(hp > 0 && wp > 0 && Hf > 0 && Wf > 0, FGVC_ERR_INVALID_ARG, "fgvc_seg_label_set_u8: bad shape");
  FGVC_REQUIRE(Hf + Wf <= SEG_MAX_TABLE - 8 && (long long)Hf * Wf < (1ll << 31), FGVC_ERR_UNSUPPORTED,
               "fgvc_seg_label_set_u8: Hf + Wf > %d", SEG_MAX_TABLE - 8);
  seg_label_set_kernel<<<1, 256, (Hf + Wf) * sizeof(int), (hipStream_t)stream>>>(map, hp, wp, Hf, Wf, out);
  FGVC_CHECK_LAUNCH("fgvc_seg_label_set_u8");
  return FGVC_OK;
}

int fgvc_seg_inject_labels_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, int C, const uint32_t* set, float* rows, void* stream) {
  FGVC_REQUIRE(map && set && rows, FGVC_ERR_INVALID_ARG, "fgvc_seg_inject_labels_u8: null pointer");
  FGVC_REQUIRE(hp > 0 && wp > 0 && Hf > 0 && Wf > 0 && C >= 1 && C <= 256, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_inject_labels_u8: bad shape (1 <= C <= 256)");
  FGVC_REQUIRE(Hf + Wf <= SEG_MAX_TABLE - 8 && (long long)Hf * Wf < (1ll << 31), FGVC_ERR_UNSUPPORTED,
               "fgvc_seg_inject_labels_u8: Hf + Wf > %d", SEG_MAX_TABLE - 8);
  const long long n = (long long)Hf * Wf * C;
  const int blocks = (int)(n < 256ll * 1024 ? (n + 255) / 256 : 1024);
  seg_inject_kernel<<<blocks, 256, (Hf + Wf) * sizeof(int), (hipStream_t)stream>>>(map, hp, wp, Hf, Wf, C, set, rows);
  FGVC_CHECK_LAUNCH("fgvc_seg_inject_labels_u8");
  return FGVC_OK;
}

int fgvc_seg_hard_onehot_f32(const float* in, int rows, int C, float* out, void* stream) {
  FGVC_REQUIRE(in && out, FGVC_ERR_INVALID_ARG, "fgvc_seg_hard_onehot_f32: null pointer");
  FGVC_REQUIRE(rows > 0 && C >= 1, FGVC_ERR_INVALID_ARG, "fgvc_seg_hard_onehot_f32: bad shape");
  seg_hard_onehot_kernel<<<cdiv(rows, 256), 256, 0, (hipStream_t)stream>>>(in, rows, C, out);
  FGVC_CHECK_LAUNCH("fgvc_seg_hard_onehot_f32");
  return FGVC_OK;
}

size_t fgvc_seg_readout_workspace_bytes(int n, int C) {
  if (n < 0 || C < 1) return 0;
  return seg_readout_workspace_bytes(n, C);
}

int fgvc_seg_readout_u8(const float* labels, int n, int Hf, int Wf, int C, int hp, int wp, int top, int left, int h, int w, int h0,
                        int w0, int norm, uint8_t* masks, void* workspace, void* stream) {
  FGVC_REQUIRE(labels && masks, FGVC_ERR_INVALID_ARG, "fgvc_seg_readout_u8: null pointer");
  FGVC_REQUIRE(n >= 0 && n <= 65535 && Hf > 0 && Wf > 0 && C >= 1 && C <= 256 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_readout_u8: bad shape (1 <= C <= 256, n <= 65535)");
  FGVC_REQUIRE(h > 0 && w > 0 && top >= 0 && left >= 0 && top + h <= hp && left + w <= wp, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_readout_u8: the unpadded window must lie inside the padded frame");
  FGVC_REQUIRE((long long)h0 * w0 < (1ll << 31) - SEG_CHUNK, FGVC_ERR_UNSUPPORTED, "fgvc_seg_readout_u8: h0*w0 out of range");
  FGVC_REQUIRE(workspace != nullptr || n == 0, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_readout_u8: workspace of fgvc_seg_readout_workspace_bytes() bytes required");
  if (n == 0) return FGVC_OK;
  ReadoutGeom g;
  g.Hf = Hf; g.Wf = Wf; g.C = C; g.h = h; g.w = w; g.h0 = h0; g.w0 = w0; g.top = top; g.left = left;
  g.s1y = (float)Hf / (float)hp; g.s1x = (float)Wf / (float)wp;
  g.s2y = (float)h / (float)h0; g.s2x = (float)w / (float)w0;
  const bool composed = !(h == h0 && w == w0);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const int HW = h0 * w0;
  const dim3 g1(SEG_NB, n), g2(cdiv(HW, SEG_CHUNK), n);
  if (composed) {
    seg_minmax_kernel<true><<<g1, SEG_BLOCK, 8 * C * sizeof(float), s>>>(labels, g, part);
    seg_argmax_kernel<true><<<g2, SEG_BLOCK, 2 * C * sizeof(float), s>>>(labels, g, part, norm, masks);
  } else {
    seg_minmax_kernel<false><<<g1, SEG_BLOCK, 8 * C * sizeof(float), s>>>(labels, g, part);
    seg_argmax_kernel<false><<<g2, SEG_BLOCK, 2 * C * sizeof(float), s>>>(labels, g, part, norm, masks);
  }
  FGVC_CHECK_LAUNCH("fgvc_seg_readout_u8");
  return FGVC_OK;
}

int fgvc_seg_readout_conf_u8(const float* labels, int n, int Hf, int Wf, int C, int hp, int wp, int top, int left, int h, int w, int h0,
                             int w0, int norm, uint8_t* masks, uint8_t* conf, int64_t* stats, void* workspace, void* stream) {
  FGVC_REQUIRE(labels && masks && conf && stats, FGVC_ERR_INVALID_ARG, "fgvc_seg_readout_conf_u8: null pointer");
  FGVC_REQUIRE(n >= 0 && n <= 65535 && Hf > 0 && Wf > 0 && C >= 1 && C <= 256 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_readout_conf_u8: bad shape (1 <= C <= 256, n <= 65535)");
  FGVC_REQUIRE(h > 0 && w > 0 && top >= 0 && left >= 0 && top + h <= hp && left + w <= wp, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_readout_conf_u8: the unpadded window must lie inside the padded frame");
  FGVC_REQUIRE((long long)h0 * w0 < (1ll << 31) - SEG_CHUNK, FGVC_ERR_UNSUPPORTED, "fgvc_seg_readout_conf_u8: h0*w0 out of range");
  FGVC_REQUIRE(workspace != nullptr || n == 0, FGVC_ERR_INVALID_ARG,
               "fgvc_seg_readout_conf_u8: workspace of fgvc_seg_readout_workspace_bytes() bytes required");
  if (n == 0) return FGVC_OK;
  ReadoutGeom g;
  g.Hf = Hf; g.Wf = Wf; g.C = C; g.h = h; g.w = w; g.h0 = h0; g.w0 = w0; g.top = top; g.left = left;
  g.s1y = (float)Hf / (float)hp; g.s1x = (float)Wf / (float)wp;
  g.s2y = (float)h / (float)h0; g.s2x = (float)w / (float)w0;
  const bool composed = !(h == h0 && w == w0);
  float* part = static_cast<float*>(workspace);
  hipStream_t s = (hipStream_t)stream;
  const int HW = h0 * w0;
  const dim3 g1(SEG_NB, n), g2(cdiv(HW, SEG_CHUNK), n);
  unsigned long long* st = reinterpret_cast<unsigned long long*>(stats);
  FGVC_REQUIRE(hipMemsetAsync(stats, 0, (size_t)n * C * 2 * sizeof(int64_t), s) == hipSuccess, FGVC_ERR_LAUNCH,
               "fgvc_seg_readout_conf_u8: clearing the statistics failed");
  if (composed) {
    seg_minmax_kernel<true><<<g1, SEG_BLOCK, 8 * C * sizeof(float), s>>>(labels, g, part);
    seg_readout_conf_kernel<true><<<g2, SEG_BLOCK, 4 * C * sizeof(float), s>>>(labels, g, part, norm, masks, SegConfOut{conf, st});
  } else {
    seg_minmax_kernel<false><<<g1, SEG_BLOCK, 8 * C * sizeof(float), s>>>(labels, g, part);
    seg_readout_conf_kernel<false><<<g2, SEG_BLOCK, 4 * C * sizeof(float), s>>>(labels, g, part, norm, masks, SegConfOut{conf, st});
  }
  FGVC_CHECK_LAUNCH("fgvc_seg_readout_conf_u8");
  return FGVC_OK;
}

static int soft_labels_check(const void* map, const float* out, int K, int hm, int wm, int hp, int wp, int top, int left, int Hf,
                             int Wf, const char* name) {
  FGVC_REQUIRE(map && out, FGVC_ERR_INVALID_ARG, "%s: null pointer", name);
  FGVC_REQUIRE(K >= 1 && K <= 256 && hm > 0 && wm > 0 && Hf > 0 && Wf > 0, FGVC_ERR_INVALID_ARG, "%s: bad shape (1 <= K <= 256)", name);
  FGVC_REQUIRE(top >= 0 && left >= 0 && top + hm <= hp && left + wm <= wp, FGVC_ERR_INVALID_ARG,
               "%s: the map must lie inside the padded frame", name);
  FGVC_REQUIRE((long long)Hf * Wf * K < (1ll << 40) && (long long)Hf * Wf < (1ll << 31), FGVC_ERR_UNSUPPORTED, "%s: too large", name);
  return FGVC_OK;
}

int fgvc_seg_soft_labels_f32(const float* map, int K, int hm, int wm, int hp, int wp, int top, int left, int Hf, int Wf, float* out,
                             void* stream) {
  const int rc = soft_labels_check(map, out, K, hm, wm, hp, wp, top, left, Hf, Wf, "fgvc_seg_soft_labels_f32");
  if (rc != FGVC_OK) return rc;
  const long long n = (long long)Hf * Wf * K;
  const int blocks = (int)(n < 256ll * 1024 ? (n + 255) / 256 : 1024);
  seg_soft_labels_kernel<float><<<blocks, 256, 0, (hipStream_t)stream>>>(map, K, hm, wm, hp, wp, top, left, Hf, Wf, out);
  FGVC_CHECK_LAUNCH("fgvc_seg_soft_labels_f32");
  return FGVC_OK;
}

int fgvc_seg_soft_labels_f64(const double* map, int K, int hm, int wm, int hp, int wp, int top, int left, int Hf, int Wf, float* out,
                             void* stream) {
  const int rc = soft_labels_check(map, out, K, hm, wm, hp, wp, top, left, Hf, Wf, "fgvc_seg_soft_labels_f64");
  if (rc != FGVC_OK) return rc;
  const long long n = (long long)Hf * Wf * K;
  const int blocks = (int)(n < 256ll * 1024 ? (n + 255) / 256 : 1024);
  seg_soft_labels_kernel<double><<<blocks, 256, 0, (hipStream_t)stream>>>(map, K, hm, wm, hp, wp, top, left, Hf, Wf, out);
  FGVC_CHECK_LAUNCH("fgvc_seg_soft_labels_f64");
  return FGVC_OK;
}

size_t fgvc_heatmap_coords_workspace_bytes(int T, int K) {
  if (T < 0 || K < 1) return 0;
  return heatmap_workspace_bytes(T, K);
}

}  // extern "C"

// fgvc_heatmap_coords_f32 (peak null) and fgvc_heatmap_coords_peak_f32 (`name`: the one called, for its errors): one body, the merge
// kernel with or without the peak's store
static int heatmap_coords_entry(const char* name, const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm,
                                int wm, int hp, int wp, int top, int left, int h0, int w0, int f64_arith, double* coords, double* peak,
                                void* workspace, void* stream) {
  FGVC_REQUIRE(map0 && coords && (bank || T <= 1), FGVC_ERR_INVALID_ARG, "%s: null pointer", name);
  FGVC_REQUIRE(T >= 0 && T <= 65535 && Hf > 0 && Wf > 0 && K >= 1 && K <= 256 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG,
               "%s: bad shape (1 <= K <= 256, T <= 65535)", name);
  FGVC_REQUIRE(hm > 0 && wm > 0 && top >= 0 && left >= 0 && top + hm <= hp && left + wm <= wp, FGVC_ERR_INVALID_ARG,
               "%s: the map must lie inside the padded frame", name);
  FGVC_REQUIRE((long long)h0 * w0 >= HM_K && (long long)h0 * w0 < (1ll << 31), FGVC_ERR_UNSUPPORTED,
               "%s: h0*w0 out of range (5 <= h0*w0 < 2^31)", name);
  FGVC_REQUIRE(workspace != nullptr || T == 0, FGVC_ERR_INVALID_ARG,
               "%s: workspace of fgvc_heatmap_coords_workspace_bytes() bytes required", name);
  if (T == 0) return FGVC_OK;
  HeatGeom g;
  g.K = K; g.Hf = Hf; g.Wf = Wf; g.hm = hm; g.wm = wm; g.hp = hp; g.wp = wp; g.top = top; g.left = left; g.h0 = h0; g.w0 = w0;
  g.nbands = HM_BANDS;
  g.s1y = (float)Hf / (float)hp; g.s1x = (float)Wf / (float)wp;
  g.s2y = (float)hm / (float)h0; g.s2x = (float)wm / (float)w0;
  const size_t maps = (size_t)T * K;
  double* part_v = static_cast<double*>(workspace);
  double* part_sum = part_v + maps * HM_BANDS * HM_K;
  int* part_i = reinterpret_cast<int*>(part_sum + maps * HM_BANDS);
  hipStream_t s = (hipStream_t)stream;
  if (map0_f64)
    heatmap_band0_kernel<double><<<dim3(K, 1, HM_BANDS), HM_BLOCK, 0, s>>>(static_cast<const double*>(map0), g, part_v, part_i, part_sum);
  else
    heatmap_band0_kernel<float><<<dim3(K, 1, HM_BANDS), HM_BLOCK, 0, s>>>(static_cast<const float*>(map0), g, part_v, part_i, part_sum);
  if (T > 1) {
    const dim3 grid(K, T - 1, HM_BANDS);
    if (hm == h0 && wm == w0)
      heatmap_band_kernel<false><<<grid, HM_BLOCK, 0, s>>>(bank, g, part_v, part_i, part_sum);
    else
      heatmap_band_kernel<true><<<grid, HM_BLOCK, 0, s>>>(bank, g, part_v, part_i, part_sum);
  }
  if (peak)
    heatmap_peak_merge_kernel<<<cdiv((int)maps, 64), 64, 0, s>>>(part_v, part_i, part_sum, HM_BANDS, K, T, w0, f64_arith, coords, peak);
  else
    heatmap_merge_kernel<<<cdiv((int)maps, 64), 64, 0, s>>>(part_v, part_i, part_sum, HM_BANDS, K, T, w0, f64_arith, coords);
  FGVC_CHECK_LAUNCH(name);
  return FGVC_OK;
}

extern "C" {

int fgvc_heatmap_coords_f32(const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm, int wm, int hp,
                            int wp, int top, int left, int h0, int w0, int f64_arith, double* coords, void* workspace, void* stream) {
  return heatmap_coords_entry("fgvc_heatmap_coords_f32", bank, map0, map0_f64, T, Hf, Wf, K, hm, wm, hp, wp, top, left, h0, w0, f64_arith, coords,
                              nullptr, workspace, stream);
}

int fgvc_heatmap_coords_peak_f32(const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm, int wm, int hp,
                                 int wp, int top, int left, int h0, int w0, int f64_arith, double* coords, double* peak, void* workspace,
                                 void* stream) {
  FGVC_REQUIRE(peak, FGVC_ERR_INVALID_ARG, "fgvc_heatmap_coords_peak_f32: null pointer");
  return heatmap_coords_entry("fgvc_heatmap_coords_peak_f32", bank, map0, map0_f64, T, Hf, Wf, K, hm, wm, hp, wp, top, left, h0, w0, f64_arith,
                              coords, peak, workspace, stream);
}

int fgvc_softmap_readout_f32(const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm, int wm, int hp,
                             int wp, int top, int left, int h0, int w0, int f_begin, int f_end, int out_f64, void* out, void* stream) {
  FGVC_REQUIRE(map0 && out && (bank || f_end <= 1), FGVC_ERR_INVALID_ARG, "fgvc_softmap_readout_f32: null pointer");
  FGVC_REQUIRE(T >= 1 && T <= 65535 && Hf > 0 && Wf > 0 && K >= 1 && K <= 256 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_softmap_readout_f32: bad shape (1 <= K <= 256, 1 <= T <= 65535)");
  FGVC_REQUIRE(0 <= f_begin && f_begin < f_end && f_end <= T, FGVC_ERR_INVALID_ARG,
               "fgvc_softmap_readout_f32: bad frame range [%d, %d) of %d frames (0 <= f_begin < f_end <= T)", f_begin, f_end, T);
  FGVC_REQUIRE(hm > 0 && wm > 0 && top >= 0 && left >= 0 && top + hm <= hp && left + wm <= wp, FGVC_ERR_INVALID_ARG,
               "fgvc_softmap_readout_f32: the map must lie inside the padded frame");
  FGVC_REQUIRE((long long)h0 * w0 < (1ll << 31) && (long long)Hf * Wf * K < (1ll << 31) &&
                   (long long)cdiv(w0, SM_TX) * cdiv(h0, SM_TY) < (1ll << 31),
               FGVC_ERR_UNSUPPORTED, "fgvc_softmap_readout_f32: h0*w0 or Hf*Wf*K out of range (< 2^31)");
  HeatGeom g;
  g.K = K; g.Hf = Hf; g.Wf = Wf; g.hm = hm; g.wm = wm; g.hp = hp; g.wp = wp; g.top = top; g.left = left; g.h0 = h0; g.w0 = w0;
  g.nbands = imin(h0, SM_MAX_BANDS0);   // frame 0's row bands
  g.s1y = (float)Hf / (float)hp; g.s1x = (float)Wf / (float)wp;
  g.s2y = (float)hm / (float)h0; g.s2x = (float)wm / (float)w0;
  if (out_f64)
    softmap_launch<double>(bank, map0, map0_f64, g, f_begin, f_end, static_cast<double*>(out), (hipStream_t)stream);
  else
    softmap_launch<float>(bank, map0, map0_f64, g, f_begin, f_end, static_cast<float*>(out), (hipStream_t)stream);
  FGVC_CHECK_LAUNCH("fgvc_softmap_readout_f32");
  return FGVC_OK;
}

}  // extern "C"
