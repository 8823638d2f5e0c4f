// DAVIS J&F on the device: the six integer pixel counts that metrics.db_eval_iou and metrics.f_measure divide,
// per (frame, object), from the two id maps themselves.
//   * a workgroup owns JF_TILE rows x JF_XW 64-pixel words of one (frame, object).  It turns that tile plus a halo of `radius` rows and one
//     word on either side into two BIT maps in LDS -- b(G) and b(S), metrics._seg2bmap of (gt == o) and (pred == o) -- one __ballot per 64
//     pixels of a row (lane i = bit i = column 64 j + i), and counts |G & S|, |G | S|, |b(S)|, |b(G)| of its own tile on the way;
//   * the disk is a chord per row offset dy: half-width wx(dy) = floor(sqrt(r^2 - dy^2)).  dil(B) at a word = OR over dy of the row word
//     smeared by 0 .. wx(dy) bits to either side, its two neighbour words shifted in (radius <= 64: one word reaches).  The smear is a
//     doubling chain of shift-ORs on 128-bit values.  Bits never cross a row's end: the words left of column 0 and right of the last one
//     are zero, and so are the bits past the width in the last word.  A thread owns one word and skips it when it holds no boundary bit;
//   * the workgroup's six partial counts go through LDS integer atomics into one 64-bit integer atomic each (the launch clears `counts`
//     first): integer sums, the same in any order.
// The id maps are read once per object from global memory (a frame pair of 480p is 0.8 MB: the cache serves the passes after the first).
#include "common.hpp"

namespace fgvc {

namespace {

constexpr int JF_TILE = 32;          // rows per workgroup (exported as fgvc_jf_tile_rows(): the tests put edges on its multiples)
constexpr int JF_XW = 16;            // 64-pixel words per workgroup: 1024 columns
constexpr int JF_BLOCK = 256;
constexpr int JF_MAX_RADIUS = 64;    // one halo word on either side

typedef unsigned long long u64;
typedef unsigned __int128 u128;

struct JfArgs {
  const uint8_t* gt;
  const uint8_t* pred;
  u64* counts;
  int t0, h, w, n_objects, radius, xtiles;
};

// OR of v << s (v >> s) for s = 0 .. k, 0 <= k <= 64
__device__ __forceinline__ u128 smear_up(u128 v, int k) {
  int m = 1;
  for (; 2 * m <= k + 1; m *= 2) v |= v << m;
  return v | (v << (k + 1 - m));
}
__device__ __forceinline__ u128 smear_down(u128 v, int k) {
  int m = 1;
  for (; 2 * m <= k + 1; m *= 2) v |= v >> m;
  return v | (v >> (k + 1 - m));
}

// the centre word of (left, centre, right) dilated by k bits along the row; bit i = column i, so "up" moves towards higher columns
__device__ __forceinline__ u64 dilate_row_word(u64 left, u64 centre, u64 right, int k) {
  const u128 lo = ((u128)centre << 64) | left, hi = ((u128)right << 64) | centre;
  return (u64)(smear_up(lo, k) >> 64) | (u64)smear_down(hi, k);
}

// metrics._seg2bmap at one pixel: s, and its east / south / south-east neighbours (false outside the image)
__device__ __forceinline__ bool boundary_bit(bool s, bool e, bool so, bool se, bool has_east, bool has_south) {
  if (has_south) return has_east ? ((s != e) | (s != so) | (s != se)) : (s != so);     // last column: south only
  return has_east ? (s != e) : false;                                                 // last row: east only; the corner: never
}

}  // namespace

__global__ __launch_bounds__(JF_BLOCK) void jf_counts_kernel(const JfArgs a) {
  extern __shared__ u64 jf_bits[];                                    // b(G) then b(S): [JF_TILE + 2 r][JF_XW + 2] words each
  __shared__ unsigned acc[6];
  __shared__ int chord[JF_MAX_RADIUS + 1];
  const int r = a.radius, tid = threadIdx.x;
  const int rows = JF_TILE + 2 * r;
  constexpr int words = JF_XW + 2;
  u64* bG = jf_bits;
  u64* bS = jf_bits + rows * words;
  const int band = blockIdx.x / a.xtiles, xt = blockIdx.x % a.xtiles;
  const int o = blockIdx.y + 1, t = a.t0 + blockIdx.z;
  const int y0 = band * JF_TILE, j0 = xt * JF_XW;
  const int W64 = cdiv(a.w, 64);
  if (tid < 6) acc[tid] = 0;
  if (tid <= r) {                                                     // the largest k with k^2 + d^2 <= r^2
    const int d = tid, q = r * r - d * d;
    int k = (int)sqrtf((float)q);
    while (k * k > q) --k;
    while ((k + 1) * (k + 1) <= q) ++k;
    chord[d] = k;
  }

  // ---- the two boundary bit maps of tile + halo, and the tile's region and boundary counts ----
  const int lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const size_t frame = (size_t)t * a.h * a.w;
  const uint8_t* G = a.gt + frame;
  const uint8_t* S = a.pred + frame;
  unsigned n_and = 0, n_or = 0, n_bs = 0, n_bg = 0;                   // the same in every lane of a wave
  for (int it = wave; it < rows * words; it += JF_BLOCK / WAVE) {
    const int ry = it / words, rj = it % words;
    const int y = y0 - r + ry, j = j0 - 1 + rj;
    u64 wg = 0, ws = 0;
    if (y >= 0 && y < a.h && j >= 0 && j < W64) {
      const int x = j * 64 + lane;
      bool g = false, s = false, bg = false, bs = false;
      if (x < a.w) {
        const bool he = x + 1 < a.w, hs = y + 1 < a.h;
        const size_t p = (size_t)y * a.w + x;
        const int e = he ? 1 : 0, so = hs ? a.w : 0;                  // (a missing neighbour: the pixel itself is read, and not used)
        const uint8_t g0 = G[p], g1 = G[p + e], g2 = G[p + so], g3 = G[p + so + e];
        const uint8_t s0 = S[p], s1 = S[p + e], s2 = S[p + so], s3 = S[p + so + e];
        g = g0 == o;
        s = s0 == o;
        bg = boundary_bit(g, he && g1 == o, hs && g2 == o, he && hs && g3 == o, he, hs);
        bs = boundary_bit(s, he && s1 == o, hs && s2 == o, he && hs && s3 == o, he, hs);
      }
      wg = __ballot(bg);
      ws = __ballot(bs);
      if (ry >= r && ry < r + JF_TILE && rj >= 1 && rj <= JF_XW) {
        n_and += __popcll(__ballot(g && s));
        n_or += __popcll(__ballot(g || s));
        n_bs += __popcll(ws);
        n_bg += __popcll(wg);
      }
    }
    if (lane == 0) {
      bG[it] = wg;
      bS[it] = ws;
    }
  }
  __syncthreads();
  if (lane == 0) {
    if (n_and) atomicAdd(&acc[0], n_and);
    if (n_or) atomicAdd(&acc[1], n_or);
    if (n_bs) atomicAdd(&acc[2], n_bs);
    if (n_bg) atomicAdd(&acc[3], n_bg);
  }

  // ---- hits: boundary bits of one map under the dilated boundary of the other; one word per thread ----
  unsigned hit_s = 0, hit_g = 0;
  for (int it = tid; it < JF_TILE * JF_XW; it += JF_BLOCK) {
    const int ty = it / JF_XW, tj = it % JF_XW;
    const int ci = (ty + r) * words + tj + 1;
    const u64 cs = bS[ci], cg = bG[ci];
    if ((cs | cg) == 0) continue;
    u64 dil_g = 0, dil_s = 0;
    for (int dy = -r; dy <= r; ++dy) {
      const int k = __builtin_amdgcn_readfirstlane(chord[dy < 0 ? -dy : dy]);     // dy is the same in every lane: scalar shift counts
      const int ri = ci + dy * words;                                 // rows (ty + r + dy) in [0, rows), words tj + 1 +- 1 in [0, words)
      if (cs) {
        const u64 l = bG[ri - 1], c = bG[ri], rr = bG[ri + 1];
        if (l | c | rr) dil_g |= dilate_row_word(l, c, rr, k);
      }
      if (cg) {
        const u64 l = bS[ri - 1], c = bS[ri], rr = bS[ri + 1];
        if (l | c | rr) dil_s |= dilate_row_word(l, c, rr, k);
      }
    }
    hit_s += __popcll(cs & dil_g);
    hit_g += __popcll(cg & dil_s);
  }
  if (hit_s) atomicAdd(&acc[4], hit_s);
  if (hit_g) atomicAdd(&acc[5], hit_g);
  __syncthreads();
  if (tid < 6 && acc[tid]) atomicAdd(a.counts + ((size_t)t * a.n_objects + (o - 1)) * 6 + tid, (u64)acc[tid]);
}

int jf_tile_rows() { return JF_TILE; }

int jf_counts_launch(const uint8_t* gt, const uint8_t* pred, int T, int h, int w, int n_objects, int radius, int64_t* counts, hipStream_t s) {
  const hipError_t e = hipMemsetAsync(counts, 0, (size_t)T * n_objects * 6 * sizeof(int64_t), s);
  if (e != hipSuccess) {
    set_error("fgvc_jf_counts_u8: clearing the counts failed: %s", hipGetErrorString(e));
    return FGVC_ERR_LAUNCH;
  }
  if (h == 0 || w == 0) return FGVC_OK;
  JfArgs a;
  a.gt = gt; a.pred = pred; a.counts = reinterpret_cast<u64*>(counts);
  a.h = h; a.w = w; a.n_objects = n_objects; a.radius = radius;
  a.xtiles = cdiv(cdiv(w, 64), JF_XW);
  const size_t lds = (size_t)2 * (JF_TILE + 2 * radius) * (JF_XW + 2) * sizeof(u64);     // 46080 bytes at radius 64
  for (int t0 = 0; t0 < T; t0 += 65535) {                                                 // grid.z is 16-bit
    a.t0 = t0;
    const dim3 grid(cdiv(h, JF_TILE) * a.xtiles, n_objects, imin(T - t0, 65535));
    jf_counts_kernel<<<grid, JF_BLOCK, lds, s>>>(a);
    FGVC_CHECK_LAUNCH("fgvc_jf_counts_u8");
  }
  return FGVC_OK;
}

}  // namespace fgvc
