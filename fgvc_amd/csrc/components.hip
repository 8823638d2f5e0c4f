// Connected components of id maps: the labels of metrics.components_host and the cleaning rule of
// metrics.clean_masks_host (drop small / all but the largest component of an id, then fill holes) from a (T, h, w) uint8 id map.
//   * a pixel's label is the smallest linear index y * w + x of its component (its root); labels live in an int32 word per pixel and only
//     ever DECREASE, and L[p] <= p always holds, so every chase of a label ends at a word that holds its own index.
//   * ccl_tile_kernel: one workgroup stages a 16 x 64 tile of ids in LDS, unites each pixel with its W, N, NW, NE neighbours of the tile by
//     union-find on LDS words (atomicMin on the larger root, retried with the value returned), and writes each pixel's label as the frame
//     index of its tile-local root.  It also clears the per-pixel words the later launches add to.
//   * ccl_seam_kernel: the pixels of a tile's first row and first / last column unite with their neighbours in OTHER tiles, the same union
//     on the global words.  Labels are read with agent-scope atomic loads; an older value is still an ancestor, so only progress, never
//     the result, depends on how fresh a read is.  The final root of a component is its minimum index whatever the order of arrival.
//   * ccl_flatten_kernel: label = root; a run of lanes with one root adds its length to the root's area word in one 32-bit atomic.
//     On the background pass it also records, per root, whether the component touches the frame's border and whether its 4-neighbours
//     that are not background carry ONE id (a word: EMPTY, an id, or an id with the CONFLICT bit).
//   * ccl_best_kernel (keep = largest only): per (frame, id) a 64-bit atomicMax of (area << 32) | ~root -- the largest, the smaller root
//     on ties.  ccl_apply_kernel writes the map after the drop and the statistics, ccl_fill_kernel the filled holes.
// No kernel waits for another workgroup: the launches on the one stream are the only order between workgroups.  All atomics are integer
// minima, maxima, sums, ors and a compare-and-swap whose loser only sets a bit, so every output is the same in any order of arrival.
#include <limits.h>

#include "common.hpp"

namespace fgvc {

namespace {

constexpr int CCL_TR = 16, CCL_TC = 64;          // a tile: one wave per row
constexpr int CCL_BLOCK = CCL_TR * CCL_TC;
constexpr int CCL_SEAM_BLOCK = 128;              // 64 pixels of the first row, 15 + 15 of the first and last column
constexpr unsigned HOLE_EMPTY = 0x200u, HOLE_CONFLICT = 0x100u;

typedef unsigned long long u64;

struct CclArgs {
  const uint8_t* map;                            // the map that is labelled, through its strides
  long long st, sy;
  const uint8_t* flags;                          // per frame: 0 = the frame is left alone; null = every frame
  int* lab;                                      // [T][h w]
  int* area;                                     // [T][h w] or null
  unsigned* info;                                // [T][h w] or null (the background pass)
  u64* zero_a;                                   // words the tile kernel clears (the statistics, the best keys), or null
  u64* zero_b;
  long long n_zero_a, n_zero_b;
  int h, w, tx, ty;
  int lo, hi;                                    // ids lo <= id < hi take part
  int conn;
};

struct CclPos {
  int t, y0, x0;
};

// workgroup -> (frame, tile row, tile column); tx, ty: the tiles of a frame's width and height
__device__ __forceinline__ CclPos ccl_pos(int tx, int ty) {
  const unsigned b = blockIdx.x;
  CclPos p;
  p.x0 = (int)(b % (unsigned)tx) * CCL_TC;
  p.y0 = (int)(b / (unsigned)tx % (unsigned)ty) * CCL_TR;
  p.t = (int)(b / ((unsigned)tx * (unsigned)ty));
  return p;
}

__device__ __forceinline__ bool ccl_on(const CclArgs& k, int t) { return k.flags == nullptr || k.flags[t] != 0; }

// ---- union-find on label words: LDS words at workgroup scope, global words at agent scope -------------------------------------------------
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* L, int a) {
  for (;;) {
    const int l = __hip_atomic_load(L + a, __ATOMIC_RELAXED, SCOPE);
    if (l == a) return a;
    a = l;                                       // l < a
  }
}

template <int SCOPE>
__device__ __forceinline__ void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(L, a);
    b = uf_find<SCOPE>(L, b);
    if (a == b) return;
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(L + a, b);         // a > b
    if (old == a) return;                        // a was a root and now hangs below b
    a = old;                                     // somebody was first: a's former parent (< a) joins b next
  }
}

__device__ __forceinline__ int lds_find(int* L, int a) { return uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(L, a); }
__device__ __forceinline__ void lds_union(int* L, int a, int b) { uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(L, a, b); }
__device__ __forceinline__ int glb_find(int* L, int a) { return uf_find<__HIP_MEMORY_SCOPE_AGENT>(L, a); }
__device__ __forceinline__ void glb_union(int* L, int a, int b) { uf_union<__HIP_MEMORY_SCOPE_AGENT>(L, a, b); }

}  // namespace

__global__ __launch_bounds__(CCL_BLOCK) void ccl_tile_kernel(const CclArgs k) {
  __shared__ int lab[CCL_BLOCK];
  __shared__ short sid[CCL_BLOCK];
  const int tid = threadIdx.x;
  const size_t gtid = (size_t)blockIdx.x * CCL_BLOCK + tid, gsize = (size_t)gridDim.x * CCL_BLOCK;
  for (size_t i = gtid; i < (size_t)k.n_zero_a; i += gsize) k.zero_a[i] = 0;
  for (size_t i = gtid; i < (size_t)k.n_zero_b; i += gsize) k.zero_b[i] = 0;
  const CclPos c = ccl_pos(k.tx, k.ty);
  if (!ccl_on(k, c.t)) return;
  const int ly = tid / CCL_TC, lx = tid % CCL_TC, y = c.y0 + ly, x = c.x0 + lx;
  const bool inside = y < k.h && x < k.w;
  int v = -1;
  if (inside) {
    const int id = k.map[(long long)c.t * k.st + (long long)y * k.sy + x];
    if (id >= k.lo && id < k.hi) v = id;
  }
  sid[tid] = (short)v;
  lab[tid] = tid;
  __syncthreads();
  if (v >= 0) {
    if (lx > 0 && sid[tid - 1] == v) lds_union(lab, tid, tid - 1);
    const bool north = ly > 0 && sid[tid - CCL_TC] == v;
    if (north) lds_union(lab, tid, tid - CCL_TC);
    // with the north pixel in the component, NW and NE hang on it through its own W union and its east neighbour's
    if (ly > 0 && !north && v != 0 && k.conn == 8) {
      if (lx > 0 && sid[tid - CCL_TC - 1] == v) lds_union(lab, tid, tid - CCL_TC - 1);
      if (lx < CCL_TC - 1 && sid[tid - CCL_TC + 1] == v) lds_union(lab, tid, tid - CCL_TC + 1);
    }
  }
  __syncthreads();
  if (!inside) return;
  const size_t g = (size_t)c.t * k.h * k.w + (size_t)y * k.w + x;
  int l = -1;
  if (v >= 0) {
    const int r = lds_find(lab, tid);
    l = (c.y0 + r / CCL_TC) * k.w + c.x0 + r % CCL_TC;
  }
  k.lab[g] = l;
  if (k.area) k.area[g] = 0;
  if (k.info) k.info[g] = HOLE_EMPTY;
}

__global__ __launch_bounds__(CCL_SEAM_BLOCK) void ccl_seam_kernel(const CclArgs k) {
  const CclPos c = ccl_pos(k.tx, k.ty);
  if (!ccl_on(k, c.t)) return;
  const int i = threadIdx.x;
  int ly, lx;
  if (i < CCL_TC) {
    ly = 0;
    lx = i;
  } else if (i < CCL_TC + CCL_TR - 1) {
    ly = i - CCL_TC + 1;
    lx = 0;
  } else if (i < CCL_TC + 2 * (CCL_TR - 1)) {
    ly = i - (CCL_TC + CCL_TR - 1) + 1;
    lx = CCL_TC - 1;
  } else {
    return;
  }
  const int y = c.y0 + ly, x = c.x0 + lx;
  if (y >= k.h || x >= k.w) return;
  const uint8_t* f = k.map + (long long)c.t * k.st;
  const int v = f[(long long)y * k.sy + x];
  if (v < k.lo || v >= k.hi) return;
  int* L = k.lab + (size_t)c.t * k.h * k.w;
  const int p = y * k.w + x;
  const bool diag = v != 0 && k.conn == 8;
  if (lx == 0 && x > 0 && f[(long long)y * k.sy + x - 1] == v) glb_union(L, p, p - 1);
  if (ly == 0 && y > 0) {
    const uint8_t* up = f + (long long)(y - 1) * k.sy;
    if (up[x] == v) glb_union(L, p, p - k.w);
    if (diag && x > 0 && up[x - 1] == v) glb_union(L, p, p - k.w - 1);
    if (diag && x + 1 < k.w && up[x + 1] == v) glb_union(L, p, p - k.w + 1);
  } else if (diag && y > 0) {                    // a column pixel below the tile's first row: the diagonal that leaves the tile
    const uint8_t* up = f + (long long)(y - 1) * k.sy;
    if (lx == 0 && x > 0 && up[x - 1] == v) glb_union(L, p, p - k.w - 1);
    if (lx == CCL_TC - 1 && x + 1 < k.w && up[x + 1] == v) glb_union(L, p, p - k.w + 1);
  }
}

__global__ __launch_bounds__(CCL_BLOCK) void ccl_flatten_kernel(const CclArgs k) {
  const CclPos c = ccl_pos(k.tx, k.ty);
  if (!ccl_on(k, c.t)) return;
  const int tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int ly = tid / CCL_TC, lx = tid % CCL_TC, y = c.y0 + ly, x = c.x0 + lx;
  const bool inside = y < k.h && x < k.w;
  const uint8_t* f = k.map + (long long)c.t * k.st;
  const size_t base = (size_t)c.t * k.h * k.w;
  int* L = k.lab + base;
  const int p = y * k.w + x;
  int r = -1;
  if (inside) {
    const int v = f[(long long)y * k.sy + x];
    if (v >= k.lo && v < k.hi) {
      r = glb_find(L, p);
      __hip_atomic_store(L + p, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  if (k.area == nullptr) return;
  // a wave is one row of the tile: a run of lanes with one root adds its length once
  const int prev = __shfl_up(r, 1);
  const bool head = lane == 0 || prev != r;
  const u64 heads = __ballot(head);
  if (head && r >= 0) {
    const u64 after = lane == WAVE - 1 ? 0ull : heads >> (lane + 1);
    const int len = after ? __ffsll((long long)after) : WAVE - lane;
    atomicAdd(k.area + base + r, len);
  }
  if (k.info == nullptr || r < 0) return;
  // the background pass: what bounds the component
  unsigned* I = k.info + base + r;
  unsigned cur = __hip_atomic_load(I, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (cur & HOLE_CONFLICT) return;               // the bit is never cleared
  if (y == 0 || y == k.h - 1 || x == 0 || x == k.w - 1) {
    atomicOr(I, HOLE_CONFLICT);
    return;
  }
  const unsigned nb[4] = {f[(long long)y * k.sy + x - 1], f[(long long)y * k.sy + x + 1], f[(long long)(y - 1) * k.sy + x],
                          f[(long long)(y + 1) * k.sy + x]};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned id = nb[j];
    if (id == 0 || id == cur) continue;
    const unsigned old = atomicCAS(I, HOLE_EMPTY, id);
    if (old == HOLE_EMPTY) {
      cur = id;
    } else if (old != id) {                      // a second id, or the bit is set already
      atomicOr(I, HOLE_CONFLICT);
      return;
    } else {
      cur = id;
    }
  }
}

namespace {

struct CleanArgs {
  const uint8_t* ids;
  long long st, sy;
  uint8_t* out;
  long long ost, osy;
  const uint8_t* flags;
  const int* lab;
  const int* area;
  const unsigned* info;
  u64* best;                                     // [T][n_ids]
  u64* stats;                                    // [T][n_ids][4]
  int h, w, tx, ty, n_ids, min_area, largest, max_hole;
};

}  // namespace

// the roots of the components of ids 1 .. n_ids - 1: the largest of each (frame, id), the smaller root on equal areas
__global__ __launch_bounds__(CCL_BLOCK) void ccl_best_kernel(const CleanArgs k) {
  const CclPos c = ccl_pos(k.tx, k.ty);
  if (k.flags && k.flags[c.t] == 0) return;
  const int tid = threadIdx.x, y = c.y0 + tid / CCL_TC, x = c.x0 + tid % CCL_TC;
  if (y >= k.h || x >= k.w) return;
  const int p = y * k.w + x;
  const size_t base = (size_t)c.t * k.h * k.w;
  if (k.lab[base + p] != p) return;
  const int id = k.ids[(long long)c.t * k.st + (long long)y * k.sy + x];
  atomicMax(k.best + (size_t)c.t * k.n_ids + id, ((u64)(unsigned)k.area[base + p] << 32) | (unsigned)~(unsigned)p);
}

__global__ __launch_bounds__(CCL_BLOCK) void ccl_apply_kernel(const CleanArgs k) {
  const CclPos c = ccl_pos(k.tx, k.ty);
  const int tid = threadIdx.x, y = c.y0 + tid / CCL_TC, x = c.x0 + tid % CCL_TC;
  if (y >= k.h || x >= k.w) return;
  const int id = k.ids[(long long)c.t * k.st + (long long)y * k.sy + x];
  int o = id;
  if ((k.flags == nullptr || k.flags[c.t] != 0) && id > 0 && id < k.n_ids) {
    const int p = y * k.w + x;
    const size_t base = (size_t)c.t * k.h * k.w, row = (size_t)c.t * k.n_ids + id;
    const int r = k.lab[base + p], a = k.area[base + r];
    bool keep = a >= k.min_area;
    if (k.largest) keep = keep && ~(unsigned)k.best[row] == (unsigned)r;
    if (r == p) {
      atomicAdd(k.stats + row * 4 + 0, 1ull);
      if (keep) atomicAdd(k.stats + row * 4 + 1, 1ull);
      else atomicAdd(k.stats + row * 4 + 2, (u64)a);
    }
    o = keep ? id : 0;
  }
  k.out[(long long)c.t * k.ost + (long long)y * k.osy + x] = (uint8_t)o;
}

__global__ __launch_bounds__(CCL_BLOCK) void ccl_fill_kernel(const CleanArgs k) {
  const CclPos c = ccl_pos(k.tx, k.ty);
  if (k.flags && k.flags[c.t] == 0) return;
  const int tid = threadIdx.x, y = c.y0 + tid / CCL_TC, x = c.x0 + tid % CCL_TC;
  if (y >= k.h || x >= k.w) return;
  uint8_t* o = k.out + (long long)c.t * k.ost + (long long)y * k.osy + x;
  if (*o != 0) return;
  const int p = y * k.w + x;
  const size_t base = (size_t)c.t * k.h * k.w;
  const int r = k.lab[base + p], a = k.area[base + r];
  const unsigned inf = k.info[base + r];
  if ((inf & (HOLE_CONFLICT | HOLE_EMPTY)) || inf >= (unsigned)k.n_ids || a > k.max_hole) return;
  *o = (uint8_t)inf;
  if (r == p) atomicAdd(k.stats + ((size_t)c.t * k.n_ids + inf) * 4 + 3, (u64)a);
}

void ccl_tile(int* rows, int* cols) {
  *rows = CCL_TR;
  *cols = CCL_TC;
}

long long ccl_blocks(int T, int h, int w) {
  return (long long)T * ((h + CCL_TR - 1) / CCL_TR) * (((long long)w + CCL_TC - 1) / CCL_TC);
}

size_t clean_workspace_bytes(int T, int h, int w, int n_ids) {
  return (size_t)T * n_ids * sizeof(u64) + (size_t)T * h * w * 3 * sizeof(int);
}

// tile, seam, flatten: three launches
static int ccl_label(const char* fn, const CclArgs& a, unsigned blocks, hipStream_t s) {
  ccl_tile_kernel<<<dim3(blocks), CCL_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH(fn);
  ccl_seam_kernel<<<dim3(blocks), CCL_SEAM_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH(fn);
  ccl_flatten_kernel<<<dim3(blocks), CCL_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH(fn);
  return FGVC_OK;
}

int components_launch(const uint8_t* ids, long long st, long long sy, int T, int h, int w, int connectivity, int background, int32_t* labels,
                      hipStream_t s) {
  CclArgs a = {};
  a.map = ids; a.st = st; a.sy = sy;
  a.lab = labels;
  a.h = h; a.w = w; a.tx = (w + CCL_TC - 1) / CCL_TC; a.ty = (h + CCL_TR - 1) / CCL_TR;
  a.lo = background ? 0 : 1; a.hi = 256; a.conn = connectivity;
  return ccl_label("fgvc_seg_components_i32", a, (unsigned)ccl_blocks(T, h, w), s);
}

int clean_launch(const uint8_t* ids, long long st, long long sy, int T, int h, int w, int n_ids, int connectivity, int min_area, int keep_largest,
                 int fill_holes, long long max_hole_area, const uint8_t* frame_flags, uint8_t* out, long long ost, long long osy, int64_t* stats,
                 void* workspace, hipStream_t s) {
  const char* fn = "fgvc_seg_clean_u8";
  const size_t px = (size_t)T * h * w;
  u64* best = reinterpret_cast<u64*>(workspace);
  int* lab = reinterpret_cast<int*>(best + (size_t)T * n_ids);
  int* area = lab + px;
  unsigned* info = reinterpret_cast<unsigned*>(area + px);
  const unsigned blocks = (unsigned)ccl_blocks(T, h, w);

  CclArgs a = {};
  a.map = ids; a.st = st; a.sy = sy; a.flags = frame_flags;
  a.lab = lab; a.area = area;
  a.zero_a = reinterpret_cast<u64*>(stats); a.n_zero_a = (long long)T * n_ids * 4;
  a.zero_b = best; a.n_zero_b = (long long)T * n_ids;
  a.h = h; a.w = w; a.tx = (w + CCL_TC - 1) / CCL_TC; a.ty = (h + CCL_TR - 1) / CCL_TR;
  a.lo = 1; a.hi = n_ids; a.conn = connectivity;
  int rc = ccl_label(fn, a, blocks, s);
  if (rc != FGVC_OK) return rc;

  CleanArgs c = {};
  c.ids = ids; c.st = st; c.sy = sy; c.out = out; c.ost = ost; c.osy = osy; c.flags = frame_flags;
  c.lab = lab; c.area = area; c.info = info; c.best = best; c.stats = reinterpret_cast<u64*>(stats);
  c.h = h; c.w = w; c.tx = a.tx; c.ty = a.ty; c.n_ids = n_ids;
  c.min_area = min_area; c.largest = keep_largest;
  c.max_hole = max_hole_area < 0 || max_hole_area > INT_MAX ? INT_MAX : (int)max_hole_area;
  if (keep_largest) {
    ccl_best_kernel<<<dim3(blocks), CCL_BLOCK, 0, s>>>(c);
    FGVC_CHECK_LAUNCH(fn);
  }
  ccl_apply_kernel<<<dim3(blocks), CCL_BLOCK, 0, s>>>(c);
  FGVC_CHECK_LAUNCH(fn);
  if (!fill_holes) return FGVC_OK;

  // the background of the map just written: 4-neighbours, with what bounds each component
  CclArgs b = {};
  b.map = out; b.st = ost; b.sy = osy; b.flags = frame_flags;
  b.lab = lab; b.area = area; b.info = info;
  b.h = h; b.w = w; b.tx = a.tx; b.ty = a.ty;
  b.lo = 0; b.hi = 1; b.conn = 4;
  rc = ccl_label(fn, b, blocks, s);
  if (rc != FGVC_OK) return rc;
  ccl_fill_kernel<<<dim3(blocks), CCL_BLOCK, 0, s>>>(c);
  FGVC_CHECK_LAUNCH(fn);
  return FGVC_OK;
}

}  // namespace fgvc
