// Objects as boxes: per frame and id, the eight integer words of metrics.object_stats_host -- area, the half-open
// box, the coordinate sums and the border count -- from a (T, h, w) uint8 id map in one launch.
//   * ONE workgroup of 16 waves owns a frame.  The minimum words are why: the result of a minimum has no neutral start among the values a
//     cleared buffer can hold (0 is a legitimate x0), so bands of one frame in several workgroups would need a finishing pass after their
//     atomics.  With the frame in one workgroup the table stays in LDS, every output word is written by one plain store, nothing has to be
//     cleared first and no global atomic is issued.
//   * the frame is cut into items of one row x 1024 pixels (64 lanes x 16 pixels: one or two aligned 16-byte loads per lane, shifted into place),
//     numbered segment-major; each wave takes a contiguous band of items, so a lane keeps its 16 columns over consecutive rows.
//   * a lane finds the runs of equal ids in its 16 pixels (all 16 equal: one compare) and adds each run [a, b) on row y to a REGISTER
//     accumulator of the id it is on: b - a, (a + b - 1)(b - a) / 2, y (b - a), the border pixels, the box.  Only a CHANGE of id sends the
//     accumulator to the LDS table (64-bit LDS atomics: add, min, max), so a background that fills the frame costs each lane one flush --
//     and where a whole wave ends on one id, the wave reduces across lanes first and one lane flushes.
// Everything is an integer sum, minimum or maximum: the same in any order.
#include "common.hpp"

namespace fgvc {

namespace {

constexpr int OBJ_BLOCK = 1024;
constexpr int OBJ_WAVES = OBJ_BLOCK / WAVE;
constexpr int OBJ_PX = 16;                       // pixels per lane
constexpr int OBJ_SEG = WAVE * OBJ_PX;           // pixels per item
constexpr int OBJ_BATCH = 4;                     // items whose loads are in flight together
constexpr int OBJ_MAX_IDS = 256;

typedef unsigned long long u64;

struct ObjArgs {
  const uint8_t* ids;
  long long st, sy;
  u64* out;
  int h, w, n_ids, segs;
};

struct ObjAcc {
  int id;                                         // -1: nothing yet
  u64 area, sx, sy, border;
  unsigned x0, y0, x1, y1;
  __device__ __forceinline__ void reset(int o) {
    id = o;
    area = sx = sy = border = 0;
    x0 = y0 = ~0u;
    x1 = y1 = 0;
  }
};

__device__ __forceinline__ void obj_flush(u64* tab, const ObjAcc& c) {
  if (c.id < 0) return;
  u64* r = tab + c.id * 8;
  atomicAdd(r + 0, c.area);
  atomicMin(r + 1, (u64)c.x0);
  atomicMin(r + 2, (u64)c.y0);
  atomicMax(r + 3, (u64)c.x1);
  atomicMax(r + 4, (u64)c.y1);
  atomicAdd(r + 5, c.sx);
  atomicAdd(r + 6, c.sy);
  if (c.border) atomicAdd(r + 7, c.border);
}

// the run [a, b) of `id` on row y
__device__ __forceinline__ void obj_run(u64* tab, ObjAcc& c, const ObjArgs& k, unsigned id, unsigned a, unsigned b, unsigned y) {
  if (id >= (unsigned)k.n_ids) return;           // an id the caller did not ask for: counted nowhere
  if ((int)id != c.id) {
    obj_flush(tab, c);
    c.reset((int)id);
  }
  const u64 len = b - a;
  c.area += len;
  c.sx += ((u64)a + b - 1) * len / 2;            // a + .. + (b - 1); one of the two factors is even
  c.sy += (u64)y * len;
  const bool edge_row = y == 0 || y == (unsigned)k.h - 1;
  c.border += edge_row ? len : (u64)((a == 0) + (b == (unsigned)k.w && k.w > 1));
  c.x0 = a < c.x0 ? a : c.x0;
  c.x1 = b > c.x1 ? b : c.x1;
  c.y0 = y < c.y0 ? y : c.y0;
  c.y1 = y + 1 > c.y1 ? y + 1 : c.y1;
}

// n <= 16 pixels at p (1 <= n) as two little-endian words; what lies past n in them is unspecified.  Rows start anywhere (854 columns
// put seven rows in eight off a 16-byte boundary), so the bytes come as the one or two ALIGNED 16-byte words that hold them, shifted into
// place.  Each word read holds at least one pixel of the lane, so it lies in a page of the map: bytes beside the map may be read, never
// used.
__device__ __forceinline__ void obj_load(const uint8_t* p, unsigned n, u64& lo, u64& hi) {
  const unsigned sh = (unsigned)reinterpret_cast<uintptr_t>(p) & 15u;
  const uint4* q = reinterpret_cast<const uint4*>(p - sh);
  const uint4 a = q[0];
  uint4 b = {0, 0, 0, 0};
  if (sh + n > 16) b = q[1];
  u64 w0 = a.x | ((u64)a.y << 32), w1 = a.z | ((u64)a.w << 32), w2 = b.x | ((u64)b.y << 32);
  const u64 w3 = b.z | ((u64)b.w << 32);
  if (sh & 8u) {
    w0 = w1;
    w1 = w2;
    w2 = w3;
  }
  const unsigned s = (sh & 7u) * 8;
  lo = s ? (w0 >> s) | (w1 << (64 - s)) : w0;
  hi = s ? (w1 >> s) | (w2 << (64 - s)) : w1;
}

__device__ __forceinline__ u64 shfl_xor_u64(u64 v, int m) {
  const unsigned a = __shfl_xor((unsigned)v, m), b = __shfl_xor((unsigned)(v >> 32), m);
  return a | ((u64)b << 32);
}

}  // namespace

__global__ __launch_bounds__(OBJ_BLOCK) void object_stats_kernel(const ObjArgs k) {
  __shared__ u64 tab[OBJ_MAX_IDS * 8];
  const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int words = k.n_ids * 8;
  for (int i = tid; i < words; i += OBJ_BLOCK) tab[i] = ((i & 7) == 1 || (i & 7) == 2) ? ~0ull : 0ull;
  __syncthreads();

  const uint8_t* frame = k.ids + (long long)blockIdx.x * k.st;
  const long long items = (long long)k.h * k.segs;
  const long long per = (items + OBJ_WAVES - 1) / OBJ_WAVES;
  const long long i0 = per * wave, i1 = i0 + per < items ? i0 + per : items;
  ObjAcc c;
  c.reset(-1);
  if (i0 < i1) {
    unsigned seg = (unsigned)(i0 / k.h), y = (unsigned)(i0 % k.h);
    for (long long it = i0; it < i1; it += OBJ_BATCH) {
      u64 lo[OBJ_BATCH], hi[OBJ_BATCH];
      unsigned xs[OBJ_BATCH], ys[OBJ_BATCH], ns[OBJ_BATCH];
#pragma unroll
      for (int j = 0; j < OBJ_BATCH; ++j) {
        ns[j] = 0;
        xs[j] = ys[j] = 0;
        lo[j] = hi[j] = 0;
        if (it + j < i1) {
          const unsigned x = seg * OBJ_SEG + lane * OBJ_PX;
          xs[j] = x;
          ys[j] = y;
          if (x < (unsigned)k.w) {
            const unsigned left = (unsigned)k.w - x;
            ns[j] = left < OBJ_PX ? left : OBJ_PX;
            obj_load(frame + (long long)y * k.sy + x, ns[j], lo[j], hi[j]);
          }
          if (++y == (unsigned)k.h) {
            y = 0;
            ++seg;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < OBJ_BATCH; ++j) {
        const unsigned n = ns[j], x = xs[j];
        if (n == 0) continue;
        u64 l = lo[j], hh = hi[j];
        unsigned rid = (unsigned)(l & 255), ra = x;
        const bool uniform = n == OBJ_PX && hh == l && l == rid * 0x0101010101010101ull;
        unsigned i = uniform ? n : 1;
        for (;;) {
          l = (l >> 8) | (hh << 56);
          hh >>= 8;
          const unsigned id = i < n ? (unsigned)(l & 255) : 256u;      // 256: the end of the lane's pixels closes the run
          if (id != rid) {
            obj_run(tab, c, k, rid, ra, x + i, ys[j]);
            if (i >= n) break;
            rid = id;
            ra = x + i;
          }
          ++i;
        }
      }
    }
  }

  // the last accumulators: a wave whose lanes all ended on one id (or on none) adds them up first
  const u64 have = __ballot(c.id >= 0);
  if (have) {
    const int fid = __shfl(c.id, __ffsll((long long)have) - 1);
    if (__all(c.id < 0 || c.id == fid)) {
      for (int m = 1; m < WAVE; m *= 2) {
        c.area += shfl_xor_u64(c.area, m);
        c.sx += shfl_xor_u64(c.sx, m);
        c.sy += shfl_xor_u64(c.sy, m);
        c.border += shfl_xor_u64(c.border, m);
        const unsigned ax0 = __shfl_xor(c.x0, m), ay0 = __shfl_xor(c.y0, m), ax1 = __shfl_xor(c.x1, m), ay1 = __shfl_xor(c.y1, m);
        c.x0 = ax0 < c.x0 ? ax0 : c.x0;
        c.y0 = ay0 < c.y0 ? ay0 : c.y0;
        c.x1 = ax1 > c.x1 ? ax1 : c.x1;
        c.y1 = ay1 > c.y1 ? ay1 : c.y1;
      }
      c.id = fid;
      if (lane == 0) obj_flush(tab, c);
    } else {
      obj_flush(tab, c);
    }
  }
  __syncthreads();

  u64* out = k.out + (size_t)blockIdx.x * words;
  for (int i = tid; i < words; i += OBJ_BLOCK) {
    const bool is_min = (i & 7) == 1 || (i & 7) == 2;
    out[i] = is_min && tab[i & ~7] == 0 ? 0ull : tab[i];               // an absent id: eight zeros
  }
}

int object_stats_launch(const uint8_t* ids, long long st, long long sy, int T, int h, int w, int n_ids, int64_t* stats, hipStream_t s) {
  ObjArgs a;
  a.ids = ids; a.st = st; a.sy = sy; a.out = reinterpret_cast<u64*>(stats);
  a.h = h; a.w = w; a.n_ids = n_ids;
  a.segs = (int)(((long long)w + OBJ_SEG - 1) / OBJ_SEG);
  object_stats_kernel<<<dim3(T), OBJ_BLOCK, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_seg_object_stats_u8");
  return FGVC_OK;
}

}  // namespace fgvc
