// Object crops: windows that follow each object, and their anti-aliased resampling onto a fixed size.
//   * object_windows_kernel: metrics.object_windows_host word for word.  One thread per (frame, object) walks the 2 r + 1 statistics rows
//     around its frame; everything is a 64-bit integer, floor and ceiling divisions are spelled out (C++ `/` truncates).
//   * crop_plan_kernel: the float64 half of viz.crop_windows_host.  One thread per (crop, axis, output index) runs the sequential tap loop
//     of viz.crop_axis_coefficients -- every operation rounded, none contracted, the taps' sum in increasing order -- and leaves the first
//     tap, the tap count and the fixed-point coefficients K = int(0.5 + k 2^22) in the caller's workspace.
//   * crop_resample_kernel: the integer half.  A workgroup owns (crop, band of CROP_BAND output rows, chunk of CROP_COLS output columns),
//     a thread one output column and channel.  The column's horizontal coefficients sit in LDS, tap-major, so that the threads of a wave
//     read consecutive banks.  The thread walks the band's source rows once: per row the clipped horizontal sum -- the uint8 intermediate
//     of the rule, which therefore never exists in memory -- is added, times the row's vertical coefficient, into the register accumulator
//     of every output row of the band whose tap range holds the source row.  Row ranges and vertical coefficients are the same for the
//     whole workgroup (scalar registers and scalar loads).  The mask bytes (nearest pixel of the mask-space window) leave in the same launch.
// Every output byte has one writer; there is no atomic anywhere.  A window that is empty, beyond CROP_LIMIT or needs more than max_taps
// taps on an axis (viz.crop_window_ok) is not planned and its crop is `fill`, its mask zero.
#include "common.hpp"

// the plan kernel restates numpy float64 one rounded operation after another: a contracted multiply-add would move a first tap or a coefficient
#pragma clang fp contract(off)

namespace fgvc {

namespace {

constexpr int CROP_COLS = 64;                   // output columns of a workgroup
constexpr int CROP_BLOCK = CROP_COLS * 3;       // a thread per (column, channel): three waves
constexpr int CROP_BAND = 8;                    // output rows of a workgroup, one register accumulator each
constexpr int CROP_BITS = 22;
constexpr long long CROP_LIMIT = 1ll << 30;

typedef long long i64;

__host__ __device__ __forceinline__ i64 fdiv64(i64 a, i64 b) {          // floor(a / b), b > 0
  const i64 q = a / b;
  return (a % b < 0) ? q - 1 : q;
}
__host__ __device__ __forceinline__ i64 cdiv64(i64 a, i64 b) {          // ceil(a / b), b > 0, any a
  const i64 q = a / b;
  return (a % b > 0) ? q + 1 : q;
}
__host__ __device__ __forceinline__ i64 max64(i64 a, i64 b) { return a > b ? a : b; }
__host__ __device__ __forceinline__ i64 abs64(i64 a) { return a < 0 ? -a : a; }

struct WinArgs {
  const i64* stats;
  const int* objects;
  i64* out;
  int T, N, M, S_h, S_w, pad_q, min_side, smooth, h, w, H, W;
};

struct CropArgs {
  const uint8_t* frames;
  i64 st, sy, sx, sc;
  const i64* windows;
  const uint8_t* ids;
  i64 ids_st, ids_sy;
  const int* objects;
  uint8_t* crops;
  uint8_t* masks;
  int* table;
  int T, H, W, M, words, S_h, S_w, h, w, max_taps, fill0, fill1, fill2;
};

__device__ __forceinline__ int crop_axis_taps(i64 span, int n) { return (int)(2 * cdiv64(max64(span, n), n) + 2); }

__device__ __forceinline__ bool crop_window_ok(i64 x0, i64 y0, i64 x1, i64 y1, const CropArgs& k) {
  if (x1 <= x0 || y1 <= y0) return false;
  if (max64(max64(abs64(x0), abs64(y0)), max64(abs64(x1), abs64(y1))) >= CROP_LIMIT) return false;
  return crop_axis_taps(x1 - x0, k.S_w) <= k.max_taps && crop_axis_taps(y1 - y0, k.S_h) <= k.max_taps;
}

// a crop's part of the table, in ints: x first taps [S_w], x tap counts [S_w], y first taps [S_h], y tap counts [S_h], x coefficients
// [S_w][max_taps], y coefficients [S_h][max_taps]
__host__ __device__ __forceinline__ size_t crop_table_ints(int S_h, int S_w, int max_taps) { return (size_t)(S_h + S_w) * (size_t)(2 + max_taps); }

__device__ __forceinline__ int clip8_round(int v) {
  v = (v + (1 << (CROP_BITS - 1))) >> CROP_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

}  // namespace

__global__ __launch_bounds__(256) void object_windows_kernel(const WinArgs k) {
  const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (i64)k.T * k.M) return;
  const int t = (int)(gid / k.M), j = (int)(gid % k.M);
  i64* out = k.out + gid * 8;
  const int o = k.objects[j];
  const bool known = o >= 0 && o < k.N;
  const i64* col = k.stats + (i64)(known ? o : 0) * 8;
  const i64 row = (i64)k.N * 8;
  if (!known || col[t * row] <= 0) {
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = 0;
    return;
  }
  const int u0 = t - k.smooth > 0 ? t - k.smooth : 0;
  const int u1 = (i64)t + k.smooth < k.T - 1 ? t + k.smooth : k.T - 1;
  i64 n = 0, Wm = 0, Hm = 0, X2 = 0, Y2 = 0;
  for (int u = u0; u <= u1; ++u) {
    const i64* s = col + u * row;
    if (s[0] <= 0) continue;
    ++n;
    Wm = max64(Wm, s[3] - s[1]);
    Hm = max64(Hm, s[4] - s[2]);
    X2 += s[1] + s[3];
    Y2 += s[2] + s[4];
  }
  i64 Wp = max64(k.min_side, Wm + 2 * cdiv64(Wm * k.pad_q, 1024));
  i64 Hp = max64(k.min_side, Hm + 2 * cdiv64(Hm * k.pad_q, 1024));
  if (Wp * k.S_h < Hp * k.S_w)
    Wp = cdiv64(Hp * k.S_w, k.S_h);
  else
    Hp = cdiv64(Wp * k.S_h, k.S_w);
  const i64 wx0 = fdiv64(X2 - n * Wp, 2 * n), wy0 = fdiv64(Y2 - n * Hp, 2 * n);
  const i64 wx1 = wx0 + Wp, wy1 = wy0 + Hp;
  out[0] = wx0;
  out[1] = wy0;
  out[2] = wx1;
  out[3] = wy1;
  out[4] = fdiv64(wx0 * k.W, k.w);
  out[5] = fdiv64(wy0 * k.H, k.h);
  out[6] = cdiv64(wx1 * k.W, k.w);
  out[7] = cdiv64(wy1 * k.H, k.h);
}

__global__ __launch_bounds__(256) void crop_plan_kernel(const CropArgs k) {
  const int per = k.S_w + k.S_h;
  const i64 gid = (i64)blockIdx.x * 256 + threadIdx.x;
  if (gid >= (i64)k.T * k.M * per) return;
  const i64 crop = gid / per;
  const int o = (int)(gid % per);
  const i64* win = k.windows + crop * k.words + (k.words - 4);
  const i64 x0 = win[0], y0 = win[1], x1 = win[2], y1 = win[3];
  if (!crop_window_ok(x0, y0, x1, y1, k)) return;
  const bool vertical = o >= k.S_w;
  const int idx = vertical ? o - k.S_w : o, n = vertical ? k.S_h : k.S_w;
  const i64 a0 = vertical ? y0 : x0, a1 = vertical ? y1 : x1;
  int* tab = k.table + crop * crop_table_ints(k.S_h, k.S_w, k.max_taps);
  int* first = tab + (vertical ? 2 * k.S_w : 0) + idx;
  int* count = first + n;
  int* K = tab + 2 * (size_t)per + ((size_t)(vertical ? k.S_w : 0) + idx) * k.max_taps;

  const double scale = (double)(a1 - a0) / (double)n;
  const double fs = scale > 1.0 ? scale : 1.0;
  const double inv = 1.0 / fs;
  const double center = (double)a0 + ((double)idx + 0.5) * scale;
  const i64 lo = (i64)floor(center - fs + 0.5);
  const i64 hi = (i64)floor(center + fs + 0.5);
  int cnt = (int)(hi - lo);
  cnt = cnt < 0 ? 0 : (cnt > k.max_taps ? k.max_taps : cnt);          // (crop_axis_taps bounds hi - lo: the clamp is a guard, not a rule)
  double ww = 0.0;
  for (int i = 0; i < cnt; ++i) {
    const double a = fabs(((double)(lo + i) - center + 0.5) * inv);
    ww = ww + (a < 1.0 ? 1.0 - a : 0.0);
  }
  for (int i = 0; i < cnt; ++i) {
    const double a = fabs(((double)(lo + i) - center + 0.5) * inv);
    const double v = a < 1.0 ? 1.0 - a : 0.0;
    const double kk = ww != 0.0 ? v / ww : v;
    K[i] = (int)(0.5 + kk * (double)(1 << CROP_BITS));
  }
  *first = (int)lo;
  *count = cnt;
}

__global__ __launch_bounds__(CROP_BLOCK) void crop_resample_kernel(const CropArgs k) {
  extern __shared__ int kx[];                                            // [max_taps][CROP_COLS]
  const int tid = threadIdx.x, col = tid / 3, c = tid - col * 3;
  const int chunks = (k.S_w + CROP_COLS - 1) / CROP_COLS, bands = (k.S_h + CROP_BAND - 1) / CROP_BAND;
  const unsigned bid = blockIdx.x;
  const int chunk = (int)(bid % chunks), band = (int)((bid / chunks) % bands);
  const i64 crop = bid / ((unsigned)chunks * bands);
  const int t = (int)(crop / k.M), j = (int)(crop % k.M);
  const int xx = chunk * CROP_COLS + col;
  const bool active = xx < k.S_w;
  const int y_first = band * CROP_BAND;
  const int nb = k.S_h - y_first < CROP_BAND ? k.S_h - y_first : CROP_BAND;
  const i64* win = k.windows + crop * k.words;
  const i64* fwin = win + (k.words - 4);
  const bool ok = crop_window_ok(fwin[0], fwin[1], fwin[2], fwin[3], k);
  const int fill = c == 0 ? k.fill0 : (c == 1 ? k.fill1 : k.fill2);
  uint8_t* out = k.crops + ((crop * k.S_h + y_first) * k.S_w + xx) * 3 + c;
  const i64 out_row = (i64)k.S_w * 3;

  if (k.masks && active && c == 0) {
    uint8_t* m = k.masks + (crop * k.S_h + y_first) * k.S_w + xx;
    const i64 wx0 = win[0], wy0 = win[1], wx1 = win[2], wy1 = win[3];
    const bool mok = ok && wx1 > wx0 && wy1 > wy0 && max64(max64(abs64(wx0), abs64(wy0)), max64(abs64(wx1), abs64(wy1))) < CROP_LIMIT;
    const int obj = k.objects[j];
    const i64 mx = mok ? wx0 + ((2 * (i64)xx + 1) * (wx1 - wx0)) / (2 * (i64)k.S_w) : -1;          // (the numerator is positive)
    for (int b = 0; b < nb; ++b) {
      uint8_t v = 0;
      if (mok) {
        const i64 my = wy0 + ((2 * (i64)(y_first + b) + 1) * (wy1 - wy0)) / (2 * (i64)k.S_h);
        if (mx >= 0 && mx < k.w && my >= 0 && my < k.h) v = k.ids[t * k.ids_st + my * k.ids_sy + mx] == obj ? 255 : 0;
      }
      m[(i64)b * k.S_w] = v;
    }
  }

  if (!ok) {
    if (active)
      for (int b = 0; b < nb; ++b) out[b * out_row] = (uint8_t)fill;
    return;
  }

  const int* tab = k.table + crop * crop_table_ints(k.S_h, k.S_w, k.max_taps);
  const int* ky = tab + 2 * (size_t)(k.S_w + k.S_h) + ((size_t)k.S_w + y_first) * k.max_taps;
  const int my_lo = active ? tab[xx] : 0, my_cnt = active ? tab[k.S_w + xx] : 0;
  {
    const int* src = tab + 2 * (size_t)(k.S_w + k.S_h) + (size_t)xx * k.max_taps;
    for (int i = c; i < my_cnt; i += 3) kx[i * CROP_COLS + col] = src[i];
  }
  int lo_b[CROP_BAND], cnt_b[CROP_BAND], acc[CROP_BAND];
#pragma unroll
  for (int b = 0; b < CROP_BAND; ++b) {
    const bool have = b < nb;
    lo_b[b] = have ? tab[2 * k.S_w + y_first + b] : 0;
    cnt_b[b] = have ? tab[2 * k.S_w + k.S_h + y_first + b] : 0;
    acc[b] = 0;
  }
  __syncthreads();

  // the first taps do not decrease with the output index, nor do the ends: the band's source rows are [r0, r1)
  int r0 = lo_b[0], r1 = lo_b[0] + cnt_b[0];
#pragma unroll
  for (int b = 1; b < CROP_BAND; ++b)
    if (b < nb) {
      r0 = imin(r0, lo_b[b]);
      r1 = imax(r1, lo_b[b] + cnt_b[b]);
    }
  const uint8_t* frame = k.frames + t * k.st + c * k.sc;
  for (int r = r0; r < r1; ++r) {
    const bool row_in = r >= 0 && r < k.H;
    const uint8_t* line = frame + (i64)(row_in ? r : 0) * k.sy;
    int sum = 0;
    for (int i = 0; i < my_cnt; ++i) {
      const int sx = my_lo + i;
      const int px = (row_in && (unsigned)sx < (unsigned)k.W) ? (int)line[sx * k.sx] : fill;
      sum += kx[i * CROP_COLS + col] * px;
    }
    const int hv = clip8_round(sum);
#pragma unroll
    for (int b = 0; b < CROP_BAND; ++b) {
      const int d = r - lo_b[b];
      if (d >= 0 && d < cnt_b[b]) acc[b] += ky[b * k.max_taps + d] * hv;
    }
  }
  if (active) {
#pragma unroll
    for (int b = 0; b < CROP_BAND; ++b)
      if (b < nb) out[b * out_row] = (uint8_t)clip8_round(acc[b]);
  }
}

int object_windows_launch(const int64_t* stats, int T, int N, const int32_t* objects, int M, int S_h, int S_w, int pad_q, int min_side, int smooth,
                          int h, int w, int H, int W, int64_t* windows, hipStream_t s) {
  WinArgs a;
  a.stats = reinterpret_cast<const i64*>(stats); a.objects = objects; a.out = reinterpret_cast<i64*>(windows);
  a.T = T; a.N = N; a.M = M; a.S_h = S_h; a.S_w = S_w; a.pad_q = pad_q; a.min_side = min_side; a.smooth = smooth;
  a.h = h; a.w = w; a.H = H; a.W = W;
  const long long n = (long long)T * M;
  object_windows_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_seg_object_windows_i64");
  return FGVC_OK;
}

size_t object_crops_workspace_bytes(int T, int M, int S_h, int S_w, int max_taps) {
  return (size_t)T * (size_t)M * crop_table_ints(S_h, S_w, max_taps) * sizeof(int);
}

// the workgroups of the two launches; 0 where either does not fit a 32-bit grid
long long object_crops_blocks(int T, int M, int S_h, int S_w) {
  const long long crops = (long long)T * M;
  const long long plan = (crops * (S_h + S_w) + 255) / 256;
  const long long res = crops * ((S_w + CROP_COLS - 1) / CROP_COLS) * ((S_h + CROP_BAND - 1) / CROP_BAND);
  return (plan < (1ll << 31) && res < (1ll << 31)) ? res : 0;
}

int object_crops_launch(const uint8_t* frames, int T, int H, int W, long long st, long long sy, long long sx, long long sc, const int64_t* windows,
                        int words, int M, int S_h, int S_w, int fill0, int fill1, int fill2, const uint8_t* ids, long long ids_st,
                        long long ids_sy, int h, int w, const int32_t* objects, int max_taps, uint8_t* crops, uint8_t* masks, void* workspace,
                        hipStream_t s) {
  CropArgs a;
  a.frames = frames; a.st = st; a.sy = sy; a.sx = sx; a.sc = sc;
  a.windows = reinterpret_cast<const i64*>(windows);
  a.ids = ids; a.ids_st = ids_st; a.ids_sy = ids_sy; a.objects = objects;
  a.crops = crops; a.masks = masks; a.table = static_cast<int*>(workspace);
  a.T = T; a.H = H; a.W = W; a.M = M; a.words = words; a.S_h = S_h; a.S_w = S_w; a.h = h; a.w = w; a.max_taps = max_taps;
  a.fill0 = fill0; a.fill1 = fill1; a.fill2 = fill2;
  const long long crops_n = (long long)T * M;
  crop_plan_kernel<<<dim3((unsigned)((crops_n * (S_h + S_w) + 255) / 256)), 256, 0, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_frames_object_crops_u8 (plan)");
  const size_t lds = (size_t)max_taps * CROP_COLS * sizeof(int);
  crop_resample_kernel<<<dim3((unsigned)object_crops_blocks(T, M, S_h, S_w)), CROP_BLOCK, lds, s>>>(a);
  FGVC_CHECK_LAUNCH("fgvc_frames_object_crops_u8");
  return FGVC_OK;
}

}  // namespace fgvc
