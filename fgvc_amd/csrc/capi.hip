// extern "C" surface of libfgvc_hip.so (see include/fgvc_hip.h): argument validation, then launch.
// Shapes are validated HERE, on the host, before any hand-written kernel is enqueued: a grid that
// does not match its operands can fault the GPU.
#include <stdarg.h>
#include <string.h>

#include "common.hpp"
#include "render_host.hpp"

namespace fgvc {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int pair_topk_launch(const float*, const float*, const int32_t*, int, int, int, int, int, int, int, int, int, int,
                     const uint8_t*, int32_t*, float*, hipStream_t);
int merge_topk_launch(const int32_t*, const float*, const int32_t*, int, int, int, int, int, float, int, int32_t*,
                      float*, float*, hipStream_t);
int normalize_launch(const float*, float*, int, int, int, int, int, hipStream_t);
int propagate_launch(const float*, const int32_t*, int, const int32_t*, const float*, int, int, int, int, int, int,
                     int, float*, hipStream_t);
int bn_act_launch(const float*, const float*, const float*, const float*, const float*, const float*, float, int, float*,
                  int, int, int, hipStream_t);
int gaussian_launch(const float*, int, int, int, int, float, float*, hipStream_t);
int softargmax_launch(const float*, int, int, int, int, int, int, const float*, float, double*, float*, hipStream_t);
int softargmax_bands();
int corr_volume_f32_launch(const float*, const float*, int, int, int, float, float*, hipStream_t);
int split_bf16_launch(const float*, uint16_t*, long long, int, hipStream_t);
int corr_volume_bf16_launch(const uint16_t*, const uint16_t*, int, int, int, float, float*, int, hipStream_t);
int local_merge_launch(const int32_t*, const float*, int, int, int, int, int, float, int32_t*, float*, float*,
                       hipStream_t);
int local_merge_plan_launch(const int32_t*, const float*, const int32_t*, int, int, int, int, int, int, int, float, int32_t*, float*,
                            float*, hipStream_t);
int topk_coord_launch(const int32_t*, const float*, int, int, int, int, int, float*, hipStream_t);
int topk_coord_rows_launch(const int32_t*, const float*, int, int, int, int, int, int, float*, hipStream_t);
int cycle_chase_launch(const float*, const float*, const float*, int, int, int, int, int, float*, float*, hipStream_t);
int flow_from_lists_launch(const int32_t*, const float*, int, int, int, int, int, int, int, int, int, int, int, float*, uint8_t*, hipStream_t);
int flow_consistency_launch(const float*, const float*, int, int, int, int, float, float*, float*, hipStream_t);
int warp_launch(const float*, const float*, int, int, int, int, int, int, float*, hipStream_t);
int flow_chain_launch(const float*, const float*, const uint8_t*, const uint8_t*, const float*, int, int, int, int, int, float*, uint8_t*,
                      hipStream_t);
int frames_rgb8_to_lab_launch(const uint8_t*, int, int, int, long long, long long, long long, long long, int, int, int, int, int, int, float*,
                              hipStream_t);
int frames_yuv_to_lab_launch(const char*, bool, const void*, const void*, const void*, int, int, int, int, int, int, int, int, long long, long long,
                             long long, long long, long long, const float*, int, int, int, int, int, int, int, float*, hipStream_t);
int frames_yuv_to_rgb8_launch(const char*, bool, const void*, const void*, const void*, int, int, int, int, int, int, int, int, long long,
                              long long, long long, long long, long long, const float*, int, uint8_t*, hipStream_t);
int frames_rgb8_to_yuv420_launch(const uint8_t*, int, int, int, long long, long long, long long, long long, uint8_t*, long long, long long,
                                 uint8_t*, uint8_t*, long long, long long, long long, const float*, int, hipStream_t);
void yuv_out_tile(int*, int*);
int jf_counts_launch(const uint8_t*, const uint8_t*, int, int, int, int, int, int64_t*, hipStream_t);
int jf_tile_rows();
int object_stats_launch(const uint8_t*, long long, long long, int, int, int, int, int64_t*, hipStream_t);
int components_launch(const uint8_t*, long long, long long, int, int, int, int, int, int32_t*, hipStream_t);
int clean_launch(const uint8_t*, long long, long long, int, int, int, int, int, int, int, int, long long, const uint8_t*, uint8_t*, long long,
                 long long, int64_t*, void*, hipStream_t);
void ccl_tile(int*, int*);
long long ccl_blocks(int, int, int);
size_t clean_workspace_bytes(int, int, int, int);
int object_windows_launch(const int64_t*, int, int, const int32_t*, int, int, int, int, int, int, int, int, int, int, int64_t*, hipStream_t);
size_t object_crops_workspace_bytes(int, int, int, int, int);
long long object_crops_blocks(int, int, int, int);
int object_crops_launch(const uint8_t*, int, int, int, long long, long long, long long, long long, const int64_t*, int, int, int, int, int, int, int,
                        const uint8_t*, long long, long long, int, int, const int32_t*, int, uint8_t*, uint8_t*, void*, hipStream_t);
int c2f_refine_launch(const int32_t*, const float*, const float*, const float*, int, int, int, int, int, int, int,
                      int, float, int, float*, int32_t*, float*, hipStream_t);

int conv_split_launch(const uint16_t*, const uint16_t*, const float*, const float*, uint16_t*, float*, int, int, int, int, int,
                      int, int, int, int, int, int, int, int, int*, hipStream_t, unsigned char* y_bank = nullptr, int bank_normalize = 1, const uint16_t* x2 = nullptr,
                      const uint16_t* w2 = nullptr, int Cin2 = 0, int bank_row_bytes = 1024);
int conv_s2_launch(const uint16_t*, const uint16_t*, const float*, uint16_t*, float*, int, int, int, int, int, int, int, int, int,
                   int, int, int, int, int*, const uint16_t*, const float*, float*, int, hipStream_t);
int conv64_launch(const uint16_t*, const uint16_t*, const float*, const float*, const uint16_t*, uint16_t*, float*, int, int, int, int, int, int,
                  int, int, int, int, int*, hipStream_t);
int stem7_launch(const float*, const uint16_t*, const float*, uint16_t*, float*, int, int, int, int, int, int, int, int, int, int, int*,
                 hipStream_t);
int nchw_to_split_nhwc_launch(const float*, uint16_t*, float*, int, int, int, int, int, int, hipStream_t);
int normalize_nhwc_launch(const float*, float*, uint16_t*, int, int, int, int, int, int, hipStream_t);
int nhwc_to_split_launch(float*, uint16_t*, int, int, int, int, int, int, int, hipStream_t);

void set_conv_cot_cap(int);
void set_conv_narrow(int);
void set_conv64_variant(int);
int conv64_probe_read(long long*);
void set_conv_debug(int);
void set_corr6_skew(int);
void set_corr6_sdma(int);
void set_pair_debug(int);
void set_readout_prune(int);
void set_conv_s2_debug(int);
int split_f16x2_launch(const float*, uint16_t*, long long, int, hipStream_t);
int split_f16f6p_launch(const float*, unsigned char*, long long, int, hipStream_t);
int pair_topk_v7_launch(const uint16_t*, const uint16_t*, const int32_t*, int, int, int, int, int, int, int, int, int, const int32_t*, int,
                        int32_t*, float*, int, hipStream_t);
int pair_topk_v5_launch(const uint16_t*, const uint16_t*, const int32_t*, int, int, int, int, int, int, int, int, int, int, const int32_t*,
                        int, int32_t*, float*, hipStream_t);
void set_pair_v5_debug(int);
int pair_v5_timeout_flag();
int pair_v5_probe_read(long long*);
void set_corr_debug(int);
int split_f16f8_launch(const float*, unsigned char*, long long, int, hipStream_t);
int corr_volume_f16f8_launch(const unsigned char*, const unsigned char*, int, int, float, float*, hipStream_t);
void set_corr8_debug(int);
int split_f16f6_launch(const float*, unsigned char*, long long, hipStream_t);
int corr_volume_f16f6_launch(const unsigned char*, const unsigned char*, int, int, float, float*, hipStream_t);
void set_corr6_debug(int);
int store_sweep_launch(float*, long long, int, hipStream_t);
int dense_attend_splits(int, int);
int dense_attend_launch(const float*, const float*, int, int, int, int, int, int, int, int, int, int, int, float*, int, hipStream_t, const float*);
int dense_kth_launch(const float*, int, int, int, float*, int, float*, hipStream_t);
int dense_attend_finish_launch(const float*, int, int, int, int, float*, hipStream_t);

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace fgvc

using namespace fgvc;

extern "C" {

const char* fgvc_version(void) { return "fgvc_hip 0.1 (gfx950)"; }
const char* fgvc_last_error(void) { return g_err; }

// The profiling ablations (a kernel without its stores, its matrix chain, its selection ...) return WRONG results.  The production
// library refuses to switch them on: the bits below are accepted only by the build with -DFGVC_ABLATIONS (libfgvc_hip_ablations.so,
// `python -m fgvc_amd.build` makes both from the same objects but this file; tools/experiments select it with FGVC_HIP_LIB).  What
// the production library still takes are A/B switches between forms with IDENTICAL results, the s_memtime probes, and the fault
// injection of the fail-closed test (poison lists + the device flag: not a result anybody can mistake for one).
static int ablation_bits(const char* name, int value) {
  if (strcmp(name, "corr_debug") == 0 || strcmp(name, "pair_debug") == 0 || strcmp(name, "conv_s2_debug") == 0) return value;
  if (strcmp(name, "corr8_debug") == 0) return value & (1 | 2);
  if (strcmp(name, "corr6_debug") == 0) return value & (1 | 2 | 256 | 512 | 1024);
  if (strcmp(name, "conv_debug") == 0) return value & (1 | 2 | 4);
  if (strcmp(name, "pair_f16_debug") == 0)
    return value & ((value & 4194304) ? (1 | 2 | 524288 | 1048576) : (1 | 2 | 4 | 8 | 16 | 32 | 64 | 2048 | 524288 | 1048576));
  return 0;
}

int fgvc_set_option(const char* name, int value) {
  FGVC_REQUIRE(name != nullptr, FGVC_ERR_INVALID_ARG, "fgvc_set_option: null name");
#ifndef FGVC_ABLATIONS
  FGVC_REQUIRE(ablation_bits(name, value) == 0, FGVC_ERR_UNSUPPORTED,
               "fgvc_set_option: %s = %d switches a profiling ablation on (bits %d: results would be wrong); this library is built without them -- "
               "use libfgvc_hip_ablations.so (FGVC_HIP_LIB)", name, value, ablation_bits(name, value));
#endif
  if (strcmp(name, "corr_debug") == 0) {   // profiling ablation: 1 = bf16 volume kernels skip their stores
    set_corr_debug(value);
    return FGVC_OK;
  }
  if (strcmp(name, "corr8_debug") == 0) {   // fgvc_corr_volume_f16f8 ablations: 1 = no stores, 2 = no MFMA (results wrong); 4 = no row
    set_corr8_debug(value);                 // classes, 8 = wave stagger, 16 = the 32x32-shape kernel (results right); >> 8 = key blocks per workgroup
    return FGVC_OK;
  }
  if (strcmp(name, "corr6_debug") == 0) {   // fgvc_corr_volume_f16f6 ablations: 1 = no stores, 2 = no MFMA, 4 = no row classes, 8 = no stagger, ...; >> 12 = half-chunks per tile pair
    set_corr6_debug(value);
    return FGVC_OK;
  }
  if (strcmp(name, "pair_debug") == 0) {   // profiling ablations; results are wrong when non-zero
    set_pair_debug(value);
    return FGVC_OK;
  }
  if (strcmp(name, "corr6_sdma") == 0) {   // A/B: staging DMAs of fgvc_corr_volume_f16f6 with a scalar base (1) or 64-bit lane addresses (0)
    set_corr6_sdma(value);
    return FGVC_OK;
  }
  if (strcmp(name, "corr6_skew") == 0) {   // fgvc_corr_volume_f16f6: stages taken from the two-segment piece and given to the others
    set_corr6_skew(value);
    return FGVC_OK;
  }
  if (strcmp(name, "conv_debug") == 0) {   // profiling ablations of fgvc_conv_split_f32; results are wrong when non-zero
    set_conv_debug(value);
    return FGVC_OK;
  }
  if (strcmp(name, "conv64_variant") == 0) {   // A/B bits of fgvc_conv64_split_f32 (csrc/conv64.hip)
    set_conv64_variant(value);
    return FGVC_OK;
  }
  if (strcmp(name, "conv_narrow") == 0) {   // fgvc_conv_split_f32 with 64 output channels per workgroup: 1 (default) = 4-row tiles,
    set_conv_narrow(value);                 // two workgroups per CU;  0 = 8-row tiles, one workgroup per CU;  +2 = the same for 128
    return FGVC_OK;
  }
  if (strcmp(name, "conv_cot_cap") == 0) {   // fgvc_conv_split_f32: at most this many output channels per workgroup (0, 64, 128)
    FGVC_REQUIRE(value == 0 || value == 64 || value == 128, FGVC_ERR_INVALID_ARG, "fgvc_set_option: conv_cot_cap must be 0, 64 or 128");
    set_conv_cot_cap(value);
    return FGVC_OK;
  }
  if (strcmp(name, "pair_f16_debug") == 0) {   // fgvc_pair_topk_f16x3 ablations (results wrong): 1 = no selection, 2 = no MFMA, 4 = no staging,
    set_pair_v5_debug(value);                  // 16 = prologue only, 32 = no epilogue, 64 = no main loop
    return FGVC_OK;
  }
  if (strcmp(name, "conv_s2_debug") == 0) {   // profiling ablations of fgvc_conv_s2_split_f32; results are wrong when non-zero
    set_conv_s2_debug(value);
    return FGVC_OK;
  }
  if (strcmp(name, "readout_prune") == 0) {   // fgvc_softargmax_top5_f32: 1 (default) = pruned read-out first, full scan only for
    set_readout_prune(value != 0);            // the maps it hands back;  0 = full scan of every map (same results)
    return FGVC_OK;
  }
  set_error("fgvc_set_option: unknown option '%s'", name);
  return FGVC_ERR_INVALID_ARG;
}

int fgvc_r2max_for_radius(float radius) {
  if (!(radius > 0.f)) return -1;
  long long d2 = (long long)ceil((double)radius * (double)radius) + 2;
  if (d2 > FGVC_NO_LIMIT) return FGVC_NO_LIMIT;
  while (d2 >= 0 && !(sqrtf((float)d2) < radius)) --d2;
  return (int)d2;
}

int fgvc_normalize_chw_to_hwc_f32(const float* in, float* out, int n, int C, int HW, int normalize, int c_out,
                                  void* stream) {
  FGVC_REQUIRE(in && out, FGVC_ERR_INVALID_ARG, "fgvc_normalize_chw_to_hwc_f32: null pointer");
  FGVC_REQUIRE(n >= 0 && C > 0 && HW > 0, FGVC_ERR_INVALID_ARG, "fgvc_normalize_chw_to_hwc_f32: bad shape n=%d C=%d HW=%d", n, C, HW);
  FGVC_REQUIRE(C <= 1024, FGVC_ERR_UNSUPPORTED, "fgvc_normalize_chw_to_hwc_f32: C=%d > 1024 (LDS tile)", C);
  FGVC_REQUIRE(n <= 65535, FGVC_ERR_UNSUPPORTED, "fgvc_normalize_chw_to_hwc_f32: n=%d > 65535 frames per call", n);
  FGVC_REQUIRE(c_out >= C, FGVC_ERR_INVALID_ARG, "fgvc_normalize_chw_to_hwc_f32: c_out=%d < C=%d", c_out, C);
  if (n == 0) return FGVC_OK;
  return normalize_launch(in, out, n, C, HW, normalize, c_out, (hipStream_t)stream);
}

int fgvc_pair_topk_f32(const float* qfeat, const float* kfeat, const int32_t* pairs, int n_pairs, int C, int Hq,
                       int Wq, int Hk, int Wk, int r2max, int ry, int rx, int topk, const uint8_t* dense_mask,
                       int32_t* idx_out, float* score_out, void* stream) {
  FGVC_REQUIRE(qfeat && kfeat && pairs && idx_out && score_out, FGVC_ERR_INVALID_ARG, "fgvc_pair_topk_f32: null pointer");
  FGVC_REQUIRE(aligned16(qfeat) && aligned16(kfeat) && aligned16(pairs), FGVC_ERR_INVALID_ARG,
               "fgvc_pair_topk_f32: qfeat/kfeat/pairs must be 16-byte aligned");
  FGVC_REQUIRE(Hq > 0 && Wq > 0 && Hk > 0 && Wk > 0 && n_pairs >= 0, FGVC_ERR_INVALID_ARG,
               "fgvc_pair_topk_f32: bad shape Hq=%d Wq=%d Hk=%d Wk=%d n_pairs=%d", Hq, Wq, Hk, Wk, n_pairs);
  FGVC_REQUIRE(topk >= 1 && topk <= 16, FGVC_ERR_UNSUPPORTED, "fgvc_pair_topk_f32: topk=%d outside 1..16", topk);
  FGVC_REQUIRE(r2max >= 0 && ry >= 0 && rx >= 0, FGVC_ERR_INVALID_ARG, "fgvc_pair_topk_f32: negative mask parameter");
  FGVC_REQUIRE(n_pairs <= 65535, FGVC_ERR_UNSUPPORTED, "fgvc_pair_topk_f32: n_pairs=%d > 65535 per call", n_pairs);
  const bool any_limit = r2max < FGVC_NO_LIMIT || ry < FGVC_NO_LIMIT || rx < FGVC_NO_LIMIT;
  FGVC_REQUIRE(!any_limit || (Hq == Hk && Wq == Wk), FGVC_ERR_INVALID_ARG,
               "fgvc_pair_topk_f32: a spatial mask needs equal query/key grids (local_attention.py:331)");
  FGVC_REQUIRE((long long)Hk * Wk < (1ll << 30) && (long long)Hq * Wq < (1ll << 30), FGVC_ERR_UNSUPPORTED,
               "fgvc_pair_topk_f32: grid too large");
  if (n_pairs == 0) return FGVC_OK;
  FGVC_REQUIRE(dense_mask == nullptr || !any_limit, FGVC_ERR_INVALID_ARG,
               "fgvc_pair_topk_f32: give either the analytic predicate or a dense mask, not both");
  return pair_topk_launch(qfeat, kfeat, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, dense_mask, idx_out,
                          score_out, (hipStream_t)stream);
}

int fgvc_split_f16x2(const float* feat, uint16_t* h_l, int64_t n_pixels, int C, void* stream) {
  FGVC_REQUIRE(feat && h_l, FGVC_ERR_INVALID_ARG, "fgvc_split_f16x2: null pointer");
  FGVC_REQUIRE(n_pixels >= 0 && C > 0 && C % 4 == 0, FGVC_ERR_INVALID_ARG, "fgvc_split_f16x2: C must be a multiple of 4");
  FGVC_REQUIRE(aligned16(feat) && aligned16(h_l), FGVC_ERR_INVALID_ARG, "fgvc_split_f16x2: 16-byte alignment required");
  if (n_pixels == 0) return FGVC_OK;
  return split_f16x2_launch(feat, h_l, n_pixels, C, (hipStream_t)stream);
}

static int pair_f16x3_common(const char* what, const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_pairs, int C,
                             int Hq, int Wq, int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs,
                             int n_runs, int32_t* idx_out, float* score_out, void* stream) {
  FGVC_REQUIRE(qsplit && ksplit && pairs && idx_out && score_out, FGVC_ERR_INVALID_ARG, "%s: null pointer", what);
  FGVC_REQUIRE(aligned16(qsplit) && aligned16(ksplit) && aligned16(pairs), FGVC_ERR_INVALID_ARG,
               "%s: qsplit/ksplit/pairs must be 16-byte aligned", what);
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "%s: C=%d unsupported (256 only; use fgvc_pair_topk_f32)", what, C);
  FGVC_REQUIRE(Hq > 0 && Wq > 0 && Hk > 0 && Wk > 0 && n_pairs >= 0, FGVC_ERR_INVALID_ARG,
               "%s: bad shape Hq=%d Wq=%d Hk=%d Wk=%d n_pairs=%d", what, Hq, Wq, Hk, Wk, n_pairs);
  FGVC_REQUIRE(topk >= 1 && topk <= 10, FGVC_ERR_UNSUPPORTED, "%s: topk=%d outside 1..10", what, topk);
  FGVC_REQUIRE(r2max >= 0 && ry >= 0 && rx >= 0, FGVC_ERR_INVALID_ARG, "%s: negative mask parameter", what);
  FGVC_REQUIRE(n_pairs <= 65535, FGVC_ERR_UNSUPPORTED, "%s: n_pairs=%d > 65535 per call", what, n_pairs);
  FGVC_REQUIRE(!runs || (n_runs >= 1 && n_runs <= n_pairs && (reinterpret_cast<uintptr_t>(runs) & 7u) == 0), FGVC_ERR_INVALID_ARG,
               "%s: runs must be 8-byte aligned, 1 <= n_runs <= n_pairs", what);
  const bool any_limit = r2max < FGVC_NO_LIMIT || ry < FGVC_NO_LIMIT || rx < FGVC_NO_LIMIT;
  FGVC_REQUIRE(!any_limit || (Hq == Hk && Wq == Wk), FGVC_ERR_INVALID_ARG,
               "%s: a spatial mask needs equal query/key grids (local_attention.py:331)", what);
  FGVC_REQUIRE(Hk < 32768 && Wk < 32768 && Hq < 32768 && Wq < 32768 && (long long)Hk * Wk < (1ll << 30) &&
                   (long long)Hq * Wq < (1ll << 30),
               FGVC_ERR_UNSUPPORTED, "%s: grid too large", what);
  if (n_pairs == 0) return FGVC_OK;
  return pair_topk_v5_launch(qsplit, ksplit, pairs, n_pairs, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked != 0 && any_limit, runs,
                             n_runs, idx_out, score_out, (hipStream_t)stream);
}

int fgvc_pair_topk_f16x3(const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq,
                         int Wq, int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, int32_t* idx_out,
                         float* score_out, void* stream) {
  return pair_f16x3_common("fgvc_pair_topk_f16x3", qsplit, ksplit, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked,
                           nullptr, 0, idx_out, score_out, stream);
}

int fgvc_pair_topk_f16x3_runs(const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq,
                              int Wq, int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs,
                              int n_runs, int32_t* idx_out, float* score_out, void* stream) {
  FGVC_REQUIRE(runs, FGVC_ERR_INVALID_ARG, "fgvc_pair_topk_f16x3_runs: null runs");
  return pair_f16x3_common("fgvc_pair_topk_f16x3_runs", qsplit, ksplit, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked,
                           runs, n_runs, idx_out, score_out, stream);
}

int fgvc_split_f16f6p(const float* feat, uint8_t* rows, int64_t n_pixels, int C, void* stream) {
  FGVC_REQUIRE(feat && rows, FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6p: null pointer");
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_split_f16f6p: C=%d unsupported (256 only)", C);
  FGVC_REQUIRE(n_pixels >= 0 && n_pixels < (1ll << 40), FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6p: bad n_pixels");
  FGVC_REQUIRE(aligned16(feat) && aligned16(rows), FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6p: 16-byte alignment required");
  if (n_pixels == 0) return FGVC_OK;
  return split_f16f6p_launch(feat, rows, n_pixels, 1024, (hipStream_t)stream);
}

int fgvc_split_f16f6x(const float* feat, uint8_t* rows, int64_t n_pixels, int C, void* stream) {
  FGVC_REQUIRE(feat && rows, FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6x: null pointer");
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_split_f16f6x: C=%d unsupported (256 only)", C);
  FGVC_REQUIRE(n_pixels >= 0 && n_pixels < (1ll << 40), FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6x: bad n_pixels");
  FGVC_REQUIRE(aligned16(feat) && aligned16(rows), FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6x: 16-byte alignment required");
  if (n_pixels == 0) return FGVC_OK;
  return split_f16f6p_launch(feat, rows, n_pixels, 2048, (hipStream_t)stream);
}

static int pair_f16f6_common(const char* what, const uint8_t* qsplit, const uint8_t* ksplit, const int32_t* pairs, int n_pairs, int C,
                             int Hq, int Wq, int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs,
                             int n_runs, int32_t* idx_out, float* score_out, void* stream, int row_bytes = 1024) {
  FGVC_REQUIRE(qsplit && ksplit && pairs && idx_out && score_out, FGVC_ERR_INVALID_ARG, "%s: null pointer", what);
  FGVC_REQUIRE(aligned16(qsplit) && aligned16(ksplit) && aligned16(pairs), FGVC_ERR_INVALID_ARG,
               "%s: qsplit/ksplit/pairs must be 16-byte aligned", what);
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "%s: C=%d unsupported (256 only; use fgvc_pair_topk_f32)", what, C);
  FGVC_REQUIRE(Hq > 0 && Wq > 0 && Hk > 0 && Wk > 0 && n_pairs >= 0, FGVC_ERR_INVALID_ARG,
               "%s: bad shape Hq=%d Wq=%d Hk=%d Wk=%d n_pairs=%d", what, Hq, Wq, Hk, Wk, n_pairs);
  FGVC_REQUIRE(topk >= 1 && topk <= 10, FGVC_ERR_UNSUPPORTED, "%s: topk=%d outside 1..10", what, topk);
  FGVC_REQUIRE(r2max >= 0 && ry >= 0 && rx >= 0, FGVC_ERR_INVALID_ARG, "%s: negative mask parameter", what);
  FGVC_REQUIRE(n_pairs <= 65535, FGVC_ERR_UNSUPPORTED, "%s: n_pairs=%d > 65535 per call", what, n_pairs);
  FGVC_REQUIRE(!runs || (n_runs >= 1 && n_runs <= n_pairs && (reinterpret_cast<uintptr_t>(runs) & 7u) == 0), FGVC_ERR_INVALID_ARG,
               "%s: runs must be 8-byte aligned, 1 <= n_runs <= n_pairs", what);
  const bool any_limit = r2max < FGVC_NO_LIMIT || ry < FGVC_NO_LIMIT || rx < FGVC_NO_LIMIT;
  FGVC_REQUIRE(any_limit && all_masked != 0, FGVC_ERR_UNSUPPORTED,
               "%s: every pair must carry FGVC_PAIR_MASKED under an analytic mask (a pair that scans the whole frame needs fgvc_pair_topk_f16x3)", what);
  FGVC_REQUIRE(Hq == Hk && Wq == Wk, FGVC_ERR_INVALID_ARG, "%s: a spatial mask needs equal query/key grids (local_attention.py:331)", what);
  FGVC_REQUIRE(Hk < 16384 && Wk < 32768 && (long long)Hk * Wk < (1ll << 30), FGVC_ERR_UNSUPPORTED, "%s: grid too large", what);
  if (n_pairs == 0) return FGVC_OK;
  return pair_topk_v7_launch(reinterpret_cast<const uint16_t*>(qsplit), reinterpret_cast<const uint16_t*>(ksplit), pairs, n_pairs, Hq, Wq, Hk, Wk,
                             r2max, ry, rx, topk, runs, n_runs, idx_out, score_out, row_bytes, (hipStream_t)stream);
}

int fgvc_pair_topk_f16f6(const uint8_t* qsplit, const uint8_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq, int Hk,
                         int Wk, int r2max, int ry, int rx, int topk, int all_masked, int32_t* idx_out, float* score_out, void* stream) {
  return pair_f16f6_common("fgvc_pair_topk_f16f6", qsplit, ksplit, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked,
                           nullptr, 0, idx_out, score_out, stream);
}

int fgvc_pair_topk_f16f6_runs(const uint8_t* qsplit, const uint8_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq,
                              int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs, int n_runs,
                              int32_t* idx_out, float* score_out, void* stream) {
  FGVC_REQUIRE(runs, FGVC_ERR_INVALID_ARG, "fgvc_pair_topk_f16f6_runs: null runs");
  return pair_f16f6_common("fgvc_pair_topk_f16f6_runs", qsplit, ksplit, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked,
                           runs, n_runs, idx_out, score_out, stream);
}

int fgvc_pair_topk_f16f6x(const uint8_t* qrows, const uint8_t* krows, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq, int Hk,
                          int Wk, int r2max, int ry, int rx, int topk, int all_masked, int32_t* idx_out, float* score_out, void* stream) {
  return pair_f16f6_common("fgvc_pair_topk_f16f6x", qrows, krows, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked,
                           nullptr, 0, idx_out, score_out, stream, 2048);
}

int fgvc_pair_topk_f16f6x_runs(const uint8_t* qrows, const uint8_t* krows, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq,
                               int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs, int n_runs,
                               int32_t* idx_out, float* score_out, void* stream) {
  FGVC_REQUIRE(runs, FGVC_ERR_INVALID_ARG, "fgvc_pair_topk_f16f6x_runs: null runs");
  return pair_f16f6_common("fgvc_pair_topk_f16f6x_runs", qrows, krows, pairs, n_pairs, C, Hq, Wq, Hk, Wk, r2max, ry, rx, topk, all_masked,
                           runs, n_runs, idx_out, score_out, stream, 2048);
}

/* debug: the 32 s_memtime words one workgroup leaves with fgvc_set_option("pair_f16_debug", 256) (tools/experiments/time_pair_v5.py) */
int fgvc_pair_topk_f16x3_probe(int64_t* out32) {
  if (!out32 || hipDeviceSynchronize() != hipSuccess) return FGVC_ERR_INVALID_ARG;
  return pair_v5_probe_read(reinterpret_cast<long long*>(out32)) == 0 ? FGVC_OK : FGVC_ERR_LAUNCH;
}

int fgvc_pair_topk_f16x3_timed_out(void) {
  if (hipDeviceSynchronize() != hipSuccess) return -1;
  return pair_v5_timeout_flag();
}

int fgvc_merge_topk_f32(const int32_t* pair_idx, const float* pair_score, const int32_t* slot_pair, int n_out, int T,
                        int HWq, int HWk, int topk, float temperature, int weight_mode, int32_t* idx_out,
                        float* logit_out, float* weight_out, void* stream) {
  FGVC_REQUIRE(pair_idx && pair_score && slot_pair && idx_out && logit_out && weight_out, FGVC_ERR_INVALID_ARG,
               "fgvc_merge_topk_f32: null pointer");
  FGVC_REQUIRE(n_out >= 0 && T >= 1 && HWq > 0 && HWk > 0, FGVC_ERR_INVALID_ARG, "fgvc_merge_topk_f32: bad shape");
  FGVC_REQUIRE(topk >= 1 && topk <= 16, FGVC_ERR_UNSUPPORTED, "fgvc_merge_topk_f32: topk=%d outside 1..16", topk);
  FGVC_REQUIRE((long long)T * HWk < (1ll << 31), FGVC_ERR_UNSUPPORTED, "fgvc_merge_topk_f32: T*HWk overflows int32");
  FGVC_REQUIRE(temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_merge_topk_f32: temperature must be > 0");
  FGVC_REQUIRE(weight_mode == FGVC_WEIGHT_SOFTMAX || weight_mode == FGVC_WEIGHT_COSINE, FGVC_ERR_INVALID_ARG,
               "fgvc_merge_topk_f32: unknown weight mode %d", weight_mode);
  FGVC_REQUIRE(n_out <= 65535, FGVC_ERR_UNSUPPORTED, "fgvc_merge_topk_f32: n_out=%d > 65535", n_out);
  if (n_out == 0) return FGVC_OK;
  return merge_topk_launch(pair_idx, pair_score, slot_pair, n_out, T, HWq, HWk, topk, temperature, weight_mode,
                           idx_out, logit_out, weight_out, (hipStream_t)stream);
}

int fgvc_propagate_topk_f32(const float* labels, const int32_t* slot_frame, int T, const int32_t* idx,
                            const float* weight, int Hq, int Wq, int Hk, int Wk, int P, int topk, int window_L,
                            float* out, void* stream) {
  FGVC_REQUIRE(labels && slot_frame && idx && weight && out, FGVC_ERR_INVALID_ARG, "fgvc_propagate_topk_f32: null pointer");
  FGVC_REQUIRE(T >= 1 && Hq > 0 && Wq > 0 && Hk > 0 && Wk > 0 && P > 0 && topk >= 1, FGVC_ERR_INVALID_ARG,
               "fgvc_propagate_topk_f32: bad shape");
  FGVC_REQUIRE(window_L == 0 || ((window_L & 1) && Hq == Hk && Wq == Wk), FGVC_ERR_INVALID_ARG,
               "fgvc_propagate_topk_f32: window_L must be odd and the grids equal");
  return propagate_launch(labels, slot_frame, T, idx, weight, Hq, Wq, Hk, Wk, P, topk, window_L, out,
                          (hipStream_t)stream);
}

int fgvc_corr_volume_f32(const float* qfeat, const float* kfeat, int C, int HWq, int HWk, float temperature,
                         float* vol, void* stream) {
  FGVC_REQUIRE(qfeat && kfeat && vol, FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f32: null pointer");
  FGVC_REQUIRE(aligned16(qfeat) && aligned16(kfeat), FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f32: features must be 16-byte aligned");
  FGVC_REQUIRE(HWq > 0 && HWk > 0 && temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f32: bad shape");
  return corr_volume_f32_launch(qfeat, kfeat, C, HWq, HWk, temperature, vol, (hipStream_t)stream);
}

int fgvc_split_bf16(const float* feat, uint16_t* hi_lo, int64_t n_pixels, int C, void* stream) {
  FGVC_REQUIRE(feat && hi_lo, FGVC_ERR_INVALID_ARG, "fgvc_split_bf16: null pointer");
  FGVC_REQUIRE(n_pixels >= 0 && C > 0 && C % 4 == 0, FGVC_ERR_INVALID_ARG, "fgvc_split_bf16: C must be a multiple of 4");
  FGVC_REQUIRE(aligned16(feat) && aligned16(hi_lo), FGVC_ERR_INVALID_ARG, "fgvc_split_bf16: 16-byte alignment required");
  if (n_pixels == 0) return FGVC_OK;
  return split_bf16_launch(feat, hi_lo, n_pixels, C, (hipStream_t)stream);
}

static int corr_bf16_common(const char* who, const uint16_t* q, const uint16_t* k, int C, int HWq, int HWk,
                            float temperature, float* vol, int nseg, void* stream) {
  FGVC_REQUIRE(q && k && vol, FGVC_ERR_INVALID_ARG, "%s: null pointer", who);
  FGVC_REQUIRE(aligned16(q) && aligned16(k), FGVC_ERR_INVALID_ARG, "%s: features must be 16-byte aligned", who);
  FGVC_REQUIRE(C > 0 && C % 64 == 0, FGVC_ERR_UNSUPPORTED, "%s: C=%d must be a multiple of 64", who, C);
  FGVC_REQUIRE(HWq > 0 && HWk > 0 && temperature > 0.f, FGVC_ERR_INVALID_ARG, "%s: bad shape", who);
  return corr_volume_bf16_launch(q, k, C, HWq, HWk, temperature, vol, nseg, (hipStream_t)stream);
}

int fgvc_corr_volume_bf16x3(const uint16_t* q, const uint16_t* k, int C, int HWq, int HWk, float temperature,
                            float* vol, void* stream) {
  return corr_bf16_common("fgvc_corr_volume_bf16x3", q, k, C, HWq, HWk, temperature, vol, 3, stream);
}

int fgvc_corr_volume_bf16(const uint16_t* q, const uint16_t* k, int C, int HWq, int HWk, float temperature,
                          float* vol, void* stream) {
  return corr_bf16_common("fgvc_corr_volume_bf16", q, k, C, HWq, HWk, temperature, vol, 1, stream);
}

int fgvc_split_f16f8(const float* feat, uint8_t* out, int64_t n_pixels, int C, void* stream) {
  FGVC_REQUIRE(feat && out, FGVC_ERR_INVALID_ARG, "fgvc_split_f16f8: null pointer");
  FGVC_REQUIRE(n_pixels >= 0 && C > 0 && C % 4 == 0, FGVC_ERR_INVALID_ARG, "fgvc_split_f16f8: C must be a multiple of 4");
  FGVC_REQUIRE(aligned16(feat) && aligned16(out), FGVC_ERR_INVALID_ARG, "fgvc_split_f16f8: 16-byte alignment required");
  if (n_pixels == 0) return FGVC_OK;
  return split_f16f8_launch(feat, out, n_pixels, C, (hipStream_t)stream);
}

int fgvc_corr_volume_f16f8(const uint8_t* q, const uint8_t* k, int C, int HWq, int HWk, float temperature, float* vol,
                           void* stream) {
  FGVC_REQUIRE(q && k && vol, FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f16f8: null pointer");
  FGVC_REQUIRE(aligned16(q) && aligned16(k) && aligned16(vol), FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f16f8: 16-byte alignment required");
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_corr_volume_f16f8: C=%d unsupported (256 only; use fgvc_corr_volume_bf16x3)", C);
  FGVC_REQUIRE(HWq > 0 && HWk > 0 && temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f16f8: bad shape");
  FGVC_REQUIRE((long long)HWq < (1ll << 30) && (long long)HWk < (1ll << 30), FGVC_ERR_UNSUPPORTED, "fgvc_corr_volume_f16f8: grid too large");
  return corr_volume_f16f8_launch(q, k, HWq, HWk, temperature, vol, (hipStream_t)stream);
}

int fgvc_split_f16f6(const float* feat, uint8_t* out, int64_t n_pixels, int C, void* stream) {
  FGVC_REQUIRE(feat && out, FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6: null pointer");
  FGVC_REQUIRE(n_pixels >= 0, FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6: negative pixel count");
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_split_f16f6: C=%d unsupported (256 only)", C);
  FGVC_REQUIRE(aligned16(feat) && aligned16(out), FGVC_ERR_INVALID_ARG, "fgvc_split_f16f6: 16-byte alignment required");
  if (n_pixels == 0) return FGVC_OK;
  return split_f16f6_launch(feat, out, n_pixels, (hipStream_t)stream);
}

int fgvc_debug_store_sweep_f32(float* buf, int64_t n_floats, int nontemporal, void* stream) {
  FGVC_REQUIRE(buf && aligned16(buf) && n_floats >= 0 && n_floats % 4 == 0, FGVC_ERR_INVALID_ARG, "fgvc_debug_store_sweep_f32: a 16-byte aligned buffer of a multiple of 4 floats");
  if (n_floats == 0) return FGVC_OK;
  return store_sweep_launch(buf, n_floats, nontemporal, (hipStream_t)stream);
}

int fgvc_corr_volume_f16f6(const uint8_t* q, const uint8_t* k, int C, int HWq, int HWk, float temperature, float* vol,
                           void* stream) {
  FGVC_REQUIRE(q && k && vol, FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f16f6: null pointer");
  FGVC_REQUIRE(aligned16(q) && aligned16(k) && aligned16(vol), FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f16f6: 16-byte alignment required");
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_corr_volume_f16f6: C=%d unsupported (256 only; use fgvc_corr_volume_bf16x3)", C);
  FGVC_REQUIRE(HWq > 0 && HWk > 0 && temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_corr_volume_f16f6: bad shape");
  FGVC_REQUIRE((long long)HWq < (1ll << 30) && (long long)HWk < (1ll << 30), FGVC_ERR_UNSUPPORTED, "fgvc_corr_volume_f16f6: grid too large");
  return corr_volume_f16f6_launch(q, k, HWq, HWk, temperature, vol, (hipStream_t)stream);
}

int fgvc_dense_attend_splits(int HWq, int HWk) { return (HWq > 0 && HWk > 0) ? dense_attend_splits(HWq, HWk) : 1; }

int fgvc_dense_attend_f32(const float* vol, const float* labels, int Hq, int Wq, int Hk, int Wk, int P, int masked, int r2max,
                          int ry, int rx, int weight_mode, int first, float* state, int nsplit, void* stream) {
  FGVC_REQUIRE(vol && labels && state, FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_f32: null pointer");
  FGVC_REQUIRE(Hq > 0 && Wq > 0 && Hk > 0 && Wk > 0, FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_f32: bad shape");
  FGVC_REQUIRE((long long)Hk * Wk < (1ll << 30) && (long long)Hq * Wq < (1ll << 30), FGVC_ERR_UNSUPPORTED,
               "fgvc_dense_attend_f32: grid too large");
  FGVC_REQUIRE(P >= 1 && P <= 32, FGVC_ERR_UNSUPPORTED, "fgvc_dense_attend_f32: P=%d outside 1..32", P);
  FGVC_REQUIRE(nsplit >= 1 && nsplit <= 65535, FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_f32: nsplit=%d", nsplit);
  FGVC_REQUIRE(weight_mode == FGVC_WEIGHT_SOFTMAX || weight_mode == FGVC_WEIGHT_COSINE || weight_mode == FGVC_WEIGHT_RAW, FGVC_ERR_INVALID_ARG,
               "fgvc_dense_attend_f32: unknown weight mode %d", weight_mode);
  FGVC_REQUIRE(!masked || (r2max >= 0 && ry >= 0 && rx >= 0), FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_f32: negative mask parameter");
  FGVC_REQUIRE(!masked || (Hq == Hk && Wq == Wk), FGVC_ERR_INVALID_ARG,
               "fgvc_dense_attend_f32: a spatial mask needs equal query/key grids (local_attention.py:331)");
  return dense_attend_launch(vol, labels, Hq, Wq, Hk, Wk, P, masked != 0, r2max, ry, rx, weight_mode,
                             first != 0, state, nsplit, (hipStream_t)stream, nullptr);
}

int fgvc_dense_kth_f32(const float* aff, int HWk, int HWq, int k, float* part, int nsplit, float* thr, void* stream) {
  FGVC_REQUIRE(aff && part && thr, FGVC_ERR_INVALID_ARG, "fgvc_dense_kth_f32: null pointer");
  FGVC_REQUIRE(HWk > 0 && HWq > 0 && (long long)HWk < (1ll << 30) && (long long)HWq < (1ll << 30), FGVC_ERR_INVALID_ARG, "fgvc_dense_kth_f32: bad shape");
  FGVC_REQUIRE(k >= 1 && k <= 64 && k <= HWk, FGVC_ERR_UNSUPPORTED, "fgvc_dense_kth_f32: k=%d outside 1..min(64, HWk)", k);
  FGVC_REQUIRE(nsplit >= 1 && nsplit <= 65535, FGVC_ERR_INVALID_ARG, "fgvc_dense_kth_f32: nsplit=%d", nsplit);
  return dense_kth_launch(aff, HWk, HWq, k, part, nsplit, thr, (hipStream_t)stream);
}

int fgvc_dense_propagate_f32(const float* aff, const float* labels, int HWk, int HWq, int P, const float* thr, float* state,
                             int nsplit, float* out, void* stream) {
  FGVC_REQUIRE(aff && labels && state && out, FGVC_ERR_INVALID_ARG, "fgvc_dense_propagate_f32: null pointer");
  FGVC_REQUIRE(HWk > 0 && HWq > 0 && (long long)HWk < (1ll << 30) && (long long)HWq < (1ll << 30), FGVC_ERR_INVALID_ARG, "fgvc_dense_propagate_f32: bad shape");
  FGVC_REQUIRE(P >= 1 && P <= 32, FGVC_ERR_UNSUPPORTED, "fgvc_dense_propagate_f32: P=%d outside 1..32 (call per 32 channels)", P);
  FGVC_REQUIRE(nsplit >= 1 && nsplit <= 65535, FGVC_ERR_INVALID_ARG, "fgvc_dense_propagate_f32: nsplit=%d", nsplit);
  const int mode = thr ? 3 : 2;
  int rc = dense_attend_launch(aff, labels, 1, HWq, 1, HWk, P, 0, FGVC_NO_LIMIT, FGVC_NO_LIMIT, FGVC_NO_LIMIT, mode, 1, state, nsplit,
                               (hipStream_t)stream, thr);
  if (rc != FGVC_OK) return rc;
  return dense_attend_finish_launch(state, nsplit, HWq, P, mode, out, (hipStream_t)stream);
}

int fgvc_dense_attend_finish_f32(const float* state, int nsplit, int HWq, int P, int weight_mode, float* out, void* stream) {
  FGVC_REQUIRE(state && out, FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_finish_f32: null pointer");
  FGVC_REQUIRE(HWq > 0 && P >= 1 && P <= 32 && nsplit >= 1, FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_finish_f32: bad shape");
  FGVC_REQUIRE(weight_mode >= 0 && weight_mode <= 2, FGVC_ERR_INVALID_ARG, "fgvc_dense_attend_finish_f32: unknown weight mode %d", weight_mode);
  return dense_attend_finish_launch(state, nsplit, HWq, P, weight_mode, out, (hipStream_t)stream);
}

int fgvc_local_corr_topk_f32(const float* qfeat, const float* kfeat, const int32_t* pairs, int n_slots, int C, int H,
                             int W, int R, int topk, float temperature, int32_t* pair_idx_ws, float* pair_score_ws,
                             int32_t* idx_out, float* logit_out, float* weight_out, void* stream) {
  FGVC_REQUIRE(pair_idx_ws && pair_score_ws && idx_out && logit_out && weight_out, FGVC_ERR_INVALID_ARG,
               "fgvc_local_corr_topk_f32: null pointer");
  FGVC_REQUIRE(R >= 0 && n_slots >= 1 && temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_local_corr_topk_f32: bad R/n_slots/temperature");
  FGVC_REQUIRE((long long)n_slots * (2 * R + 1) * (2 * R + 1) < (1ll << 31), FGVC_ERR_UNSUPPORTED,
               "fgvc_local_corr_topk_f32: index overflow");
  int rc = fgvc_pair_topk_f32(qfeat, kfeat, pairs, n_slots, C, H, W, H, W, FGVC_NO_LIMIT, R, R, topk, nullptr,
                              pair_idx_ws, pair_score_ws, stream);
  if (rc != FGVC_OK) return rc;
  return local_merge_launch(pair_idx_ws, pair_score_ws, n_slots, H, W, R, topk, temperature, idx_out, logit_out,
                            weight_out, (hipStream_t)stream);
}

int fgvc_local_corr_topk_f16x3(const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_slots, int C,
                               int H, int W, int R, int topk, float temperature, int32_t* pair_idx_ws,
                               float* pair_score_ws, int32_t* idx_out, float* logit_out, float* weight_out,
                               void* stream) {
  FGVC_REQUIRE(pair_idx_ws && pair_score_ws && idx_out && logit_out && weight_out, FGVC_ERR_INVALID_ARG,
               "fgvc_local_corr_topk_f16x3: null pointer");
  FGVC_REQUIRE(R >= 0 && n_slots >= 1 && temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_local_corr_topk_f16x3: bad R/n_slots/temperature");
  FGVC_REQUIRE((long long)n_slots * (2 * R + 1) * (2 * R + 1) < (1ll << 31), FGVC_ERR_UNSUPPORTED,
               "fgvc_local_corr_topk_f16x3: index overflow");
  // every slot of a local window is a masked pair (the window IS the mask): all_masked = 1
  int rc = fgvc_pair_topk_f16x3(qsplit, ksplit, pairs, n_slots, C, H, W, H, W, FGVC_NO_LIMIT, R, R, topk, 1, pair_idx_ws,
                                pair_score_ws, stream);
  if (rc != FGVC_OK) return rc;
  return local_merge_launch(pair_idx_ws, pair_score_ws, n_slots, H, W, R, topk, temperature, idx_out, logit_out,
                            weight_out, (hipStream_t)stream);
}

int fgvc_local_merge_plan_f32(const int32_t* pair_idx, const float* pair_score, int n_pairs, const int32_t* slot_pair, int n_rows,
                              int max_slots, int H, int W, int R, int topk, float temperature, int32_t* idx_out, float* logit_out,
                              float* weight_out, void* stream) {
  FGVC_REQUIRE(pair_idx && pair_score && slot_pair && idx_out && logit_out && weight_out, FGVC_ERR_INVALID_ARG,
               "fgvc_local_merge_plan_f32: null pointer");
  FGVC_REQUIRE(H > 0 && W > 0 && R >= 0 && n_pairs >= 1 && n_rows >= 0 && max_slots >= 1, FGVC_ERR_INVALID_ARG,
               "fgvc_local_merge_plan_f32: bad shape H=%d W=%d R=%d n_pairs=%d n_rows=%d max_slots=%d", H, W, R, n_pairs, n_rows, max_slots);
  FGVC_REQUIRE(topk >= 1 && topk <= 16, FGVC_ERR_UNSUPPORTED, "fgvc_local_merge_plan_f32: topk=%d outside 1..16", topk);
  FGVC_REQUIRE(temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_local_merge_plan_f32: temperature must be > 0");
  FGVC_REQUIRE(n_rows <= 65535, FGVC_ERR_UNSUPPORTED, "fgvc_local_merge_plan_f32: n_rows=%d > 65535 per call", n_rows);
  FGVC_REQUIRE((long long)max_slots * (2 * R + 1) * (2 * R + 1) < (1ll << 31) && (long long)H * W < (1ll << 30), FGVC_ERR_UNSUPPORTED,
               "fgvc_local_merge_plan_f32: index overflow");
  if (n_rows == 0) return FGVC_OK;
  return local_merge_plan_launch(pair_idx, pair_score, slot_pair, n_pairs, n_rows, max_slots, H, W, R, topk, temperature, idx_out,
                                 logit_out, weight_out, (hipStream_t)stream);
}

int fgvc_topk_coord_f32(const int32_t* idx, const float* weight, int H, int W, int R, int topk, int scale, float* out,
                        void* stream) {
  FGVC_REQUIRE(idx && weight && out, FGVC_ERR_INVALID_ARG, "fgvc_topk_coord_f32: null pointer");
  FGVC_REQUIRE(H > 0 && W > 0 && R >= 0 && topk >= 1 && scale >= 1, FGVC_ERR_INVALID_ARG, "fgvc_topk_coord_f32: bad shape");
  return topk_coord_launch(idx, weight, H, W, R, topk, scale, out, (hipStream_t)stream);
}

int fgvc_topk_coord_rows_f32(const int32_t* idx, const float* weight, int rows, int H, int W, int R, int topk, int scale, float* out,
                             void* stream) {
  FGVC_REQUIRE(idx && weight && out, FGVC_ERR_INVALID_ARG, "fgvc_topk_coord_rows_f32: null pointer");
  FGVC_REQUIRE(rows >= 1 && rows <= 65535 && H > 0 && W > 0 && R >= 0 && topk >= 1 && scale >= 1 && (long long)H * W < (1ll << 30),
               FGVC_ERR_INVALID_ARG, "fgvc_topk_coord_rows_f32: bad shape");
  FGVC_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, FGVC_ERR_INVALID_ARG, "fgvc_topk_coord_rows_f32: out must be 8-byte aligned");
  return topk_coord_rows_launch(idx, weight, rows, H, W, R, topk, scale, out, (hipStream_t)stream);
}

int fgvc_cycle_chase_f32(const float* fields, const float* traj, const float* start_xy, int n, int P, int H, int W, int scale,
                         float* back_out, float* err_out, void* stream) {
  FGVC_REQUIRE(fields && traj && start_xy && back_out && err_out, FGVC_ERR_INVALID_ARG, "fgvc_cycle_chase_f32: null pointer");
  FGVC_REQUIRE(n >= 1 && P >= 1 && H > 0 && W > 0 && scale >= 1 && (long long)H * W < (1ll << 30) && (long long)n * P < (1ll << 30),
               FGVC_ERR_INVALID_ARG, "fgvc_cycle_chase_f32: bad shape");
  FGVC_REQUIRE(((reinterpret_cast<uintptr_t>(fields) | reinterpret_cast<uintptr_t>(traj) | reinterpret_cast<uintptr_t>(start_xy) |
                 reinterpret_cast<uintptr_t>(back_out)) & 7u) == 0,
               FGVC_ERR_INVALID_ARG, "fgvc_cycle_chase_f32: the (x, y) arrays must be 8-byte aligned");
  return cycle_chase_launch(fields, traj, start_xy, n, P, H, W, scale, back_out, err_out, (hipStream_t)stream);
}

int fgvc_flow_from_lists_f32(const int32_t* idx, const float* weight, int rows, int H, int W, int R, int topk, int scale, int renorm, int h,
                             int w, int pad_left, int pad_top, float* flow_out, uint8_t* valid_out, void* stream) {
  FGVC_REQUIRE(idx && weight && flow_out && valid_out, FGVC_ERR_INVALID_ARG, "fgvc_flow_from_lists_f32: null pointer");
  FGVC_REQUIRE(rows >= 1 && rows <= 65535 && H > 0 && W > 0 && R >= 0 && topk >= 1 && scale >= 1 && (long long)H * W < (1ll << 30),
               FGVC_ERR_INVALID_ARG, "fgvc_flow_from_lists_f32: bad shape (rows=%d, %d x %d cells, R=%d, topk=%d, scale=%d)", rows, H, W, R, topk, scale);
  // grid.y = ceil(h / 16) is 16-bit; pixel and cell coordinates times scale stay inside an int
  FGVC_REQUIRE(h > 0 && w > 0 && pad_left >= 0 && pad_top >= 0 && h <= 16 * 65535 && (long long)h * w < (1ll << 30) &&
                   (long long)pad_left + w < (1ll << 30) && (long long)pad_top + h < (1ll << 30) && (long long)imax(H, W) * scale < (1ll << 30),
               FGVC_ERR_INVALID_ARG, "fgvc_flow_from_lists_f32: bad output (%d x %d, pad %d, %d)", h, w, pad_left, pad_top);
  return flow_from_lists_launch(idx, weight, rows, H, W, R, topk, scale, renorm != 0, h, w, pad_left, pad_top, flow_out, valid_out,
                                (hipStream_t)stream);
}

int fgvc_flow_consistency_f32(const float* flow_fw, const float* flow_bw, int n, int h, int w, int mode, float diff, float* occ_fw,
                              float* occ_bw, void* stream) {
  FGVC_REQUIRE(flow_fw && flow_bw && occ_fw && occ_bw, FGVC_ERR_INVALID_ARG, "fgvc_flow_consistency_f32: null pointer");
  FGVC_REQUIRE(n >= 1 && n <= 65535 && h > 0 && w > 0 && (long long)h * w < (1ll << 30), FGVC_ERR_INVALID_ARG,
               "fgvc_flow_consistency_f32: bad shape (n=%d, %d x %d)", n, h, w);
  FGVC_REQUIRE(mode == FGVC_FLOW_CONSISTENCY || mode == FGVC_FLOW_FB_ABS, FGVC_ERR_INVALID_ARG, "fgvc_flow_consistency_f32: mode=%d", mode);
  return flow_consistency_launch(flow_fw, flow_bw, n, h, w, mode, diff, occ_fw, occ_bw, (hipStream_t)stream);
}

int fgvc_warp_f32(const float* feat, const float* flow, int N, int C, int H, int W, int align_corners, int use_mask, float* out, void* stream) {
  FGVC_REQUIRE(feat && flow && out, FGVC_ERR_INVALID_ARG, "fgvc_warp_f32: null pointer");
  FGVC_REQUIRE(N >= 1 && N <= 65535 && C >= 1 && H > 0 && W > 0 && (long long)H * W < (1ll << 30), FGVC_ERR_INVALID_ARG,
               "fgvc_warp_f32: bad shape (N=%d, C=%d, %d x %d)", N, C, H, W);
  return warp_launch(feat, flow, N, C, H, W, align_corners != 0, use_mask != 0, out, (hipStream_t)stream);
}

int fgvc_flow_chain_f32(const float* flow_fw, const float* flow_bw, const uint8_t* ok_fw, const uint8_t* ok_bw, const float* query, int T,
                        int P, int h, int w, int visibility, float* traj_out, uint8_t* vis_out, void* stream) {
  FGVC_REQUIRE(T >= 1 && T <= 65536 && P >= 0 && h > 0 && w > 0 && (long long)h * w < (1ll << 30), FGVC_ERR_INVALID_ARG,
               "fgvc_flow_chain_f32: bad shape (T=%d, P=%d, %d x %d)", T, P, h, w);
  FGVC_REQUIRE(visibility == FGVC_CHAIN_FRAME || visibility == FGVC_CHAIN_CONSISTENCY, FGVC_ERR_INVALID_ARG,
               "fgvc_flow_chain_f32: visibility=%d", visibility);
  if (P == 0) return FGVC_OK;
  FGVC_REQUIRE(query && traj_out && vis_out && (T == 1 || (flow_fw && flow_bw)), FGVC_ERR_INVALID_ARG, "fgvc_flow_chain_f32: null pointer");
  FGVC_REQUIRE(visibility == FGVC_CHAIN_FRAME || T == 1 || (ok_fw && ok_bw), FGVC_ERR_INVALID_ARG,
               "fgvc_flow_chain_f32: visibility 'consistency' needs both masks");
  FGVC_REQUIRE(((uintptr_t)traj_out & 7) == 0, FGVC_ERR_INVALID_ARG, "fgvc_flow_chain_f32: alignment (8 bytes for traj_out)");
  const bool sticky = visibility == FGVC_CHAIN_CONSISTENCY;
  return flow_chain_launch(flow_fw, flow_bw, sticky ? ok_fw : nullptr, sticky ? ok_bw : nullptr, query, T, P, h, w, sticky, traj_out, vis_out,
                           (hipStream_t)stream);
}

int fgvc_frames_rgb8_to_lab_f32(const uint8_t* frames, int T, int h0, int w0, int64_t stride_t, int64_t stride_y, int64_t stride_x,
                                int64_t stride_c, int h, int w, int pad_left, int pad_right, int pad_top, int pad_bottom, float* out,
                                void* stream) {
  FGVC_REQUIRE(frames && out, FGVC_ERR_INVALID_ARG, "fgvc_frames_rgb8_to_lab_f32: null pointer");
  FGVC_REQUIRE(T > 0 && h0 > 0 && w0 > 0 && h > 0 && w > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_lab_f32: non-positive size (T=%d, %d x %d -> %d x %d)", T, h0, w0, h, w);
  FGVC_REQUIRE(pad_left >= 0 && pad_right >= 0 && pad_top >= 0 && pad_bottom >= 0, FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_lab_f32: negative pad (%d, %d, %d, %d)", pad_left, pad_right, pad_top, pad_bottom);
  const long long hp = (long long)pad_top + h + pad_bottom, wp = (long long)pad_left + w + pad_right;
  // grid.z = T and grid.y = ceil(hp / 4) are 16-bit; a lane's column index 4 * (blockIdx.x * 256 + lane) and hp * wp stay inside an int
  FGVC_REQUIRE(T <= 65535 && hp <= 4 * 65535ll && wp < (1ll << 30) && hp * wp < (1ll << 31), FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_lab_f32: shape beyond the launch grid (T <= 65535, padded rows <= 262140, padded plane < 2^31 pixels)");
  return frames_rgb8_to_lab_launch(frames, T, h0, w0, stride_t, stride_y, stride_x, stride_c, h, w, pad_left, pad_right, pad_top, pad_bottom,
                                   out, (hipStream_t)stream);
}

struct YuvFormat {                                         // the yuvp pair's format arguments
  int sample_bytes, depth, shift, sub_x, sub_y;
};
static const YuvFormat YUV420 = {1, 8, 0, 2, 2};           // what the 8-bit 4:2:0 pair's planes are in those words

// what the four fgvc_frames_yuv* entries check alike: pointers, the siting and -- `fmt`: the yuvp pair's, null for the 8-bit 4:2:0 pair --
// the sample format, the subsampling and the planes' alignment
static int yuv_check(const char* fn, const void* y, const void* u, const void* v, const void* out, const YuvFormat* fmt, int siting) {
  FGVC_REQUIRE(y && u && v && out, FGVC_ERR_INVALID_ARG, "%s: null pointer", fn);
  if (fmt) {
    FGVC_REQUIRE(fmt->sample_bytes == 1 || fmt->sample_bytes == 2, FGVC_ERR_INVALID_ARG, "%s: sample_bytes=%d (1 or 2)", fn, fmt->sample_bytes);
    FGVC_REQUIRE(fmt->depth >= 8 && fmt->depth <= 16 && fmt->shift >= 0 && fmt->depth + fmt->shift <= 8 * fmt->sample_bytes,
                 FGVC_ERR_INVALID_ARG, "%s: depth=%d, shift=%d (depth 8..16, shift >= 0, depth + shift within the %d bits of a sample)", fn,
                 fmt->depth, fmt->shift, 8 * fmt->sample_bytes);
    FGVC_REQUIRE((fmt->sub_x == 1 || fmt->sub_x == 2) && (fmt->sub_y == 1 || fmt->sub_y == 2), FGVC_ERR_INVALID_ARG,
                 "%s: sub_x=%d, sub_y=%d (1 or 2 each)", fn, fmt->sub_x, fmt->sub_y);
  }
  FGVC_REQUIRE(siting == FGVC_YUV_SITING_LEFT || siting == FGVC_YUV_SITING_CENTER, FGVC_ERR_INVALID_ARG,
               "%s: siting=%d (FGVC_YUV_SITING_LEFT or FGVC_YUV_SITING_CENTER)", fn, siting);
  FGVC_REQUIRE(!fmt || fmt->sample_bytes == 1 || ((((uintptr_t)y) | ((uintptr_t)u) | ((uintptr_t)v)) & 1) == 0, FGVC_ERR_INVALID_ARG,
               "%s: alignment (16-bit planes at even addresses)", fn);
  return FGVC_OK;
}

// the Lab pair: checks, then the launch.  fmt: as yuv_check's; coef = (y_off, cy, c_off, crv, cgu, cgv, cbu)
static int yuv_to_lab(const char* fn, const void* y, const void* u, const void* v, const YuvFormat* fmt, int T, int h0, int w0, int64_t y_stride_t,
                      int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, const float* coef, int siting, int h, int w,
                      int pad_left, int pad_right, int pad_top, int pad_bottom, float* out, void* stream) {
  const int rc = yuv_check(fn, y, u, v, out, fmt, siting);
  if (rc != FGVC_OK) return rc;
  FGVC_REQUIRE(T > 0 && h0 > 0 && w0 > 0 && h > 0 && w > 0, FGVC_ERR_INVALID_ARG, "%s: non-positive size (T=%d, %d x %d -> %d x %d)", fn, T, h0,
               w0, h, w);
  FGVC_REQUIRE(pad_left >= 0 && pad_right >= 0 && pad_top >= 0 && pad_bottom >= 0, FGVC_ERR_INVALID_ARG, "%s: negative pad (%d, %d, %d, %d)",
               fn, pad_left, pad_right, pad_top, pad_bottom);
  const long long hp = (long long)pad_top + h + pad_bottom, wp = (long long)pad_left + w + pad_right;
  // the grid of fgvc_frames_rgb8_to_lab_f32; a source column's position in quarter chroma samples, 2 x, stays inside an int
  FGVC_REQUIRE(T <= 65535 && hp <= 4 * 65535ll && wp < (1ll << 30) && hp * wp < (1ll << 31) && h0 < (1 << 30) && w0 < (1 << 30),
               FGVC_ERR_INVALID_ARG,
               "%s: shape beyond the launch grid (T <= 65535, padded rows <= 262140, padded plane < 2^31 pixels, source sides < 2^30)", fn);
  const YuvFormat& f = fmt ? *fmt : YUV420;
  return frames_yuv_to_lab_launch(fn, !fmt, y, u, v, f.sample_bytes, f.depth, f.shift, f.sub_x, f.sub_y, T, h0, w0, y_stride_t, y_stride_y,
                                  c_stride_t, c_stride_y, c_stride_x, coef, siting, h, w, pad_left, pad_right, pad_top, pad_bottom, out,
                                  (hipStream_t)stream);
}

// the bytes pair
static int yuv_to_rgb8(const char* fn, const void* y, const void* u, const void* v, const YuvFormat* fmt, int T, int h0, int w0, int64_t y_stride_t,
                       int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, const float* coef, int siting,
                       uint8_t* out, void* stream) {
  const int rc = yuv_check(fn, y, u, v, out, fmt, siting);
  if (rc != FGVC_OK) return rc;
  FGVC_REQUIRE(T > 0 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG, "%s: non-positive size (T=%d, %d x %d)", fn, T, h0, w0);
  FGVC_REQUIRE(T <= 65535 && h0 <= 4 * 65535ll && w0 < (1 << 30) && (long long)h0 * w0 < (1ll << 31), FGVC_ERR_INVALID_ARG,
               "%s: shape beyond the launch grid (T <= 65535, rows <= 262140, frame < 2^31 pixels)", fn);
  const YuvFormat& f = fmt ? *fmt : YUV420;
  return frames_yuv_to_rgb8_launch(fn, !fmt, y, u, v, f.sample_bytes, f.depth, f.shift, f.sub_x, f.sub_y, T, h0, w0, y_stride_t, y_stride_y,
                                   c_stride_t, c_stride_y, c_stride_x, coef, siting, out, (hipStream_t)stream);
}

// the 8-bit 4:2:0 pair launches the fixed-format instances (no fmt), the yuvp pair the run-time ones -- also at depth 8, (2, 2), shift 0
int fgvc_frames_yuv420_to_lab_f32(const uint8_t* y, const uint8_t* u, const uint8_t* v, int T, int h0, int w0, int64_t y_stride_t,
                                  int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, float y_off, float cy,
                                  float crv, float cgu, float cgv, float cbu, int siting, int h, int w, int pad_left, int pad_right,
                                  int pad_top, int pad_bottom, float* out, void* stream) {
  const float coef[7] = {y_off, cy, 128.0f, crv, cgu, cgv, cbu};
  return yuv_to_lab("fgvc_frames_yuv420_to_lab_f32", y, u, v, nullptr, T, h0, w0, y_stride_t, y_stride_y, c_stride_t, c_stride_y, c_stride_x,
                    coef, siting, h, w, pad_left, pad_right, pad_top, pad_bottom, out, stream);
}

int fgvc_frames_yuv420_to_rgb8(const uint8_t* y, const uint8_t* u, const uint8_t* v, int T, int h0, int w0, int64_t y_stride_t,
                               int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, float y_off, float cy, float crv,
                               float cgu, float cgv, float cbu, int siting, uint8_t* out, void* stream) {
  const float coef[7] = {y_off, cy, 128.0f, crv, cgu, cgv, cbu};
  return yuv_to_rgb8("fgvc_frames_yuv420_to_rgb8", y, u, v, nullptr, T, h0, w0, y_stride_t, y_stride_y, c_stride_t, c_stride_y, c_stride_x, coef,
                     siting, out, stream);
}

int fgvc_frames_yuvp_to_lab_f32(const void* y, const void* u, const void* v, int sample_bytes, int depth, int shift, int sub_x, int sub_y, int T,
                                int h0, int w0, int64_t y_stride_t, int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y,
                                int64_t c_stride_x, float y_off, float cy, float c_off, float crv, float cgu, float cgv, float cbu, int siting,
                                int h, int w, int pad_left, int pad_right, int pad_top, int pad_bottom, float* out, void* stream) {
  const YuvFormat fmt = {sample_bytes, depth, shift, sub_x, sub_y};
  const float coef[7] = {y_off, cy, c_off, crv, cgu, cgv, cbu};
  return yuv_to_lab("fgvc_frames_yuvp_to_lab_f32", y, u, v, &fmt, T, h0, w0, y_stride_t, y_stride_y, c_stride_t, c_stride_y, c_stride_x, coef,
                    siting, h, w, pad_left, pad_right, pad_top, pad_bottom, out, stream);
}

int fgvc_frames_yuvp_to_rgb8(const void* y, const void* u, const void* v, int sample_bytes, int depth, int shift, int sub_x, int sub_y, int T,
                             int h0, int w0, int64_t y_stride_t, int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y,
                             int64_t c_stride_x, float y_off, float cy, float c_off, float crv, float cgu, float cgv, float cbu, int siting,
                             uint8_t* out, void* stream) {
  const YuvFormat fmt = {sample_bytes, depth, shift, sub_x, sub_y};
  const float coef[7] = {y_off, cy, c_off, crv, cgu, cgv, cbu};
  return yuv_to_rgb8("fgvc_frames_yuvp_to_rgb8", y, u, v, &fmt, T, h0, w0, y_stride_t, y_stride_y, c_stride_t, c_stride_y, c_stride_x, coef, siting,
                     out, stream);
}

int fgvc_yuv_out_tile_rows(void) {
  int rows, cols;
  yuv_out_tile(&rows, &cols);
  return rows;
}

int fgvc_yuv_out_tile_cols(void) {
  int rows, cols;
  yuv_out_tile(&rows, &cols);
  return cols;
}

int fgvc_frames_rgb8_to_yuv420(const uint8_t* frames, int T, int h0, int w0, int64_t stride_t, int64_t stride_y, int64_t stride_x,
                               int64_t stride_c, uint8_t* y, int64_t y_stride_t, int64_t y_stride_y, uint8_t* u, uint8_t* v,
                               int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, float kr, float kg, float kb, float y_off, float sy,
                               float cu, float cv, int siting, void* stream) {
  FGVC_REQUIRE(T >= 0 && h0 > 0 && w0 > 0, FGVC_ERR_INVALID_ARG, "fgvc_frames_rgb8_to_yuv420: T=%d negative or a non-positive size (%d x %d)", T,
               h0, w0);
  FGVC_REQUIRE(siting == FGVC_YUV_SITING_LEFT || siting == FGVC_YUV_SITING_CENTER, FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_yuv420: siting=%d (FGVC_YUV_SITING_LEFT or FGVC_YUV_SITING_CENTER)", siting);
  const int rows = fgvc_yuv_out_tile_rows();
  // grid.z = T and grid.y = ceil(h0 / rows) are 16-bit; a lane's column index stays inside an int
  FGVC_REQUIRE(T <= 65535 && h0 <= rows * 65535ll && w0 < (1 << 30), FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_yuv420: shape beyond the launch grid (T <= 65535, rows <= %lld, columns < 2^30)", rows * 65535ll);
  const long long ch = (h0 + 1) / 2, cw = (w0 + 1) / 2;
  FGVC_REQUIRE(y_stride_y >= w0 && (T <= 1 || y_stride_t >= (h0 - 1) * (long long)y_stride_y + w0), FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_yuv420: luma rows and frames must not overlap (strides %lld, %lld bytes for %d x %d)",
               (long long)y_stride_t, (long long)y_stride_y, h0, w0);
  const long long crow = (cw - 1) * (long long)c_stride_x + 1;        // the bytes a chroma row spans
  FGVC_REQUIRE(c_stride_x >= 1 && c_stride_y >= crow && (T <= 1 || c_stride_t >= (ch - 1) * (long long)c_stride_y + crow), FGVC_ERR_INVALID_ARG,
               "fgvc_frames_rgb8_to_yuv420: chroma samples, rows and frames must not overlap (strides %lld, %lld, %lld bytes for %lld x %lld)",
               (long long)c_stride_t, (long long)c_stride_y, (long long)c_stride_x, ch, cw);
  if (T == 0) return FGVC_OK;                                         // no pixel exists
  FGVC_REQUIRE(frames && y && u && v, FGVC_ERR_INVALID_ARG, "fgvc_frames_rgb8_to_yuv420: null pointer");
  const float coef[7] = {kr, kg, kb, y_off, sy, cu, cv};
  return frames_rgb8_to_yuv420_launch(frames, T, h0, w0, stride_t, stride_y, stride_x, stride_c, y, y_stride_t, y_stride_y, u, v, c_stride_t,
                                      c_stride_y, c_stride_x, coef, siting, (hipStream_t)stream);
}

int fgvc_jf_tile_rows(void) { return jf_tile_rows(); }

int fgvc_jf_counts_u8(const uint8_t* gt, const uint8_t* pred, int T, int h, int w, int n_objects, int radius, int64_t* counts, void* stream) {
  FGVC_REQUIRE(T >= 0 && h >= 0 && w >= 0, FGVC_ERR_INVALID_ARG, "fgvc_jf_counts_u8: negative size (T=%d, %d x %d)", T, h, w);
  FGVC_REQUIRE(n_objects >= 0 && n_objects <= 255, FGVC_ERR_INVALID_ARG, "fgvc_jf_counts_u8: n_objects=%d (0 .. 255: the ids are bytes)", n_objects);
  FGVC_REQUIRE(radius >= 1, FGVC_ERR_INVALID_ARG, "fgvc_jf_counts_u8: radius=%d (at least 1)", radius);
  FGVC_REQUIRE(radius <= 64, FGVC_ERR_UNSUPPORTED, "fgvc_jf_counts_u8: radius=%d beyond 64 (the disk reaches one 64-pixel word to either side)", radius);
  FGVC_REQUIRE((long long)h * w < (1ll << 31), FGVC_ERR_INVALID_ARG, "fgvc_jf_counts_u8: a frame of %d x %d has 2^31 pixels or more", h, w);
  if (T == 0 || n_objects == 0) return FGVC_OK;                       // no element of `counts` exists
  FGVC_REQUIRE(gt && pred && counts, FGVC_ERR_INVALID_ARG, "fgvc_jf_counts_u8: null pointer");
  return jf_counts_launch(gt, pred, T, h, w, n_objects, radius, counts, (hipStream_t)stream);
}

int fgvc_seg_object_stats_u8(const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y, int T, int h, int w, int n_ids, int64_t* stats,
                             void* stream) {
  const char* fn = "fgvc_seg_object_stats_u8";
  FGVC_REQUIRE(ids, FGVC_ERR_INVALID_ARG, "%s: ids: null pointer", fn);
  FGVC_REQUIRE(stats, FGVC_ERR_INVALID_ARG, "%s: stats: null pointer", fn);
  FGVC_REQUIRE(n_ids >= 1 && n_ids <= 256, FGVC_ERR_INVALID_ARG, "%s: n_ids=%d (1 .. 256: the ids are bytes)", fn, n_ids);
  FGVC_REQUIRE(T >= 1, FGVC_ERR_INVALID_ARG, "%s: T=%d (at least 1)", fn, T);
  FGVC_REQUIRE(h >= 1, FGVC_ERR_INVALID_ARG, "%s: h=%d (at least 1)", fn, h);
  FGVC_REQUIRE(w >= 1, FGVC_ERR_INVALID_ARG, "%s: w=%d (at least 1)", fn, w);
  // sum_x and sum_y stay below h w max(h, w): 64-bit sums hold them with room to spare below 2^62
  FGVC_REQUIRE((unsigned __int128)h * (unsigned)w * (unsigned)(h > w ? h : w) < ((unsigned __int128)1 << 62), FGVC_ERR_INVALID_ARG,
               "%s: h, w = %d, %d: h w max(h, w) reaches 2^62", fn, h, w);
  FGVC_REQUIRE(ids_stride_y >= w && (T == 1 || ids_stride_t >= 0), FGVC_ERR_INVALID_ARG,
               "%s: ids_stride_y: a row stride of at least w = %d bytes and a non-negative frame stride, got %lld, %lld", fn, w,
               (long long)ids_stride_y, (long long)ids_stride_t);
  return object_stats_launch(ids, ids_stride_t, ids_stride_y, T, h, w, n_ids, stats, (hipStream_t)stream);
}

int fgvc_seg_ccl_tile_rows(void) {
  int rows, cols;
  ccl_tile(&rows, &cols);
  return rows;
}

int fgvc_seg_ccl_tile_cols(void) {
  int rows, cols;
  ccl_tile(&rows, &cols);
  return cols;
}

// what the two component entries ask of a map read through its strides
static int ccl_map_checks(const char* fn, const char* what, const void* p, int64_t stride_t, int64_t stride_y, int T, int h, int w) {
  FGVC_REQUIRE(p, FGVC_ERR_INVALID_ARG, "%s: %s: null pointer", fn, what);
  FGVC_REQUIRE(stride_y >= w && (T == 1 || stride_t >= 0), FGVC_ERR_INVALID_ARG,
               "%s: %s_stride_y: a row stride of at least w = %d bytes and a non-negative frame stride, got %lld, %lld", fn, what, w,
               (long long)stride_y, (long long)stride_t);
  return FGVC_OK;
}

static int ccl_shape_checks(const char* fn, int T, int h, int w, int connectivity) {
  FGVC_REQUIRE(T >= 1, FGVC_ERR_INVALID_ARG, "%s: T=%d (at least 1)", fn, T);
  FGVC_REQUIRE(h >= 1, FGVC_ERR_INVALID_ARG, "%s: h=%d (at least 1)", fn, h);
  FGVC_REQUIRE(w >= 1, FGVC_ERR_INVALID_ARG, "%s: w=%d (at least 1)", fn, w);
  FGVC_REQUIRE((long long)h * w < (1ll << 31), FGVC_ERR_INVALID_ARG, "%s: h, w = %d, %d: a frame of 2^31 pixels or more (a label is an int32 index)",
               fn, h, w);
  FGVC_REQUIRE(connectivity == 4 || connectivity == 8, FGVC_ERR_INVALID_ARG, "%s: connectivity=%d (4 or 8)", fn, connectivity);
  FGVC_REQUIRE(ccl_blocks(T, h, w) < (1ll << 31), FGVC_ERR_UNSUPPORTED, "%s: T=%d frames of %d x %d: 2^31 tiles or more (one workgroup a tile)", fn,
               T, h, w);
  return FGVC_OK;
}

int fgvc_seg_components_i32(const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y, int T, int h, int w, int connectivity, int background,
                            int32_t* labels, void* stream) {
  const char* fn = "fgvc_seg_components_i32";
  FGVC_REQUIRE(labels, FGVC_ERR_INVALID_ARG, "%s: labels: null pointer", fn);
  int rc = ccl_shape_checks(fn, T, h, w, connectivity);
  if (rc != FGVC_OK) return rc;
  rc = ccl_map_checks(fn, "ids", ids, ids_stride_t, ids_stride_y, T, h, w);
  if (rc != FGVC_OK) return rc;
  FGVC_REQUIRE(background == 0 || background == 1, FGVC_ERR_INVALID_ARG, "%s: background=%d (0 or 1)", fn, background);
  return components_launch(ids, ids_stride_t, ids_stride_y, T, h, w, connectivity, background, labels, (hipStream_t)stream);
}

size_t fgvc_seg_clean_workspace_bytes(int T, int h, int w, int n_ids) {
  if (T < 1 || h < 1 || w < 1 || n_ids < 1 || n_ids > 256 || (long long)h * w >= (1ll << 31)) return 0;
  return clean_workspace_bytes(T, h, w, n_ids);
}

int fgvc_seg_clean_u8(const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y, int T, int h, int w, int n_ids, int connectivity, int min_area,
                      int keep_largest, int fill_holes, int64_t max_hole_area, const uint8_t* frame_flags, uint8_t* out, int64_t out_stride_t,
                      int64_t out_stride_y, int64_t* stats, void* workspace, size_t workspace_bytes, void* stream) {
  const char* fn = "fgvc_seg_clean_u8";
  FGVC_REQUIRE(stats, FGVC_ERR_INVALID_ARG, "%s: stats: null pointer", fn);
  FGVC_REQUIRE(workspace, FGVC_ERR_INVALID_ARG, "%s: workspace: null pointer", fn);
  FGVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, FGVC_ERR_INVALID_ARG, "%s: workspace: must be 8-byte aligned", fn);
  FGVC_REQUIRE(n_ids >= 1 && n_ids <= 256, FGVC_ERR_INVALID_ARG, "%s: n_ids=%d (1 .. 256: the ids are bytes)", fn, n_ids);
  int rc = ccl_shape_checks(fn, T, h, w, connectivity);
  if (rc != FGVC_OK) return rc;
  rc = ccl_map_checks(fn, "ids", ids, ids_stride_t, ids_stride_y, T, h, w);
  if (rc != FGVC_OK) return rc;
  rc = ccl_map_checks(fn, "out", out, out_stride_t, out_stride_y, T, h, w);
  if (rc != FGVC_OK) return rc;
  FGVC_REQUIRE(T == 1 || out_stride_t >= (h - 1) * (long long)out_stride_y + w, FGVC_ERR_INVALID_ARG,
               "%s: out_stride_t: the frames of out must not overlap (strides %lld, %lld bytes for %d x %d)", fn, (long long)out_stride_t,
               (long long)out_stride_y, h, w);
  FGVC_REQUIRE(out != ids || (out_stride_t == ids_stride_t && out_stride_y == ids_stride_y), FGVC_ERR_INVALID_ARG,
               "%s: out: in place (out == ids) needs the strides of ids", fn);
  FGVC_REQUIRE(min_area >= 0, FGVC_ERR_INVALID_ARG, "%s: min_area=%d (at least 0)", fn, min_area);
  FGVC_REQUIRE(keep_largest == 0 || keep_largest == 1, FGVC_ERR_INVALID_ARG, "%s: keep_largest=%d (0 or 1)", fn, keep_largest);
  FGVC_REQUIRE(fill_holes == 0 || fill_holes == 1, FGVC_ERR_INVALID_ARG, "%s: fill_holes=%d (0 or 1)", fn, fill_holes);
  const size_t need = clean_workspace_bytes(T, h, w, n_ids);
  FGVC_REQUIRE(workspace_bytes >= need, FGVC_ERR_INVALID_ARG, "%s: workspace_bytes=%zu, %zu needed (fgvc_seg_clean_workspace_bytes)", fn,
               workspace_bytes, need);
  return clean_launch(ids, ids_stride_t, ids_stride_y, T, h, w, n_ids, connectivity, min_area, keep_largest, fill_holes, max_hole_area, frame_flags,
                      out, out_stride_t, out_stride_y, stats, workspace, (hipStream_t)stream);
}

int fgvc_seg_object_windows_i64(const int64_t* stats, int T, int n_ids, const int32_t* objects, int M, int size_h, int size_w, int pad_q,
                                int min_side, int smooth, int mask_h, int mask_w, int frame_h, int frame_w, int64_t* windows, void* stream) {
  const char* fn = "fgvc_seg_object_windows_i64";
  FGVC_REQUIRE(T >= 0 && M >= 0, FGVC_ERR_INVALID_ARG, "%s: T=%d, M=%d (at least 0)", fn, T, M);
  FGVC_REQUIRE(n_ids >= 1, FGVC_ERR_INVALID_ARG, "%s: n_ids=%d (at least 1)", fn, n_ids);
  FGVC_REQUIRE(size_h >= 1 && size_h <= 1024 && size_w >= 1 && size_w <= 1024, FGVC_ERR_INVALID_ARG, "%s: size = %d, %d (1 .. 1024 a side)", fn,
               size_h, size_w);
  FGVC_REQUIRE(pad_q >= 0 && pad_q <= 4096, FGVC_ERR_INVALID_ARG, "%s: pad_q=%d (0 .. 4096 = pad 0 .. 4 in 1/1024)", fn, pad_q);
  FGVC_REQUIRE(min_side >= 1 && min_side <= 32768, FGVC_ERR_INVALID_ARG, "%s: min_side=%d (1 .. 32768)", fn, min_side);
  FGVC_REQUIRE(smooth >= 0 && smooth < (1 << 20), FGVC_ERR_INVALID_ARG, "%s: smooth=%d (0 .. 2^20 - 1)", fn, smooth);
  FGVC_REQUIRE(mask_h >= 1 && mask_h <= 32768 && mask_w >= 1 && mask_w <= 32768, FGVC_ERR_INVALID_ARG,
               "%s: mask_h, mask_w = %d, %d (1 .. 32768)", fn, mask_h, mask_w);
  FGVC_REQUIRE(frame_h >= 1 && frame_h <= 32768 && frame_w >= 1 && frame_w <= 32768, FGVC_ERR_INVALID_ARG,
               "%s: frame_h, frame_w = %d, %d (1 .. 32768)", fn, frame_h, frame_w);
  if (T == 0 || M == 0) return FGVC_OK;
  FGVC_REQUIRE(stats && objects && windows, FGVC_ERR_INVALID_ARG, "%s: stats, objects or windows: null pointer", fn);
  FGVC_REQUIRE((long long)T * M < (1ll << 31), FGVC_ERR_INVALID_ARG, "%s: T M = %lld windows (below 2^31)", fn, (long long)T * M);
  return object_windows_launch(stats, T, n_ids, objects, M, size_h, size_w, pad_q, min_side, smooth, mask_h, mask_w, frame_h, frame_w, windows,
                               (hipStream_t)stream);
}

size_t fgvc_frames_object_crops_workspace_bytes(int T, int M, int size_h, int size_w, int max_taps) {
  if (T < 1 || M < 1 || size_h < 1 || size_h > 1024 || size_w < 1 || size_w > 1024 || max_taps < 4 || max_taps > 256) return 0;
  return object_crops_workspace_bytes(T, M, size_h, size_w, max_taps);
}

int fgvc_frames_object_crops_u8(const uint8_t* frames, int T, int H, int W, int64_t frames_stride_t, int64_t frames_stride_y,
                                int64_t frames_stride_x, int64_t frames_stride_c, const int64_t* windows, int window_words, int M, int size_h,
                                int size_w, int fill_r, int fill_g, int fill_b, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                                int mask_h, int mask_w, const int32_t* objects, int max_taps, uint8_t* crops, uint8_t* masks, void* workspace,
                                size_t workspace_bytes, void* stream) {
  const char* fn = "fgvc_frames_object_crops_u8";
  FGVC_REQUIRE(T >= 0 && M >= 0, FGVC_ERR_INVALID_ARG, "%s: T=%d, M=%d (at least 0)", fn, T, M);
  FGVC_REQUIRE(H >= 1 && H <= 32768 && W >= 1 && W <= 32768, FGVC_ERR_INVALID_ARG, "%s: H, W = %d, %d (1 .. 32768)", fn, H, W);
  FGVC_REQUIRE(window_words == 4 || window_words == 8, FGVC_ERR_INVALID_ARG, "%s: window_words=%d (4 or 8)", fn, window_words);
  FGVC_REQUIRE(size_h >= 1 && size_h <= 1024 && size_w >= 1 && size_w <= 1024, FGVC_ERR_INVALID_ARG, "%s: size = %d, %d (1 .. 1024 a side)", fn,
               size_h, size_w);
  FGVC_REQUIRE(max_taps >= 4 && max_taps <= 256, FGVC_ERR_INVALID_ARG, "%s: max_taps=%d (4 .. 256 taps per axis)", fn, max_taps);
  FGVC_REQUIRE((unsigned)fill_r < 256u && (unsigned)fill_g < 256u && (unsigned)fill_b < 256u, FGVC_ERR_INVALID_ARG,
               "%s: fill = %d, %d, %d (bytes)", fn, fill_r, fill_g, fill_b);
  FGVC_REQUIRE((masks != nullptr) == (ids != nullptr), FGVC_ERR_INVALID_ARG, "%s: ids and masks: both or neither", fn);
  if (T == 0 || M == 0) return FGVC_OK;
  FGVC_REQUIRE(frames && windows && crops, FGVC_ERR_INVALID_ARG, "%s: frames, windows or crops: null pointer", fn);
  FGVC_REQUIRE((reinterpret_cast<uintptr_t>(windows) & 7u) == 0, FGVC_ERR_INVALID_ARG, "%s: windows: must be 8-byte aligned", fn);
  if (ids) {
    FGVC_REQUIRE(objects, FGVC_ERR_INVALID_ARG, "%s: objects: null pointer with ids", fn);
    FGVC_REQUIRE(mask_h >= 1 && mask_h <= 32768 && mask_w >= 1 && mask_w <= 32768, FGVC_ERR_INVALID_ARG,
                 "%s: mask_h, mask_w = %d, %d (1 .. 32768)", fn, mask_h, mask_w);
    FGVC_REQUIRE(ids_stride_y >= mask_w && (T == 1 || ids_stride_t >= 0), FGVC_ERR_INVALID_ARG,
                 "%s: ids_stride_y: a row stride of at least mask_w = %d bytes and a non-negative frame stride, got %lld, %lld", fn, mask_w,
                 (long long)ids_stride_y, (long long)ids_stride_t);
  }
  FGVC_REQUIRE(object_crops_blocks(T, M, size_h, size_w) > 0, FGVC_ERR_INVALID_ARG, "%s: T M = %lld crops of %d x %d: too many workgroups", fn,
               (long long)T * M, size_h, size_w);
  FGVC_REQUIRE(workspace, FGVC_ERR_INVALID_ARG, "%s: workspace: null pointer", fn);
  FGVC_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, FGVC_ERR_INVALID_ARG, "%s: workspace: must be 4-byte aligned", fn);
  const size_t need = object_crops_workspace_bytes(T, M, size_h, size_w, max_taps);
  FGVC_REQUIRE(workspace_bytes >= need, FGVC_ERR_INVALID_ARG, "%s: workspace_bytes=%zu, %zu needed (fgvc_frames_object_crops_workspace_bytes)",
               fn, workspace_bytes, need);
  return object_crops_launch(frames, T, H, W, frames_stride_t, frames_stride_y, frames_stride_x, frames_stride_c, windows, window_words, M, size_h,
                             size_w, fill_r, fill_g, fill_b, ids, ids_stride_t, ids_stride_y, mask_h, mask_w, objects, max_taps, crops, masks,
                             workspace, (hipStream_t)stream);
}

int fgvc_render_tile_rows(void) {
  int rows, cols;
  render_tile(&rows, &cols);
  return rows;
}

int fgvc_render_tile_cols(void) {
  int rows, cols;
  render_tile(&rows, &cols);
  return cols;
}

// The three render entries share their 25 leading arguments (render_host.hpp's RenderCall) and the two sets of checks below; `fn` is the
// entry's name.  First the sizes, which come before the "no pixel exists" return ...
static int render_check_sizes(const char* fn, const RenderCall& c) {
  FGVC_REQUIRE(c.T >= 0 && c.h >= 0 && c.w >= 0, FGVC_ERR_INVALID_ARG, "%s: negative size (T=%d, %d x %d)", fn, c.T, c.h, c.w);
  FGVC_REQUIRE(c.P >= 0, FGVC_ERR_INVALID_ARG, "%s: P=%d", fn, c.P);
  FGVC_REQUIRE((long long)c.h * c.w < (1ll << 29), FGVC_ERR_INVALID_ARG, "%s: a frame of %d x %d has 2^29 pixels or more", fn, c.h, c.w);
  return FGVC_OK;
}

// ... then the operands: pointers, strides, the overlay's, and (dots: the entry will run the point stage) the radius.  What else the points
// need differs between the entries and stays with each.
static int render_check_operands(const char* fn, const RenderCall& c, bool dots) {
  FGVC_REQUIRE(c.frames && c.out, FGVC_ERR_INVALID_ARG, "%s: null pointer", fn);
  const long long row = 3ll * c.w;
  FGVC_REQUIRE(c.f_sy >= row && (c.T == 1 || c.f_st >= 0), FGVC_ERR_INVALID_ARG,
               "%s: frames: a row stride of at least 3 w = %lld bytes, got %lld", fn, row, c.f_sy);
  FGVC_REQUIRE(c.o_sy >= row && (c.T == 1 || c.o_st >= (long long)(c.h - 1) * c.o_sy + row), FGVC_ERR_INVALID_ARG,
               "%s: out: rows and frames must not overlap (strides %lld, %lld bytes for %d x %d)", fn, c.o_st, c.o_sy, c.h, c.w);
  if (c.ids) {
    FGVC_REQUIRE(c.palette, FGVC_ERR_INVALID_ARG, "%s: ids without a palette", fn);
    FGVC_REQUIRE(c.alpha >= 0 && c.alpha <= 256, FGVC_ERR_INVALID_ARG, "%s: alpha=%d (0 .. 256)", fn, c.alpha);
    FGVC_REQUIRE(c.i_sy >= c.w && (c.T == 1 || c.i_st >= 0), FGVC_ERR_INVALID_ARG,
                 "%s: ids: a row stride of at least w = %d bytes, got %lld", fn, c.w, c.i_sy);
  }
  if (dots) {
    FGVC_REQUIRE(c.radius >= 1, FGVC_ERR_INVALID_ARG, "%s: radius=%d (at least 1)", fn, c.radius);
    FGVC_REQUIRE(c.radius <= 31, FGVC_ERR_UNSUPPORTED, "%s: radius=%d beyond 31", fn, c.radius);
  }
  return FGVC_OK;
}

static bool aligned8(const void* p, const void* q, const void* r = nullptr) {
  return ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(r)) & 7u) == 0;
}

int fgvc_render_frames_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                          int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                          const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                          int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                          const uint8_t* colors, int P, int radius, const double* icon, void* stream) {
  const char* fn = "fgvc_render_frames_u8";
  const RenderCall c{frames, frames_stride_t, frames_stride_y, out, out_stride_t, out_stride_y, T, h, w, ids, ids_stride_t, ids_stride_y,
                     palette, alpha, contour != 0, tracks, tracks_stride_p, tracks_stride_t, visibles, visibles_stride_p, visibles_stride_t,
                     colors, P, radius, icon};
  if (int rc = render_check_sizes(fn, c)) return rc;
  if (T == 0 || h == 0 || w == 0) return FGVC_OK;                     // no pixel exists
  if (int rc = render_check_operands(fn, c, tracks && P > 0)) return rc;
  if (tracks && P > 0) {
    FGVC_REQUIRE(colors && icon, FGVC_ERR_INVALID_ARG, "%s: tracks without colors or the icon table", fn);
    FGVC_REQUIRE(aligned8(tracks, icon), FGVC_ERR_INVALID_ARG, "%s: tracks and icon must be 8-byte aligned", fn);
  }
  return render_frames_launch(c, (hipStream_t)stream);
}

int fgvc_render_trails_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                          int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                          const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                          int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                          const uint8_t* colors, int P, int radius, const double* icon, int trail, double linewidth, double ro2, double g,
                          const double* fade, const uint8_t* time_colors, void* stream) {
  const char* fn = "fgvc_render_trails_u8";
  const RenderCall c{frames, frames_stride_t, frames_stride_y, out, out_stride_t, out_stride_y, T, h, w, ids, ids_stride_t, ids_stride_y,
                     palette, alpha, contour != 0, tracks, tracks_stride_p, tracks_stride_t, visibles, visibles_stride_p, visibles_stride_t,
                     colors, P, radius, icon};
  if (int rc = render_check_sizes(fn, c)) return rc;
  FGVC_REQUIRE(trail >= 1 && trail <= 64, FGVC_ERR_INVALID_ARG, "%s: trail=%d (1 .. 64)", fn, trail);
  FGVC_REQUIRE(linewidth >= 1.0 && linewidth <= 16.0, FGVC_ERR_INVALID_ARG, "%s: linewidth=%g (1 .. 16)", fn, linewidth);
  FGVC_REQUIRE((long long)P * trail < (1ll << 30), FGVC_ERR_UNSUPPORTED, "%s: P * trail = %lld items, 2^30 or more", fn, (long long)P * trail);
  if (T == 0 || h == 0 || w == 0) return FGVC_OK;                     // no pixel exists
  if (int rc = render_check_operands(fn, c, P > 0 && icon)) return rc;
  if (P > 0) {
    FGVC_REQUIRE(tracks && fade, FGVC_ERR_INVALID_ARG, "%s: null tracks or fade table", fn);
    FGVC_REQUIRE(colors || (time_colors && !icon), FGVC_ERR_INVALID_ARG, "%s: neither colors nor time_colors", fn);
    FGVC_REQUIRE(T == 1 || tracks_stride_t >= 0, FGVC_ERR_INVALID_ARG, "%s: tracks: a negative frame stride (%lld)", fn, c.trk_st);
    FGVC_REQUIRE(T == 1 || !visibles || visibles_stride_t >= 0, FGVC_ERR_INVALID_ARG, "%s: visibles: a negative frame stride (%lld)", fn,
                 c.vis_st);
    FGVC_REQUIRE(ro2 > 0.0 && g > 0.0 && ro2 <= 81.0, FGVC_ERR_INVALID_ARG, "%s: ro2=%g, g=%g (both positive, ro2 <= 81)", fn, ro2, g);
    FGVC_REQUIRE(aligned8(tracks, icon, fade), FGVC_ERR_INVALID_ARG, "%s: tracks, icon and fade must be 8-byte aligned", fn);
  }
  const int reach = (int)ceil(linewidth / 2.0 + 0.5);                 // ceil(ro): what a segment's box is grown by
  return render_trails_launch(c, trail, reach, ro2, g, fade, time_colors, (hipStream_t)stream);
}

int fgvc_render_pose_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                        int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                        const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                        int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                        const uint8_t* colors, int P, int radius, const double* icon, const int32_t* skeleton, int E,
                        const uint8_t* limb_colors, double limb_width, double ro2, double g, double limb_alpha, const void* heat, int heat_f64,
                        int K, int64_t heat_stride_t, int64_t heat_stride_k, int64_t heat_stride_y, const uint8_t* heat_colors,
                        double heat_gain, double heat_alpha, void* stream) {
  const char* fn = "fgvc_render_pose_u8";
  const RenderCall c{frames, frames_stride_t, frames_stride_y, out, out_stride_t, out_stride_y, T, h, w, ids, ids_stride_t, ids_stride_y,
                     palette, alpha, contour != 0, tracks, tracks_stride_p, tracks_stride_t, visibles, visibles_stride_p, visibles_stride_t,
                     colors, P, radius, icon};
  if (int rc = render_check_sizes(fn, c)) return rc;
  FGVC_REQUIRE(E >= 0, FGVC_ERR_INVALID_ARG, "%s: E=%d", fn, E);
  FGVC_REQUIRE(E < (1 << 30), FGVC_ERR_UNSUPPORTED, "%s: E = %d limbs, 2^30 or more", fn, E);
  FGVC_REQUIRE(!heat || (K >= 1 && K <= 256), FGVC_ERR_INVALID_ARG, "%s: K=%d heat maps (1 .. 256)", fn, K);
  if (T == 0 || h == 0 || w == 0) return FGVC_OK;                     // no pixel exists
  if (int rc = render_check_operands(fn, c, P > 0 && icon)) return rc;
  if (heat) {
    FGVC_REQUIRE(heat_colors, FGVC_ERR_INVALID_ARG, "%s: heat without heat_colors", fn);
    FGVC_REQUIRE(isfinite(heat_gain) && heat_gain > 0.0, FGVC_ERR_INVALID_ARG, "%s: heat_gain=%g (finite, > 0)", fn, heat_gain);
    FGVC_REQUIRE(heat_alpha >= 0.0 && heat_alpha <= 1.0, FGVC_ERR_INVALID_ARG, "%s: heat_alpha=%g (0 .. 1)", fn, heat_alpha);
    FGVC_REQUIRE(heat_stride_y >= w && (T == 1 || heat_stride_t >= 0) && (K == 1 || heat_stride_k >= 0), FGVC_ERR_INVALID_ARG,
                 "%s: heat: a row stride of at least w = %d elements and non-negative strides, got %lld, %lld, %lld", fn, w,
                 (long long)heat_stride_t, (long long)heat_stride_k, (long long)heat_stride_y);
    FGVC_REQUIRE((reinterpret_cast<uintptr_t>(heat) & (heat_f64 ? 7u : 3u)) == 0, FGVC_ERR_INVALID_ARG,
                 "%s: heat must be aligned to its element size", fn);
  }
  if (P > 0 && (E > 0 || icon)) {
    FGVC_REQUIRE(tracks, FGVC_ERR_INVALID_ARG, "%s: limbs or dots without tracks", fn);
    FGVC_REQUIRE(T == 1 || tracks_stride_t >= 0, FGVC_ERR_INVALID_ARG, "%s: tracks: a negative frame stride (%lld)", fn, c.trk_st);
    FGVC_REQUIRE(T == 1 || !visibles || visibles_stride_t >= 0, FGVC_ERR_INVALID_ARG, "%s: visibles: a negative frame stride (%lld)", fn,
                 c.vis_st);
    if (E > 0) {
      FGVC_REQUIRE(skeleton && limb_colors, FGVC_ERR_INVALID_ARG, "%s: limbs without a skeleton or limb_colors", fn);
      FGVC_REQUIRE(limb_width >= 1.0 && limb_width <= 16.0, FGVC_ERR_INVALID_ARG, "%s: limb_width=%g (1 .. 16)", fn, limb_width);
      FGVC_REQUIRE(limb_alpha >= 0.0 && limb_alpha <= 1.0, FGVC_ERR_INVALID_ARG, "%s: limb_alpha=%g (0 .. 1)", fn, limb_alpha);
      FGVC_REQUIRE(ro2 > 0.0 && g > 0.0 && ro2 <= 81.0, FGVC_ERR_INVALID_ARG, "%s: ro2=%g, g=%g (both positive, ro2 <= 81)", fn, ro2, g);
      FGVC_REQUIRE((reinterpret_cast<uintptr_t>(skeleton) & 3u) == 0, FGVC_ERR_INVALID_ARG, "%s: skeleton must be 4-byte aligned", fn);
    }
    FGVC_REQUIRE(!icon || colors, FGVC_ERR_INVALID_ARG, "%s: dots without colors", fn);
    FGVC_REQUIRE(aligned8(tracks, icon), FGVC_ERR_INVALID_ARG, "%s: tracks and icon must be 8-byte aligned", fn);
  }
  const int reach = E > 0 ? (int)ceil(limb_width / 2.0 + 0.5) : 0;    // ceil(ro): what a limb's box is grown by
  return render_pose_launch(c, skeleton, E, limb_colors, reach, ro2, g, limb_alpha, heat, heat_f64 != 0, heat ? K : 0, heat_stride_t,
                            heat_stride_k, heat_stride_y, heat_colors, heat_gain, heat_alpha, (hipStream_t)stream);
}

int fgvc_render_boxes_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                         int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                         const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                         int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                         const uint8_t* colors, int P, int radius, const double* icon, const int32_t* boxes, int64_t boxes_stride_t,
                         const uint8_t* box_visibles, int64_t box_visibles_stride_t, const uint8_t* box_colors, int N, int box_width,
                         int box_alpha, const int32_t* box_labels, int label_scale, const uint8_t* digits, void* stream) {
  const char* fn = "fgvc_render_boxes_u8";
  const RenderCall c{frames, frames_stride_t, frames_stride_y, out, out_stride_t, out_stride_y, T, h, w, ids, ids_stride_t, ids_stride_y,
                     palette, alpha, contour != 0, tracks, tracks_stride_p, tracks_stride_t, visibles, visibles_stride_p, visibles_stride_t,
                     colors, P, radius, icon};
  if (int rc = render_check_sizes(fn, c)) return rc;
  FGVC_REQUIRE(N >= 0 && N <= 255, FGVC_ERR_INVALID_ARG, "%s: N=%d boxes (0 .. 255)", fn, N);
  FGVC_REQUIRE(box_width >= 1 && box_width <= 16, FGVC_ERR_INVALID_ARG, "%s: box_width=%d (1 .. 16)", fn, box_width);
  FGVC_REQUIRE(box_alpha >= 0 && box_alpha <= 256, FGVC_ERR_INVALID_ARG, "%s: box_alpha=%d (0 .. 256)", fn, box_alpha);
  FGVC_REQUIRE(label_scale >= 1 && label_scale <= 4, FGVC_ERR_INVALID_ARG, "%s: label_scale=%d (1 .. 4)", fn, label_scale);
  if (T == 0 || h == 0 || w == 0) return FGVC_OK;                     // no pixel exists
  if (int rc = render_check_operands(fn, c, tracks && P > 0)) return rc;
  if (tracks && P > 0) {
    FGVC_REQUIRE(colors && icon, FGVC_ERR_INVALID_ARG, "%s: tracks without colors or the icon table", fn);
    FGVC_REQUIRE(aligned8(tracks, icon), FGVC_ERR_INVALID_ARG, "%s: tracks and icon must be 8-byte aligned", fn);
  }
  if (N > 0) {
    FGVC_REQUIRE(boxes && box_colors, FGVC_ERR_INVALID_ARG, "%s: boxes or box_colors: null pointer", fn);
    FGVC_REQUIRE((reinterpret_cast<uintptr_t>(boxes) & 3u) == 0 && (reinterpret_cast<uintptr_t>(box_labels) & 3u) == 0, FGVC_ERR_INVALID_ARG,
                 "%s: boxes and box_labels must be 4-byte aligned", fn);
    FGVC_REQUIRE(T == 1 || (boxes_stride_t >= 0 && (!box_visibles || box_visibles_stride_t >= 0)), FGVC_ERR_INVALID_ARG,
                 "%s: boxes, box_visibles: a negative frame stride (%lld, %lld)", fn, (long long)boxes_stride_t,
                 (long long)box_visibles_stride_t);
    FGVC_REQUIRE(!box_labels || digits, FGVC_ERR_INVALID_ARG, "%s: box_labels without the digits table", fn);
  }
  return render_boxes_launch(c, boxes, boxes_stride_t, box_visibles, box_visibles_stride_t, box_colors, N, box_width, box_alpha, box_labels,
                             label_scale, digits, (hipStream_t)stream);
}

int fgvc_c2f_refine_f32(const int32_t* coarse_arg, const float* qfine, const float* kfine, const float* vfine, int T,
                        int H, int W, int scale, int Cf, int P, int Rf, int topk, float temperature, float* out,
                        int32_t* idx_out, float* logit_out, void* stream) {
  return fgvc_c2f_refine_mode_f32(coarse_arg, qfine, kfine, vfine, T, H, W, scale, Cf, P, Rf, topk, temperature, FGVC_WEIGHT_SOFTMAX,
                                  out, idx_out, logit_out, stream);
}

int fgvc_c2f_refine_mode_f32(const int32_t* coarse_arg, const float* qfine, const float* kfine, const float* vfine, int T,
                             int H, int W, int scale, int Cf, int P, int Rf, int topk, float temperature, int weight_mode,
                             float* out, int32_t* idx_out, float* logit_out, void* stream) {
  FGVC_REQUIRE(coarse_arg && qfine && kfine && vfine && out && idx_out && logit_out, FGVC_ERR_INVALID_ARG,
               "fgvc_c2f_refine_f32: null pointer");
  FGVC_REQUIRE(T >= 1 && H > 0 && W > 0 && scale >= 1 && P > 0 && Rf >= 0, FGVC_ERR_INVALID_ARG, "fgvc_c2f_refine_f32: bad shape");
  FGVC_REQUIRE(Cf > 0 && Cf % 4 == 0, FGVC_ERR_UNSUPPORTED, "fgvc_c2f_refine_f32: Cf=%d must be a multiple of 4", Cf);
  FGVC_REQUIRE(aligned16(qfine) && aligned16(kfine), FGVC_ERR_INVALID_ARG, "fgvc_c2f_refine_f32: 16-byte alignment required");
  FGVC_REQUIRE(topk >= 1 && topk <= 16, FGVC_ERR_UNSUPPORTED, "fgvc_c2f_refine_f32: topk=%d outside 1..16", topk);
  FGVC_REQUIRE(temperature > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_c2f_refine_f32: temperature must be > 0");
  FGVC_REQUIRE(weight_mode == FGVC_WEIGHT_SOFTMAX || weight_mode == FGVC_WEIGHT_COSINE, FGVC_ERR_INVALID_ARG,
               "fgvc_c2f_refine_mode_f32: weight_mode %d (FGVC_WEIGHT_SOFTMAX or FGVC_WEIGHT_COSINE)", weight_mode);
  return c2f_refine_launch(coarse_arg, qfine, kfine, vfine, T, H, W, scale, Cf, P, Rf, topk, temperature, weight_mode, out,
                           idx_out, logit_out, (hipStream_t)stream);
}

int fgvc_bn_act_f32(const float* x, const float* residual, const float* mean, const float* var, const float* gamma,
                    const float* beta, float eps, int relu, float* out, int N, int C, int HW, void* stream) {
  FGVC_REQUIRE(x && mean && var && gamma && beta && out, FGVC_ERR_INVALID_ARG, "fgvc_bn_act_f32: null pointer");
  FGVC_REQUIRE(N >= 0 && C > 0 && HW > 0 && eps >= 0.f, FGVC_ERR_INVALID_ARG, "fgvc_bn_act_f32: bad shape");
  if (N == 0) return FGVC_OK;
  return bn_act_launch(x, residual, mean, var, gamma, beta, eps, relu, out, N, C, HW, (hipStream_t)stream);
}

static bool conv_pad_ok(int H, int W, int Hp, int Wp) {
  return Hp >= 8 * cdiv(H, 8) + 2 && Wp >= 32 * cdiv(W, 32) + 8;
}

int fgvc_nchw_to_split_nhwc_f32(const float* in, uint16_t* out, float* out_f32, int N, int C, int H, int W, int Hp, int Wp,
                                void* stream) {
  FGVC_REQUIRE(in && (out || out_f32), FGVC_ERR_INVALID_ARG, "fgvc_nchw_to_split_nhwc_f32: null pointer");
  FGVC_REQUIRE(N >= 0 && C > 0 && C % 32 == 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_nchw_to_split_nhwc_f32: bad shape (C must be a multiple of 32)");
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG,
               "fgvc_nchw_to_split_nhwc_f32: padded size %dx%d too small for %dx%d (need >= 8*ceil(H/8)+2 x 32*ceil(W/32)+8)", Hp, Wp, H, W);
  FGVC_REQUIRE(aligned16(out) && aligned16(out_f32) && (long long)N * (C / 32) <= 65535 && H <= 65535, FGVC_ERR_INVALID_ARG,
               "fgvc_nchw_to_split_nhwc_f32: alignment / grid limits");
  if (N == 0) return FGVC_OK;
  return nchw_to_split_nhwc_launch(in, out, out_f32, N, C, H, W, Hp, Wp, (hipStream_t)stream);
}

int fgvc_conv_split_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, uint16_t* y_split,
                        float* y_f32, int N, int H, int W, int Hp, int Wp, int Cin, int Cout, int KS, int relu,
                        void* stream) {
  return fgvc_conv_split_fmt_f32(x, w, bias, residual, y_split, y_f32, N, H, W, Hp, Wp, Cin, Cout, KS, relu, FGVC_ACT_BF16X2, 0,
                                 FGVC_ACT_BF16X2, 0, nullptr, stream);
}

int fgvc_conv_split_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, uint16_t* y_split,
                            float* y_f32, int N, int H, int W, int Hp, int Wp, int Cin, int Cout, int KS, int relu, int in_fmt,
                            int in_scale_log2, int out_fmt, int out_scale_log2, int* overflow, void* stream) {
  FGVC_REQUIRE(x && w && bias && (y_split || y_f32), FGVC_ERR_INVALID_ARG, "fgvc_conv_split_f32: null pointer");
  FGVC_REQUIRE(in_fmt >= 0 && in_fmt <= 3 && out_fmt >= 0 && out_fmt <= 3, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_fmt_f32: unknown format %d / %d", in_fmt, out_fmt);
  FGVC_REQUIRE(out_fmt == FGVC_ACT_BF16X2 || !y_split || overflow, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_fmt_f32: an f16-format output needs the overflow word");
  FGVC_REQUIRE(in_scale_log2 > -100 && in_scale_log2 < 100 && out_scale_log2 > -100 && out_scale_log2 < 100, FGVC_ERR_INVALID_ARG,
               "fgvc_conv_split_fmt_f32: scale exponent out of range");
  FGVC_REQUIRE(N >= 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_f32: bad shape");
  FGVC_REQUIRE(KS == 1 || KS == 3, FGVC_ERR_UNSUPPORTED, "fgvc_conv_split_f32: kernel size %d (1 or 3, stride 1)", KS);
  FGVC_REQUIRE(Cin > 0 && Cin % 32 == 0 && Cout > 0 && Cout % 64 == 0, FGVC_ERR_UNSUPPORTED,
               "fgvc_conv_split_f32: Cin=%d must be a multiple of 32 and Cout=%d of 64", Cin, Cout);
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG, "fgvc_conv_split_f32: padded size %dx%d too small for %dx%d", Hp, Wp, H, W);
  FGVC_REQUIRE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(residual) && aligned16(y_split) && aligned16(y_f32),
               FGVC_ERR_INVALID_ARG, "fgvc_conv_split_f32: 16-byte alignment required");
  FGVC_REQUIRE((const void*)x != (const void*)y_split, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_f32: in-place not supported");
  if (N == 0) return FGVC_OK;
  return conv_split_launch(x, w, bias, residual, y_split, y_f32, N, H, W, Hp, Wp, Cin, Cout, KS, relu, in_fmt, in_scale_log2, out_fmt,
                           out_scale_log2, overflow, (hipStream_t)stream);
}

int fgvc_conv_split_proj_fmt_f32(const uint16_t* x, const uint16_t* w, const uint16_t* x2, const uint16_t* w2, const float* bias,
                                 const float* residual, uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp, int Cin, int Cin2,
                                 int relu, int in_fmt, int in_scale_log2, int out_fmt, int out_scale_log2, int* overflow, void* stream) {
  FGVC_REQUIRE(x && w && x2 && w2 && bias && (y_split || y_f32), FGVC_ERR_INVALID_ARG, "fgvc_conv_split_proj_fmt_f32: null pointer");
  FGVC_REQUIRE(in_fmt >= 0 && in_fmt <= 3 && out_fmt >= 0 && out_fmt <= 3, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_proj_fmt_f32: unknown format %d / %d", in_fmt, out_fmt);
  FGVC_REQUIRE(out_fmt == FGVC_ACT_BF16X2 || !y_split || overflow, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_proj_fmt_f32: an f16-format output needs the overflow word");
  FGVC_REQUIRE(in_scale_log2 > -100 && in_scale_log2 < 100 && out_scale_log2 > -100 && out_scale_log2 < 100, FGVC_ERR_INVALID_ARG,
               "fgvc_conv_split_proj_fmt_f32: scale exponent out of range");
  FGVC_REQUIRE(N >= 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_proj_fmt_f32: bad shape");
  FGVC_REQUIRE(Cin > 0 && Cin % 32 == 0 && Cin2 > 0 && Cin2 % 32 == 0, FGVC_ERR_UNSUPPORTED,
               "fgvc_conv_split_proj_fmt_f32: Cin=%d and Cin2=%d must be multiples of 32 (Cout is 256)", Cin, Cin2);
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG, "fgvc_conv_split_proj_fmt_f32: padded size %dx%d too small for %dx%d", Hp, Wp, H, W);
  FGVC_REQUIRE(aligned16(x) && aligned16(w) && aligned16(x2) && aligned16(w2) && aligned16(bias) && aligned16(residual) && aligned16(y_split) &&
               aligned16(y_f32), FGVC_ERR_INVALID_ARG, "fgvc_conv_split_proj_fmt_f32: 16-byte alignment required");
  FGVC_REQUIRE((const void*)x != (const void*)y_split && (const void*)x2 != (const void*)y_split, FGVC_ERR_INVALID_ARG,
               "fgvc_conv_split_proj_fmt_f32: in-place not supported");
  if (N == 0) return FGVC_OK;
  return conv_split_launch(x, w, bias, residual, y_split, y_f32, N, H, W, Hp, Wp, Cin, 256, 3, relu, in_fmt, in_scale_log2, out_fmt,
                           out_scale_log2, overflow, (hipStream_t)stream, nullptr, 1, x2, w2, Cin2);
}

static int conv_split_bank_common(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, void* bank, int N,
                                  int H, int W, int Hp, int Wp, int Cin, int KS, int relu, int in_fmt, int in_scale_log2,
                                  int normalize, void* stream, int row_bytes) {
  FGVC_REQUIRE(x && w && bias && bank, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_bank_f16f6p_f32: null pointer");
  FGVC_REQUIRE(in_fmt >= 0 && in_fmt <= 3, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_bank_f16f6p_f32: unknown format %d", in_fmt);
  FGVC_REQUIRE(in_scale_log2 > -100 && in_scale_log2 < 100, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_bank_f16f6p_f32: scale exponent out of range");
  FGVC_REQUIRE(N >= 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "fgvc_conv_split_bank_f16f6p_f32: bad shape");
  FGVC_REQUIRE(KS == 3, FGVC_ERR_UNSUPPORTED, "fgvc_conv_split_bank_f16f6p_f32: kernel size %d (3 x 3, stride 1: the last convolution of a BasicBlock)", KS);
  FGVC_REQUIRE(Cin > 0 && Cin % 32 == 0, FGVC_ERR_UNSUPPORTED, "fgvc_conv_split_bank_f16f6p_f32: Cin=%d must be a multiple of 32 (Cout is 256)", Cin);
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG, "fgvc_conv_split_bank_f16f6p_f32: padded size %dx%d too small for %dx%d", Hp, Wp, H, W);
  FGVC_REQUIRE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(residual) && aligned16(bank), FGVC_ERR_INVALID_ARG,
               "fgvc_conv_split_bank_f16f6p_f32: 16-byte alignment required");
  if (N == 0) return FGVC_OK;
  return conv_split_launch(x, w, bias, residual, nullptr, nullptr, N, H, W, Hp, Wp, Cin, 256, KS, relu, in_fmt, in_scale_log2, 0, 0, nullptr,
                           (hipStream_t)stream, reinterpret_cast<unsigned char*>(bank), normalize, nullptr, nullptr, 0, row_bytes);
}

int fgvc_conv_split_bank_f16f6p_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, void* bank, int N,
                                    int H, int W, int Hp, int Wp, int Cin, int KS, int relu, int in_fmt, int in_scale_log2,
                                    int normalize, void* stream) {
  return conv_split_bank_common(x, w, bias, residual, bank, N, H, W, Hp, Wp, Cin, KS, relu, in_fmt, in_scale_log2, normalize, stream, 1024);
}

int fgvc_conv_split_bank_f16f6x_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, void* bank, int N,
                                    int H, int W, int Hp, int Wp, int Cin, int KS, int relu, int in_fmt, int in_scale_log2,
                                    int normalize, void* stream) {
  return conv_split_bank_common(x, w, bias, residual, bank, N, H, W, Hp, Wp, Cin, KS, relu, in_fmt, in_scale_log2, normalize, stream, 2048);
}

/* debug: the 32 s_memtime sums workgroup 77 leaves with fgvc_set_option("conv64_variant", 8) (tools/experiments/time_conv64_variants.py) */
int fgvc_conv64_probe(int64_t* out32) {
  FGVC_REQUIRE(out32 != nullptr, FGVC_ERR_INVALID_ARG, "fgvc_conv64_probe: null pointer");
  return conv64_probe_read(reinterpret_cast<long long*>(out32)) == 0 ? FGVC_OK : FGVC_ERR_LAUNCH;
}

int fgvc_conv64_split_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, uint16_t* y_split,
                          float* y_f32, int N, int H, int W, int Hp, int Wp, int relu, void* stream) {
  return fgvc_conv64_split_res_f32(x, w, bias, residual, nullptr, y_split, y_f32, N, H, W, Hp, Wp, relu, stream);
}

int fgvc_conv64_split_res_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual,
                              const uint16_t* residual_split, uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp,
                              int relu, void* stream) {
  return fgvc_conv64_split_fmt_f32(x, w, bias, residual, residual_split, y_split, y_f32, N, H, W, Hp, Wp, relu, FGVC_ACT_BF16X2, 0,
                                   FGVC_ACT_BF16X2, 0, nullptr, stream);
}

int fgvc_conv64_split_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual,
                              const uint16_t* residual_split, uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp,
                              int relu, int in_fmt, int in_scale_log2, int out_fmt, int out_scale_log2, int* overflow, void* stream) {
  FGVC_REQUIRE(x && w && bias && (y_split || y_f32), FGVC_ERR_INVALID_ARG, "fgvc_conv64_split_f32: null pointer");
  FGVC_REQUIRE((in_fmt == FGVC_ACT_BF16X2 || in_fmt == FGVC_ACT_F16F8) && (out_fmt == FGVC_ACT_BF16X2 || out_fmt == FGVC_ACT_F16F8),
               FGVC_ERR_UNSUPPORTED, "fgvc_conv64_split_fmt_f32: formats %d -> %d (bf16x2 or f16f8)", in_fmt, out_fmt);
  FGVC_REQUIRE(out_fmt == FGVC_ACT_BF16X2 || !y_split || overflow, FGVC_ERR_INVALID_ARG,
               "fgvc_conv64_split_fmt_f32: an f16-format output needs the overflow word");
  FGVC_REQUIRE(in_scale_log2 > -100 && in_scale_log2 < 100 && out_scale_log2 > -100 && out_scale_log2 < 100, FGVC_ERR_INVALID_ARG,
               "fgvc_conv64_split_fmt_f32: scale exponent out of range");
  FGVC_REQUIRE(!(residual && residual_split), FGVC_ERR_INVALID_ARG, "fgvc_conv64_split_res_f32: one residual, f32 or split, not both");
  FGVC_REQUIRE(!residual_split || in_fmt == FGVC_ACT_BF16X2, FGVC_ERR_UNSUPPORTED,
               "fgvc_conv64_split_fmt_f32: a split residual is read as (hi, lo) bf16: bf16x2 tensors only");
  FGVC_REQUIRE(N >= 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "fgvc_conv64_split_f32: bad shape");
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG, "fgvc_conv64_split_f32: padded size %dx%d too small for %dx%d", Hp, Wp, H, W);
  FGVC_REQUIRE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(residual) && aligned16(residual_split) && aligned16(y_split) &&
                   aligned16(y_f32),
               FGVC_ERR_INVALID_ARG, "fgvc_conv64_split_f32: 16-byte alignment required");
  FGVC_REQUIRE((const void*)x != (const void*)y_split && (!residual_split || (const void*)residual_split != (const void*)y_split),
               FGVC_ERR_INVALID_ARG, "fgvc_conv64_split_f32: in-place not supported");
  if (N == 0) return FGVC_OK;
  return conv64_launch(x, w, bias, residual, residual_split, y_split, y_f32, N, H, W, Hp, Wp, relu, in_fmt, in_scale_log2, out_fmt,
                       out_scale_log2, overflow, (hipStream_t)stream);
}

int fgvc_conv_s2_split_f32(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N,
                           int H, int W, int Hp, int Wp, int Cin, int Cout, int KS, int Hop, int Wop, int relu, void* stream) {
  return fgvc_conv_s2_split_fmt_f32(x, w, bias, y_split, y_f32, N, H, W, Hp, Wp, Cin, Cout, KS, Hop, Wop, relu, FGVC_ACT_BF16X2, 0, nullptr, stream);
}

int fgvc_conv_s2_split_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N,
                               int H, int W, int Hp, int Wp, int Cin, int Cout, int KS, int Hop, int Wop, int relu, int out_fmt,
                               int out_scale_log2, int* overflow, void* stream) {
  return fgvc_conv_s2_split_proj_fmt_f32(x, w, bias, y_split, y_f32, nullptr, nullptr, nullptr, N, H, W, Hp, Wp, Cin, Cout, KS, Cout, Hop, Wop,
                                         relu, 0, out_fmt, out_scale_log2, overflow, stream);
}

int fgvc_conv_s2_split_proj_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32,
                                    const uint16_t* w2, const float* bias2, float* y2_f32, int N, int H, int W, int Hp, int Wp, int Cin,
                                    int Cout, int KS, int Cout2, int Hop, int Wop, int relu, int relu2, int out_fmt, int out_scale_log2,
                                    int* overflow, void* stream) {
  FGVC_REQUIRE(x && w && bias && (y_split || y_f32), FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_f32: null pointer");
  FGVC_REQUIRE(out_fmt >= 0 && out_fmt <= 3 && out_scale_log2 > -100 && out_scale_log2 < 100, FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_fmt_f32: bad output format / scale");
  FGVC_REQUIRE(out_fmt == FGVC_ACT_BF16X2 || !y_split || overflow, FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_fmt_f32: an f16-format output needs the overflow word");
  FGVC_REQUIRE(N >= 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_f32: bad shape");
  FGVC_REQUIRE(KS == 1 || KS == 3, FGVC_ERR_UNSUPPORTED, "fgvc_conv_s2_split_f32: kernel size %d (1 or 3, stride 2)", KS);
  FGVC_REQUIRE(Cin > 0 && Cin % 32 == 0 && Cout > 0 && Cout % 32 == 0, FGVC_ERR_UNSUPPORTED,
               "fgvc_conv_s2_split_f32: Cin=%d and Cout=%d must be multiples of 32", Cin, Cout);
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;     // both forms: floor((H + 2 pad - KS) / 2) + 1 with pad = KS / 2
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_f32: padded size %dx%d too small for %dx%d", Hp, Wp, H, W);
  FGVC_REQUIRE(!y_split || conv_pad_ok(Ho, Wo, Hop, Wop), FGVC_ERR_INVALID_ARG,
               "fgvc_conv_s2_split_f32: padded output size %dx%d too small for %dx%d", Hop, Wop, Ho, Wo);
  FGVC_REQUIRE(aligned16(x) && aligned16(w) && aligned16(bias) && aligned16(y_split) && aligned16(y_f32),
               FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_f32: 16-byte alignment required");
  FGVC_REQUIRE((const void*)x != (const void*)y_split, FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_f32: in-place not supported");
  if (w2 || bias2 || y2_f32) {                                // the projection in the same launch: all three or none
    FGVC_REQUIRE(w2 && bias2 && y2_f32, FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_proj_fmt_f32: null pointer (w2, bias2 and y2_f32 go together)");
    FGVC_REQUIRE(KS == 3, FGVC_ERR_UNSUPPORTED, "fgvc_conv_s2_split_proj_fmt_f32: the projection rides in the 3x3 kernel only (KS = %d)", KS);
    FGVC_REQUIRE(Cout2 == Cout, FGVC_ERR_UNSUPPORTED, "fgvc_conv_s2_split_proj_fmt_f32: the projection's Cout=%d differs from the convolution's %d", Cout2, Cout);
    FGVC_REQUIRE(aligned16(w2) && aligned16(bias2) && aligned16(y2_f32), FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_proj_fmt_f32: 16-byte alignment required");
    FGVC_REQUIRE((const void*)y2_f32 != (const void*)y_f32, FGVC_ERR_INVALID_ARG, "fgvc_conv_s2_split_proj_fmt_f32: the two f32 outputs must differ");
  }
  if (N == 0) return FGVC_OK;
  return conv_s2_launch(x, w, bias, y_split, y_f32, N, Hp, Wp, Cin, Cout, KS, Ho, Wo, Hop, Wop, relu, out_fmt, out_scale_log2, overflow,
                        w2, bias2, y2_f32, relu2, (hipStream_t)stream);
}

int fgvc_stem7_split_f32(const float* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N, int H,
                         int W, int Hop, int Wop, int relu, void* stream) {
  return fgvc_stem7_split_fmt_f32(x, w, bias, y_split, y_f32, N, H, W, Hop, Wop, relu, FGVC_ACT_BF16X2, 0, nullptr, stream);
}

int fgvc_stem7_split_fmt_f32(const float* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N, int H,
                             int W, int Hop, int Wop, int relu, int out_fmt, int out_scale_log2, int* overflow, void* stream) {
  FGVC_REQUIRE(x && w && bias && (y_split || y_f32), FGVC_ERR_INVALID_ARG, "fgvc_stem7_split_f32: null pointer");
  FGVC_REQUIRE(out_fmt == FGVC_ACT_BF16X2 || out_fmt == FGVC_ACT_F16F8, FGVC_ERR_UNSUPPORTED, "fgvc_stem7_split_fmt_f32: output format %d", out_fmt);
  FGVC_REQUIRE(out_fmt == FGVC_ACT_BF16X2 || !y_split || overflow, FGVC_ERR_INVALID_ARG,
               "fgvc_stem7_split_fmt_f32: an f16-format output needs the overflow word");
  FGVC_REQUIRE(out_scale_log2 > -100 && out_scale_log2 < 100, FGVC_ERR_INVALID_ARG, "fgvc_stem7_split_fmt_f32: scale exponent out of range");
  FGVC_REQUIRE(N >= 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "fgvc_stem7_split_f32: bad shape");
  const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;     // floor((H + 6 - 7) / 2) + 1
  FGVC_REQUIRE(!y_split || conv_pad_ok(Ho, Wo, Hop, Wop), FGVC_ERR_INVALID_ARG,
               "fgvc_stem7_split_f32: padded output size %dx%d too small for %dx%d", Hop, Wop, Ho, Wo);
  FGVC_REQUIRE(aligned16(w) && aligned16(bias) && aligned16(y_split) && aligned16(y_f32) && ((uintptr_t)x & 3) == 0,
               FGVC_ERR_INVALID_ARG, "fgvc_stem7_split_f32: alignment (16 bytes; 4 for x)");
  if (N == 0) return FGVC_OK;
  return stem7_launch(x, w, bias, y_split, y_f32, N, H, W, Ho, Wo, Hop, Wop, relu, out_fmt, out_scale_log2, overflow, (hipStream_t)stream);
}

int fgvc_nhwc_to_split_f32(float* x, uint16_t* out, int N, int C, int H, int W, int Hp, int Wp, int relu, void* stream) {
  FGVC_REQUIRE(x && out, FGVC_ERR_INVALID_ARG, "fgvc_nhwc_to_split_f32: null pointer");
  FGVC_REQUIRE(N >= 0 && C > 0 && C % 32 == 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG,
               "fgvc_nhwc_to_split_f32: bad shape (C must be a multiple of 32)");
  FGVC_REQUIRE(conv_pad_ok(H, W, Hp, Wp), FGVC_ERR_INVALID_ARG, "fgvc_nhwc_to_split_f32: padded size %dx%d too small for %dx%d", Hp, Wp, H, W);
  FGVC_REQUIRE(aligned16(x) && aligned16(out), FGVC_ERR_INVALID_ARG, "fgvc_nhwc_to_split_f32: 16-byte alignment required");
  FGVC_REQUIRE((long long)N * H * W * C / 4 < (1ll << 31) * 256, FGVC_ERR_UNSUPPORTED, "fgvc_nhwc_to_split_f32: tensor too large");
  if (N == 0) return FGVC_OK;
  return nhwc_to_split_launch(x, out, N, C, H, W, Hp, Wp, relu, (hipStream_t)stream);
}

static int normalize_split_common(const char* what, const float* in, float* out_f32, uint16_t* out_split, int N, int C, int H, int W,
                                  int normalize, int fmt, void* stream) {
  FGVC_REQUIRE(in && (out_f32 || out_split), FGVC_ERR_INVALID_ARG, "%s: null pointer", what);
  FGVC_REQUIRE(N >= 0 && C > 0 && C % 4 == 0 && H > 0 && W > 0, FGVC_ERR_INVALID_ARG, "%s: bad shape", what);
  FGVC_REQUIRE(aligned16(in) && aligned16(out_f32) && aligned16(out_split), FGVC_ERR_INVALID_ARG, "%s: 16-byte alignment required", what);
  if (N == 0) return FGVC_OK;
  return normalize_nhwc_launch(in, out_f32, out_split, N, C, H, W, normalize, fmt, (hipStream_t)stream);
}

int fgvc_normalize_split_nhwc_f32(const float* in, float* out_f32, uint16_t* out_split, int N, int C, int H, int W, int normalize,
                                  void* stream) {
  return normalize_split_common("fgvc_normalize_split_nhwc_f32", in, out_f32, out_split, N, C, H, W, normalize, 0, stream);
}

int fgvc_normalize_split_f16x2_nhwc_f32(const float* in, float* out_f32, uint16_t* out_split, int N, int C, int H, int W,
                                        int normalize, void* stream) {
  return normalize_split_common("fgvc_normalize_split_f16x2_nhwc_f32", in, out_f32, out_split, N, C, H, W, normalize, 1, stream);
}

int fgvc_normalize_split_f16f6p_nhwc_f32(const float* in, uint8_t* rows, int N, int C, int H, int W, int normalize, void* stream) {
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_normalize_split_f16f6p_nhwc_f32: C=%d unsupported (256 only)", C);
  return normalize_split_common("fgvc_normalize_split_f16f6p_nhwc_f32", in, nullptr, reinterpret_cast<uint16_t*>(rows), N, C, H, W, normalize, 2, stream);
}

int fgvc_normalize_split_f16f6x_nhwc_f32(const float* in, uint8_t* rows, int N, int C, int H, int W, int normalize, void* stream) {
  FGVC_REQUIRE(C == 256, FGVC_ERR_UNSUPPORTED, "fgvc_normalize_split_f16f6x_nhwc_f32: C=%d unsupported (256 only)", C);
  return normalize_split_common("fgvc_normalize_split_f16f6x_nhwc_f32", in, nullptr, reinterpret_cast<uint16_t*>(rows), N, C, H, W, normalize, 3, stream);
}

int fgvc_normalize_nhwc_f32(const float* in, float* out, int N, int C, int H, int W, int normalize, void* stream) {
  FGVC_REQUIRE(in && out, FGVC_ERR_INVALID_ARG, "fgvc_normalize_nhwc_f32: null pointer");
  return fgvc_normalize_split_nhwc_f32(in, out, nullptr, N, C, H, W, normalize, stream);
}

int fgvc_gaussian_labels_f32(const float* points, int P, int Hf, int Wf, int stride, float sigma, float* out,
                             void* stream) {
  FGVC_REQUIRE(points && out, FGVC_ERR_INVALID_ARG, "fgvc_gaussian_labels_f32: null pointer");
  FGVC_REQUIRE(P > 0 && Hf > 0 && Wf > 0 && stride >= 1 && sigma > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_gaussian_labels_f32: bad shape");
  return gaussian_launch(points, P, Hf, Wf, stride, sigma, out, (hipStream_t)stream);
}

size_t fgvc_softargmax_workspace_bytes(int n_frames, int P) {
  if (n_frames < 0 || P < 0) return 0;
  return (size_t)n_frames * P * (softargmax_bands() * (2 * 5 + 1) + 1) * sizeof(float);
}

int fgvc_softargmax_top5_f32(const float* labels, int n_frames, int Hf, int Wf, int P, int h, int w,
                             const float* gauss_points, float sigma, double* coords, void* workspace, void* stream) {
  FGVC_REQUIRE(labels && coords, FGVC_ERR_INVALID_ARG, "fgvc_softargmax_top5_f32: null pointer");
  FGVC_REQUIRE(n_frames >= 0 && Hf > 0 && Wf > 0 && P > 0 && h > 0 && w > 0, FGVC_ERR_INVALID_ARG, "fgvc_softargmax_top5_f32: bad shape");
  FGVC_REQUIRE((long long)h * w < (1ll << 31) && h * w >= 5, FGVC_ERR_UNSUPPORTED, "fgvc_softargmax_top5_f32: h*w out of range");
  FGVC_REQUIRE(n_frames <= 65535 && sigma > 0.f, FGVC_ERR_INVALID_ARG, "fgvc_softargmax_top5_f32: bad n_frames/sigma");
  FGVC_REQUIRE(workspace != nullptr || n_frames == 0, FGVC_ERR_INVALID_ARG,
               "fgvc_softargmax_top5_f32: workspace of fgvc_softargmax_workspace_bytes() bytes required");
  FGVC_REQUIRE(P <= 65535, FGVC_ERR_UNSUPPORTED, "fgvc_softargmax_top5_f32: P > 65535");
  if (n_frames == 0) return FGVC_OK;
  return softargmax_launch(labels, n_frames, Hf, Wf, P, h, w, gauss_points, sigma, coords,
                           static_cast<float*>(workspace), (hipStream_t)stream);
}

}  // extern "C"
