/*
 * fgvc_hip.h -- C ABI of libfgvc_hip.so: FGVC's label-propagation inference hot path
 * as hand-written HIP kernels for MI355X (gfx950 / CDNA4).
 *
 * The reference (qianduoduolr/FGVC, "mmpt") is pure Python; its FFI for this path is
 * "call these torch functions".  Each entry point below replaces the body of one reference
 * function (cited as file:line relative to the reference tree); fgvc_amd/mmpt_api/ rebuilds the
 * reference's Python signatures on top of them and INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host"; buffers are caller-owned
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is
 *     enqueued asynchronously on it; nothing here allocates, frees or synchronises
 *     (the functions are hipGraph-capturable)
 *   - return value: FGVC_OK or an FGVC_ERR_* code; fgvc_last_error() gives the text
 *     (thread-local).  No exceptions cross the ABI.
 *   - feature maps are CHANNELS-LAST ("hwc"): feat[frame][pixel][channel], pixel = y*W + x
 *   - label maps are PIXEL-MAJOR ("hwp"):     lab[frame][pixel][label]
 *   - top-k lists are in canonical order: score descending, index ascending among equals
 *     (torch.topk leaves tie order unspecified; see DESIGN.md "tie policy")
 */
#ifndef FGVC_HIP_H
#define FGVC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FGVC_OK 0
#define FGVC_ERR_INVALID_ARG 1
#define FGVC_ERR_UNSUPPORTED 2
#define FGVC_ERR_LAUNCH 3

/* mask predicate on the integer offset (dy,dx) = key pixel - query pixel
 *   keep  <=>  dy*dy+dx*dx <= r2max  &&  |dy| <= ry  &&  |dx| <= rx
 * circle (affinity_utils.py:98-109, local_attention.py:463-467): r2max = largest d2 with
 *   sqrtf(d2) < radius (fgvc_r2max_for_radius), ry = rx = FGVC_NO_LIMIT
 * square (affinity_utils.py:86-96): r2max = FGVC_NO_LIMIT, ry = nr_h/2, rx = nr_w/2
 * none: all three FGVC_NO_LIMIT */
#define FGVC_NO_LIMIT 0x3fffffff

/* pairs[i] = {query_frame, key_frame, flags, reserved} */
#define FGVC_PAIR_MASKED 1      /* apply the mask predicate to this pair (else full frame)   */

/* weight modes of fgvc_merge_topk_f32 (local_attention.py:368-373) */
#define FGVC_WEIGHT_SOFTMAX 0
#define FGVC_WEIGHT_COSINE 1
#define FGVC_WEIGHT_RAW 2     /* fgvc_dense_attend_f32 only: the affinity itself is the weight, no normalisation (local_square_attention, topk=None) */

const char* fgvc_version(void);
const char* fgvc_last_error(void);

/* Process-wide tuning knobs (host only, not thread-safe against concurrent launches).
 *   "conv_cot_cap"       fgvc_conv_split_f32: at most this many output channels per workgroup (0 = widest, 64, 128).
 *   "conv_narrow"        fgvc_conv_split_f32: 4-row tiles with two workgroups per CU for the 64-channel layers (bit 0, default) /
 *                        the 128-channel 3x3 layers (bit 1).
 *   "readout_prune"      fgvc_softargmax_top5_f32: 1 (default) = pruned read-out, full scan only for the maps it hands back;
 *                        0 = full scan of every map.  Identical results.
 *   "conv64_variant"     fgvc_conv64_split_fmt_f32 (f16 + fp8 operands): 0 (default) = conv64p_kernel, round 5's one-stream-per-tile kernel, for the
 *                        forms the encoder launches; 16 = conv64_kernel<1> (round 3's: the kernel every other form runs on), 32 = the K-split
 *                        experiment, 128 = conv64p_kernel in raster tile order; 8 = s_memtime probe of one workgroup (fgvc_conv64_probe).
 *                        16 and 128 give identical results (A/B switches); the tests hold 0 against 16 bit for bit.
 *   "conv_debug" 1024    fgvc_conv_split_* with f16 + FP6 operands, 3 x 3, 128 / 256-channel tiles: conv_split_kernel (rounds 2-4) instead of
 *                        conv256p_kernel (round 5: one wave per SIMD, main loop one assembly statement).  Identical results (A/B switch).
 *   "pair_f16_debug" 4194304   fgvc_pair_topk_f16f6[x]: pair_topk_kernel_v8 (round 6: one kind of wave, a key block staged once for eight query
 *                        blocks) instead of pair_topk_kernel_v7.  Identical scores, lists equal up to exact score ties across the K-th place.
 *   "pair_debug", "pair_f16_debug", "corr_debug", "corr6_debug", "corr8_debug", "conv_debug", "conv_s2_debug": besides such A/B bits and
 *                        the s_memtime probes these words carry PROFILING ABLATIONS (a kernel without its stores / matrix chain / selection /
 *                        staging): results are WRONG.  libfgvc_hip.so REFUSES them (FGVC_ERR_UNSUPPORTED); libfgvc_hip_ablations.so -- the
 *                        same objects, this one function compiled with -DFGVC_ABLATIONS -- accepts them (fgvc_amd._lib.ablations(),
 *                        FGVC_HIP_LIB; tools/experiments/ablate_*.py, time_*.py). */
int fgvc_set_option(const char* name, int value);

/* Largest integer d2 such that sqrtf((float)d2) < radius, -1 if none (host helper). */
int fgvc_r2max_for_radius(float radius);

/* ---- A5 step 0: F.normalize(dim=1) + NCHW -> channels-last -------------------------------
 * replaces local_attention.py:308-313 (F.normalize(query/key, p=2, dim=1) and the .view()s).
 * in [n][C][HW] f32 (the encoder's NCHW output)  ->  out [n][HW][c_out] f32, c_out >= C,
 * out = in / max(||in||_2 over C, 1e-12) when normalize != 0, plain transpose otherwise;
 * channels C..c_out-1 are written as zeros (zero padding does not change any dot product; it lets
 * callers round C up to a channel count the MFMA kernels support). */
int fgvc_normalize_chw_to_hwc_f32(const float* in, float* out, int n, int C, int HW,
                                  int normalize, int c_out, void* stream);

/* ---- A5 step 1: windowed correlation + running top-k, one (query frame, key frame) pair per
 * grid.y.  Replaces the einsum / masked_fill_ / topk of local_attention.py:321-356 (and the
 * per-chunk mask rebuild of masked_attention_efficient_v2, :452-475) for ONE key frame; the
 * (T*HW x step) slab is never materialised.  f32 MFMA (v_mfma_f32_32x32x2_f32), exact f32.
 *   qfeat [n_qframes][Hq*Wq][C], kfeat [n_kframes][Hk*Wk][C]   (normalised, channels-last)
 *   pairs [n_pairs][4] int32 (device)
 *   idx_out   [n_pairs][Hq*Wq][topk] int32   key pixel index ky*Wk+kx, -1 where fewer than topk
 *                                            candidates exist
 *   score_out [n_pairs][Hq*Wq][topk] f32     raw dot product (NOT yet divided by temperature),
 *                                            descending; -inf where idx = -1
 *   dense_mask: NULL, or an arbitrary [Hk*Wk][Hq*Wq] bool (uint8) mask tensor as accepted by
 *               local_attention.py:329-353; then the analytic predicate must be off (all FGVC_NO_LIMIT)
 *               and FGVC_PAIR_MASKED pairs traverse the full frame consulting the tensor
 * C in {32, 64, 128, 256}; 1 <= topk <= 16.  An analytic mask needs Hq==Hk, Wq==Wk. */
int fgvc_pair_topk_f32(const float* qfeat, const float* kfeat, const int32_t* pairs, int n_pairs,
                       int C, int Hq, int Wq, int Hk, int Wk, int r2max, int ry, int rx, int topk,
                       const uint8_t* dense_mask, int32_t* idx_out, float* score_out, void* stream);

/* Same operator and outputs as fgvc_pair_topk_f32 on the 16-bit matrix pipe, f32-grade (replaces local_attention.py:331-371 like
 * fgvc_pair_topk_f32; the default pair kernel of the engine for C == 256): f16 operands h = f16(2^14 x), l = f16(2^14 x - h) as
 * fgvc_split_f16x2 writes them ([pixel][h C | l C]), three products h h + l h + h l on v_mfma_f32_32x32x16_f16 accumulated in f32
 * (22 significand bits per element; a score differs from the f32 dot product by ~1e-7, the size of f32 summation-order noise);
 * selection runs on fixed-point keys with 24 fractional bits (scores closer than 6e-8 tie and are ordered by pixel index, like
 * equal f32 scores), in waves of their own beside the multiplying ones; key blocks travel through a producer / consumer ring
 * without workgroup barriers.
 *   Precondition: feature rows L2-normalised (|q.k| <= 1), as fgvc_normalize_chw_to_hwc_f32(normalize=1) makes them.
 *   C == 256; 1 <= topk <= 10; analytic mask only (a dense mask tensor needs fgvc_pair_topk_f32).
 *   A query tile walks a list of at most 4096 key blocks (4x8 pixels): the key blocks within the mask's reach for a pair with
 *   FGVC_PAIR_MASKED, the whole key grid for a pair without.  `pairs` lives on the device, so the caller states with
 *   all_masked != 0 that EVERY pair carries FGVC_PAIR_MASKED; then only the reach is checked against the list (a 480x854 grid
 *   with a radius-6 window is fine), otherwise the whole grid must fit (FGVC_ERR_UNSUPPORTED beyond 4096 blocks).  A pair
 *   that breaks the promise on such a grid gets empty lists (-1 / -inf), never truncated ones. */
int fgvc_split_f16x2(const float* feat, uint16_t* h_l /* [n][2][C] f16: h then l */, int64_t n_pixels, int C, void* stream);
int fgvc_pair_topk_f16x3(const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq,
                         int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, int32_t* idx_out,
                         float* score_out, void* stream);
/* ... with the pairs taken in RUNS: runs[n_runs][2] (device, int32) = (first pair, count) of consecutive pairs that share the query
 * frame AND the FGVC_PAIR_MASKED flag (the driver's pair list has them that way: a query frame against its <= 6 key frames,
 * vanilla_tracker.py:353-362); every pair belongs to exactly one run.  A workgroup then sets the query block up once per run and
 * streams the key blocks of its pairs through one ring.  Outputs are indexed by pair as before.  The caller vouches for the runs
 * (they live on the device); list longer runs first (the launch does not reorder). */
int fgvc_pair_topk_f16x3_runs(const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq,
                              int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs, int n_runs,
                              int32_t* idx_out, float* score_out, void* stream);
int fgvc_pair_topk_f16x3_timed_out(void);

/* The same operator (replaces local_attention.py:331-371) in the PRECISION-CONSISTENT arithmetic of the rest of the path -- the
 * encoder computes in f16 + fp8, the dense volume in f16 + FP6: h = f16(256 x), the cross sums h_k l_q + l_k h_q in block-scaled FP6
 * (e2m3, one E8M0 scale per 32 channels) on v_mfma_scale_f32_32x32x64_f8f6f4: 1.5 matrix-pipe units per product where
 * fgvc_pair_topk_f16x3 spends 3, scores within ~6e-5 logit (tau 0.07) of float64 on Gaussian rows (bar: 1e-3), quantised to 2^-20
 * (1.4e-5 logit); indices equal the reference's wherever its scores are further apart than that error.  The engine uses it when the
 * encoder runs f16f8 (whose features are already +-3e-5 logit from the reference's); fgvc_pair_topk_f16x3 remains the 1e-7-grade form.
 *   fgvc_split_f16f6p: feat [n][256] f32 (L2-normalised) -> rows [n][1024] bytes, laid out for the pair kernel's lanes:
 *     [0, 512) h 256 f16 | [512, 640) h6 mains, group v at 32 v + 16 hi | [640, 704) h6 tails (8 B per group and lane half) |
 *     [704, 832) l6 mains | [832, 896) l6 tails | [896, 928) scale bytes, 16 hi + {H v, 4 + L v} | zero.  Group v, lane half hi, element
 *     e = 8 m + i is channel 64 v + 16 m + 8 hi + i (what a lane of the 32 x 32 x 16 f16 shape holds in fragments 4 v .. 4 v + 3);
 *     those 32 channels are one scale block (fgvc_amd/csrc/pair_topk_v7.hpp).  A DIFFERENT layout from fgvc_split_f16f6's.
 *   fgvc_pair_topk_f16f6[_runs]: arguments and outputs of fgvc_pair_topk_f16x3[_runs]; C == 256, topk <= 10, an analytic mask that
 *   every pair carries (all_masked != 0) and that reaches at most 64 key blocks (4 x 8 pixels) per 8 x 16 query tile -- a radius-15
 *   disc reaches 56 -- else FGVC_ERR_UNSUPPORTED.  Same fail-closed protocol; fgvc_pair_topk_f16x3_timed_out() reports for both. */
int fgvc_split_f16f6p(const float* feat, uint8_t* rows, int64_t n_pixels, int C, void* stream);
int fgvc_pair_topk_f16f6(const uint8_t* qsplit, const uint8_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq, int Hk,
                         int Wk, int r2max, int ry, int rx, int topk, int all_masked, int32_t* idx_out, float* score_out, void* stream);
int fgvc_pair_topk_f16f6_runs(const uint8_t* qsplit, const uint8_t* ksplit, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq,
                              int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs, int n_runs,
                              int32_t* idx_out, float* score_out, void* stream);
/* The same rows with the pixel's EXACT channels behind them (round 5: the bank of the default configuration): 2 KiB per pixel =
 * [the 1 KiB row of fgvc_split_f16f6p | 256 f32 = the normalised channels themselves].  fgvc_pair_topk_f16f6x[_runs] = fgvc_pair_topk_f16f6[_runs]
 * on these rows (same arithmetic, same lists, a row stride of 2048 bytes); fgvc_merge_refine_topk_f32 reads the second KiB
 * (row_bytes = 2048, base + 1024) to re-score near-ties exactly.  One tensor, one slice per frame, one message per halo frame. */
int fgvc_split_f16f6x(const float* feat, uint8_t* rows, int64_t n_pixels, int C, void* stream);
int fgvc_pair_topk_f16f6x(const uint8_t* qrows, const uint8_t* krows, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq, int Hk,
                          int Wk, int r2max, int ry, int rx, int topk, int all_masked, int32_t* idx_out, float* score_out, void* stream);
int fgvc_pair_topk_f16f6x_runs(const uint8_t* qrows, const uint8_t* krows, const int32_t* pairs, int n_pairs, int C, int Hq, int Wq,
                               int Hk, int Wk, int r2max, int ry, int rx, int topk, int all_masked, const int32_t* runs, int n_runs,
                               int32_t* idx_out, float* score_out, void* stream);
int fgvc_pair_topk_f16x3_probe(int64_t* out32);   /* debug: s_memtime words of one workgroup (pair_f16_debug = 256) */

/* ---- A5 step 2: merge the per-pair lists of the T key slots of each query frame, divide by the
 * temperature and turn the k logits into weights.  Replaces the global topk over T*HW
 * (local_attention.py:356) and :368-371.
 *   slot_pair [n_out][T] int32 (device): pair id feeding slot t of output frame f, -1 = unused
 *   idx_out [n_out][HWq][topk] = slot*HWk + key pixel   (the reference's flat key index, :312)
 *   logit_out, weight_out [n_out][HWq][topk] f32 */
int fgvc_merge_topk_f32(const int32_t* pair_idx, const float* pair_score, const int32_t* slot_pair,
                        int n_out, int T, int HWq, int HWk, int topk, float temperature,
                        int weight_mode, int32_t* idx_out, float* logit_out, float* weight_out,
                        void* stream);

/* ---- A5 step 2 behind a pair kernel with APPROXIMATE scores (fgvc_pair_topk_f16f6: |score - exact| <= eps): the same merge, made
 * index-exact again.  Replaces the global topk over T*HW (local_attention.py:353-356) like fgvc_merge_topk_f32; the lists it writes are
 * the exact top-k in the exact order wherever the pair kernel's scores are within `eps` (raw dot-product units) of the exact products.
 *   Candidates whose approximate scores lie within 2 eps of a neighbour in the merged order (and can reach the top k) are re-scored
 *   from the EXACT rows -- q_exact / k_exact: 256 f32 per pixel at `base + frame * frame_bytes + pixel * row_bytes` (row_bytes >= 1024:
 *   a plain [frame][pixel][256] f32 bank, or the f32 half of the 2 KiB rows of fgvc_split_f16f6x) -- with products and sums in f64;
 *   a query whose window the pair lists do not close (a slot's own last entry inside it) is recomputed from every candidate under the
 *   mask predicate (r2max / ry / rx as the pair kernel got them; pairs without FGVC_PAIR_MASKED scan the whole frame).
 *   pairs [n_pairs][4] int32 as the pair kernel took them; slot_pair, outputs, weight modes as fgvc_merge_topk_f32; 1 <= topk <= 10 = the
 *   length of the pair lists; C == 256.  Two slots fed by ONE pair (frame 0 twice while idx <= precede_frames,
 *   vanilla_tracker.py:353-362) are exact twins: the lower slot first, as equal scores are ordered everywhere.
 *   workspace: fgvc_merge_refine_workspace_bytes(n_out, HWq) bytes, 16-byte aligned; after the call its first five 32-bit words hold
 *   {queries re-scored, of them recomputed from scratch, candidates re-scored, from-scratch queries beyond the scan queue, the largest
 *   |approximate - exact| score among the re-scored candidates as f32 bits}: the last one is `eps` MEASURED on the call's own data --
 *   a caller that finds it above the eps it passed must not trust the lists (fgvc_amd raises). */
size_t fgvc_merge_refine_workspace_bytes(int n_out, int HWq);
int fgvc_merge_refine_topk_f32(const int32_t* pair_idx, const float* pair_score, const int32_t* slot_pair, const int32_t* pairs,
                               const void* q_exact, int64_t q_frame_bytes, int q_row_bytes, const void* k_exact, int64_t k_frame_bytes,
                               int k_row_bytes, int n_out, int T, int Hq, int Wq, int Hk, int Wk, int C, int topk, float temperature,
                               int weight_mode, float eps, int r2max, int ry, int rx, int32_t* idx_out, float* logit_out,
                               float* weight_out, void* workspace, void* stream);

/* ---- A5 step 3: label propagation  out[i][p] = sum_r weight[i][r] * labels[slot(idx)][pix(idx)][p]
 * replaces the index_select + einsum of local_attention.py:360-375.
 *   labels [n_label_frames][HWk][P]; slot_frame [T] int32 (device): label frame of each key slot
 *   window_L = 0: idx = slot*HWk + pixel.   window_L = L > 0 (A7 local window, vanilla_tracker.py:550-566):
 *   idx = slot*L*L + (dy+R)*L + (dx+R) relative to the query pixel, taps outside the image read 0. */
int fgvc_propagate_topk_f32(const float* labels, const int32_t* slot_frame, int T,
                            const int32_t* idx, const float* weight, int Hq, int Wq, int Hk, int Wk,
                            int P, int topk, int window_L, float* out, void* stream);

/* ---- A5'': dense correlation volume  vol[j][i] = <k_j, q_i> / temperature,  j key, i query
 * replaces affinity_utils.py:6-21 (compute_affinity), local_attention.py:231 / :321-323 and
 * correlation.py:51 for one (query, key) frame pair.  vol is [HWk][HWq] f32, row-major.
 *   _f32    : exact f32 MFMA
 *   _bf16x3 : inputs pre-split by fgvc_split_bf16 into hi+lo bf16, three bf16 MFMA products
 *             (hi*hi + hi*lo + lo*hi), f32 accumulate; |error| <= ~2e-5 in cosine
 *   _bf16   : hi part only (reduced precision, configs[4]) */
int fgvc_corr_volume_f32(const float* qfeat, const float* kfeat, int C, int HWq, int HWk,
                         float temperature, float* vol, void* stream);
int fgvc_split_bf16(const float* feat, uint16_t* hi_lo /* [n][2][C] bf16: hi then lo */, int64_t n_pixels,
                    int C, void* stream);
int fgvc_corr_volume_bf16x3(const uint16_t* q_hi_lo, const uint16_t* k_hi_lo, int C, int HWq, int HWk,
                            float temperature, float* vol, void* stream);
int fgvc_corr_volume_bf16(const uint16_t* q_hi_lo, const uint16_t* k_hi_lo, int C, int HWq, int HWk,
                          float temperature, float* vol, void* stream);

/* The parity-grade volume at two bf16-MFMA times per tile (bf16x3: three): x is stored as h = f16(256 x), h8 = e4m3(h) and
 * l8 = e4m3(256 (256 x - h)); sum h h on v_mfma_f32_32x32x16_f16, the cross sums h8 l8 on the block-scaled fp8 instruction
 * v_mfma_scale_f32_32x32x64_f8f6f4 (twice the K per cycle), l l (2^-22) dropped: every entry within ~1e-4 logit of the f32
 * product on Gaussian features (bound asserted by the tests: 1e-3, the north_star's score bar).  Rows must be L2-normalised
 * (|x| <= 1: 256 x and its residual stay inside the f16 / e4m3 ranges).  C == 256.
 *   fgvc_split_f16f8: feat [n][C] f32 -> out [n][4 C] bytes = [h: C f16 | h8: C bytes | l8: C bytes] per pixel.
 *   fgvc_corr_volume_f16f8: q, k in that format -> vol [HWk][HWq] f32 = <k, q> / temperature.  When HWq * 4 is not a multiple of
 *   128 bytes the launch splits the key rows into classes of equal line phase so that every store still writes whole lines. */
int fgvc_split_f16f8(const float* feat, uint8_t* out, int64_t n_pixels, int C, void* stream);
int fgvc_corr_volume_f16f8(const uint8_t* q_split, const uint8_t* k_split, int C, int HWq, int HWk,
                           float temperature, float* vol, void* stream);

/* The same volume (replaces affinity_utils.py:6-21 `compute_affinity`, local_attention.py:231) at 1.5 bf16-MFMA times per tile: the
 * cross sums in block-scaled FP6 (e2m3, one E8M0 scale per 32 consecutive channels) on v_mfma_scale_f32_16x16x128_f8f6f4, which
 * retires FP6 at four times the f16 rate.  Same accuracy as f16f8 (simulated and measured; asserted bound 1e-3 logit), rows must be
 * L2-normalised, C == 256.
 *   fgvc_split_f16f6: feat [n][256] f32 -> out [n][1024] bytes = [h: 256 f16 | h6: 192 B | l6: 192 B | 16 scale bytes | zero pad]
 *   (exact layout: fgvc_amd/csrc/corr_volume_f6.hip).
 *   fgvc_corr_volume_f16f6: q, k in that format -> vol [HWk][HWq] f32 = <k, q> / temperature. */
int fgvc_split_f16f6(const float* feat, uint8_t* out, int64_t n_pixels, int C, void* stream);
int fgvc_corr_volume_f16f6(const uint8_t* q_split, const uint8_t* k_split, int C, int HWq, int HWk,
                           float temperature, float* vol, void* stream);

/* Measurement helper (no reference counterpart): zeros over `n_floats` floats by a linear sweep of 16-byte stores (plain or non-temporal) --
 * the store ceiling bench.py prices fgvc_corr_volume_f16f6's write stream against; fgvc_set_option("corr6_debug", 1024) replays that
 * kernel's own store sequence without its loads and multiplies (zeros are written). */
int fgvc_debug_store_sweep_f32(float* buf, int64_t n_floats, int nontemporal, void* stream);

/* ---- A5, topk=None branch: weights over EVERY unmasked key instead of the k best
 * replaces local_attention.py:376-383 (`cur_affinity.softmax(dim=1)` / `.clamp(min=0)**2` over the (T*HWk x step) slab and the
 * einsum with value_vec).  Called once per key slot t with that slot's dense volume vol[HWk][HWq] (fgvc_corr_volume_*, already
 * divided by the temperature; -inf entries are skipped) and labels[HWk][P]:
 *   softmax mode: per query an online softmax state {running max, denominator, P weighted label sums} in
 *     state[nsplit][HWq][P+2] f32, `first` != 0 starts it, later calls merge into it;
 *   cosine mode (weight_mode = FGVC_WEIGHT_COSINE): plain sums of max(a,0)^2 * label;
 *   raw mode (FGVC_WEIGHT_RAW): plain sums of a * label over the unmasked keys (reference local_attention.py:38-103 with topk=None).
 * masked != 0 applies the predicate (r2max, ry, rx) on key - query offsets (equal grids required) and visits only the key
 * rows a band of queries can reach.  nsplit = fgvc_dense_attend_splits(HWq, HWk) (host helper) workgroups share a band's key rows.
 * fgvc_dense_attend_finish_f32 merges the splits and normalises: out[HWq][P]. P <= 32. */
int fgvc_dense_attend_splits(int HWq, int HWk);
int fgvc_dense_attend_f32(const float* vol, const float* labels, int Hq, int Wq, int Hk, int Wk, int P, int masked,
                          int r2max, int ry, int rx, int weight_mode, int first, float* state, int nsplit, void* stream);
int fgvc_dense_attend_finish_f32(const float* state, int nsplit, int HWq, int P, int weight_mode, float* out, void* stream);

/* ---- A5'': `propagate` (reference affinity_utils.py:33-50): new_img = img @ affinity for a GIVEN dense affinity aff[HWk][HWq]
 * (e.g. what fgvc_corr_volume_* wrote, softmaxed or not), labels [HWk][P] pixel-major, out [HWq][P], P <= 32 per call:
 *   thr == NULL   out[i][p] = sum_j aff[j][i] * labels[j][p]                                               (:45-49)
 *   thr != NULL   w = max(aff[j][i] - thr[i], 0);  out[i][p] = sum_j w * labels[j][p] / max(sum_j w, 1e-12)  (the `topk` branch, :36-44)
 * One streaming pass over the slab (the kernel of fgvc_dense_attend_f32); state = nsplit * HWq * (P + 2) floats of workspace,
 * nsplit = fgvc_dense_attend_splits(HWq, HWk).
 * fgvc_dense_kth_f32: thr[i] = k-th largest entry of column i of aff (1 <= k <= 64), one more pass; part = workspace of
 * nsplit * HWq * (k <= 16 ? 16 : 64) floats. */
int fgvc_dense_kth_f32(const float* aff, int HWk, int HWq, int k, float* part, int nsplit, float* thr, void* stream);
int fgvc_dense_propagate_f32(const float* aff, const float* labels, int HWk, int HWq, int P, const float* thr, float* state,
                             int nsplit, float* out, void* stream);

/* ---- A7: single-scale local-window correlation + top-k (mmcv.ops.Correlation semantics as used at
 * vanilla_tracker.py:435-443,547-566; torch twin local_attention.py:1190-1240).
 * Same kernel as fgvc_pair_topk_f32 with a square window |dy|,|dx| <= R; additionally the zero-padded
 * taps outside the image are candidates with score exactly 0.
 *   idx_out [HW][topk] = slot*(2R+1)^2 + (dy+R)*(2R+1) + (dx+R);  logit = corr/temperature (divided after
 *   top-k, :563); weight = softmax(logit). */
int fgvc_local_corr_topk_f32(const float* qfeat, const float* kfeat, const int32_t* pairs, int n_slots,
                             int C, int H, int W, int R, int topk, float temperature,
                             int32_t* pair_idx_ws, float* pair_score_ws,
                             int32_t* idx_out, float* logit_out, float* weight_out, void* stream);
/* the same on the f16 matrix pipe: features as written by fgvc_split_f16x2 from L2-NORMALISED rows, C == 256, topk <= 10
 * (fgvc_pair_topk_f16x3 with the square window, then the same merge) -- the default of the HR driver for C == 256 */
int fgvc_local_corr_topk_f16x3(const uint16_t* qsplit, const uint16_t* ksplit, const int32_t* pairs, int n_slots,
                               int C, int H, int W, int R, int topk, float temperature,
                               int32_t* pair_idx_ws, float* pair_score_ws,
                               int32_t* idx_out, float* logit_out, float* weight_out, void* stream);

/* The merge step of fgvc_local_corr_topk_* for every output frame of a planned clip in one launch (HRVanillaTracker's label maps,
 * vanilla_tracker.py:663-830 with masked_attention_efficient_correlation, local_attention.py:883-1006).
 *   pair_idx / pair_score [n_pairs][H*W][topk]: lists of fgvc_pair_topk_{f32,f16x3} with the square window |dy|,|dx| <= R;
 *   slot_pair [n_rows][max_slots] int32 (device): pair feeding key slot j of row r, -1 = no slot (ids outside [0, n_pairs) too).
 *   idx_out / logit_out / weight_out [n_rows][H*W][topk]: idx = j*(2R+1)^2 + (dy+R)*(2R+1) + (dx+R), zero-padded taps added per
 *   slot, logit = score / temperature after the top-k, weight = softmax.  A row equals fgvc_local_corr_topk_* on the same lists bit
 *   for bit; a pair that fills two slot positions gives two candidate sets.  No atomics, no workspace. */
int fgvc_local_merge_plan_f32(const int32_t* pair_idx, const float* pair_score, int n_pairs, const int32_t* slot_pair, int n_rows,
                              int max_slots, int H, int W, int R, int topk, float temperature, int32_t* idx_out, float* logit_out,
                              float* weight_out, void* stream);

/* ---- A7 get_coord (vanilla_tracker.py:445-488): expected image coordinate of every query pixel under the top-k
 * window weights of fgvc_local_corr_topk_f32 with ONE key slot (taps outside the grid contribute (0,0), like the
 * zero-padded F.unfold of the coordinate grid).  idx/weight [H*W][topk] -> out [H*W][2] = (x, y) in image pixels
 * (feature coordinate * scale). */
int fgvc_topk_coord_f32(const int32_t* idx, const float* weight, int H, int W, int R, int topk, int scale,
                        float* out, void* stream);
/* ... for `rows` single-slot lists in one launch: idx / weight [rows][H*W][topk] -> out [rows][H*W][2] = (x, y) interleaved (8-byte
 * aligned: one bilinear tap of fgvc_cycle_chase_f32 is one 8-byte load).  Row r equals fgvc_topk_coord_f32 on its lists bit for bit. */
int fgvc_topk_coord_rows_f32(const int32_t* idx, const float* weight, int rows, int H, int W, int R, int topk, int scale,
                             float* out, void* stream);

/* ---- forward-backward cycle check of predicted tracks: HRVanillaTracker.forward_test_forward's step
 * (vanilla_tracker.py:639: bilinear_sample, align_corners=True, zero padding, corr_lookup.py:31-65) run backwards in time.
 *   fields [n][H*W][2]: fields[j] maps a position (image pixels) in frame s+1+j to frame s+j (fgvc_topk_coord_rows_f32);
 *   traj [n][P][2] = predicted (x, y) of frames s+1 .. s+n, start_xy [P][2] = the query points at frame s.
 * One thread per (i, p): y = traj[i][p]; for j = i .. 0: y = sample(fields[j], y / scale).  back_out [n][P][2] = y,
 * err_out [n][P] = |y - start_xy[p]|.  A non-finite position at any hop, or traj = (-1, -1) (the read-out of an all-zero map), gives
 * back = NaN and err = +inf.  No atomics, no workspace. */
int fgvc_cycle_chase_f32(const float* fields, const float* traj, const float* start_xy, int n, int P, int H, int W, int scale,
                         float* back_out, float* err_out, void* stream);

/* ---- Dense optical flow.
 * Read-out: `rows` single-slot window lists (fgvc_local_merge_plan_f32: idx = tap, negative = empty) -> full-resolution flow, one launch.
 *   idx / weight [rows][H*W][topk] on the H x W feature grid, window radius R; a feature cell sits on padded pixel cell * scale.
 *   Per cell, over its non-empty taps inside the grid (the selection of fgvc_topk_coord_rows_f32): S = sum w, C = sum w (kx, ky) scale;
 *   displacement = C / S - (qx, qy) scale with renorm != 0, C - (qx, qy) scale with renorm == 0 (get_coord's own sum: its zero-padded
 *   taps pull towards the origin); S == 0: displacement 0, the cell is invalid.
 *   Output pixel (x, y) is padded pixel (X, Y) = (x + pad_left, y + pad_top): cells floor(X / scale) and the one after it, both clamped
 *   to W - 1 (rows alike to H - 1), interpolated bilinearly with the fractions (X mod scale) / scale.
 *   flow_out [rows][2][h][w] f32 in pixels, channel 0 = x; valid_out [rows][h][w] uint8 = 1 when all four cells are valid.
 * FGVC_ERR_INVALID_ARG for a null pointer, rows outside 1 .. 65535, a non-positive size, a negative pad, a feature grid of 2^30 cells or more,
 * an output plane of 2^30 pixels or more, h above 1048560.  No atomics, no workspace. */
int fgvc_flow_from_lists_f32(const int32_t* idx, const float* weight, int rows, int H, int W, int R, int topk, int scale, int renorm,
                             int h, int w, int pad_left, int pad_top, float* flow_out, uint8_t* valid_out, void* stream);

/* Forward-backward check of two dense flows, both directions in one launch: the reference's occlusion_estimation
 * (occlusion_estimation.py:95-177) as it runs.  flow_fw / flow_bw [n][2][h][w] f32; occ_fw / occ_bw [n][1][h][w] f32, 1 = consistent.
 *   warped = Warp()(other, own): bilinear, zero padding, align_corners=False on a grid normalised by w - 1 / h - 1, times
 *   (grid_sample(ones) > 0.9999);  sq = sum_c (own_c + warped_c)^2.
 *   FGVC_FLOW_CONSISTENCY: sq < sum_c (own_c * 2 + warped_c^2) * 0.01 + 0.5;   FGVC_FLOW_FB_ABS: sqrt(sq) < diff.
 * f32 arithmetic without contraction.  FGVC_ERR_INVALID_ARG for a null pointer, n outside 1 .. 65535, a non-positive size, a plane of 2^30
 * pixels or more, an unknown mode.  No atomics, no workspace. */
#define FGVC_FLOW_CONSISTENCY 0
#define FGVC_FLOW_FB_ABS 1
int fgvc_flow_consistency_f32(const float* flow_fw, const float* flow_bw, int n, int h, int w, int mode, float diff, float* occ_fw,
                              float* occ_bw, void* stream);

/* The reference's Warp.forward (warp.py:55-82) with mode='bilinear', padding_mode='zeros': feat [N][C][H][W], flow [N][2][H][W] ->
 * out [N][C][H][W] = grid_sample(feat, grid) * mask, grid = (pixel + flow) * 2 / max(size - 1, 1) - 1, mask = (grid_sample(ones, grid) >
 * 0.9999) with use_mask != 0, else 1.  Same limits as the check above. */
int fgvc_warp_f32(const float* feat, const float* flow, int N, int C, int H, int W, int align_corners, int use_mask, float* out,
                  void* stream);

/* ---- Point tracks in both time directions by chaining the dense flow: the reference's TAP-Vid flow-chaining
 * baseline (RAFT.forward_test, raft.py:247-289, on bilinear_sample2d, samp.py:5-99), whole clip, every point, both directions, one launch.
 *   flow_fw / flow_bw [T-1][2][h][w] f32, channel 0 = x: flow_fw[g] takes frame g to g + 1, flow_bw[g] frame g + 1 to g (null with T = 1);
 *   query [P][3] f32 = (t, x, y); ok_fw / ok_bw [T-1][h][w] uint8, read by FGVC_CHAIN_CONSISTENCY only.
 * Per point: traj[tq] = (x, y) as given; for t = tq + 1 .. T - 1: c = c + S(flow_fw[t - 1], c); from the query point again, for
 * t = tq - 1 .. 0: c = c + S(flow_bw[t], c).  S = bilinear_sample2d in f32 without contraction: x0f = floorf(x), x1f = x0f + 1 (y alike);
 * taps at clamp(x0, 0, w - 1), clamp(x0 + 1, 0, w - 1) (y alike); weights (x1f-x)(y1f-y), (x-x0f)(y1f-y), (x1f-x)(y-y0f), (x-x0f)(y-y0f);
 * value ((w00 i00 + w01 i01) + w10 i10) + w11 i11, every product rounded.
 *   FGVC_CHAIN_FRAME (raft.py:285-288): vis = x >= 0 && y >= 0 && x < w && y < h, per frame.
 *   FGVC_CHAIN_CONSISTENCY: a hop is good when its source position is inside the frame and ok[clamp(floorf(y + 0.5f))][clamp(floorf(x + 0.5f))]
 *   of that hop's field is non-zero; a frame is visible when it is inside the frame and every hop between the query frame and it was good.
 * Fail closed: a position that is non-finite or has |x| or |y| >= 2^23 is never turned into an index -- that frame and every later one on
 * that side are NaN with vis = 0 (the query frame keeps the query as given); a query time that is no integer of [0, T) makes every frame of
 * its point NaN with vis = 0.
 *   traj_out [T][P][2] f32 (8-byte aligned), vis_out [T][P] uint8.  P = 0: nothing is launched.
 * FGVC_ERR_INVALID_ARG for T outside 1 .. 65536, a negative P, a non-positive size, a plane of 2^30 pixels or more, an unknown visibility,
 * a null pointer that is read, a misaligned traj_out.  No atomics, no workspace. */
#define FGVC_CHAIN_FRAME 0
#define FGVC_CHAIN_CONSISTENCY 1
int fgvc_flow_chain_f32(const float* flow_fw, const float* flow_bw, const uint8_t* ok_fw, const uint8_t* ok_bw, const float* query, int T,
                        int P, int h, int w, int visibility, float* traj_out, uint8_t* vis_out, void* stream);

/* ---- The input stage: decoded uint8 RGB frames -> the network's planar f32 input, one launch.  Per frame exactly
 * what datasets.preprocess_tapvid_frames defines (configs/eval/base_data.py:1-7: Resize, RGB2LAB, Normalize): bilinear resize (h0, w0) ->
 * (h, w) on the 0..255 values (align_corners=False, no antialiasing, edge clamped; the identity at the same size), / 255 and clamp to
 * [0, 1], sRGB -> linear -> XYZ -> CIE Lab (D65, OpenCV's documented constants; parity with cv2 itself unpinned), (x - [50, 0, 0]) /
 * [50, 127, 127].  Source coordinates and bilinear weights are computed in double and rounded once; the rest is f32.
 *   frames: T frames of h0 x w0 x 3 bytes addressed by four BYTE strides (frame, row, column, channel): channels-last (T, h0, w0, 3),
 *           planar (T, 3, h0, w0) and non-contiguous crops of either are read in place.
 *   out [T][3][pad_top + h + pad_bottom][pad_left + w + pad_right] f32, contiguous: the frame at (pad_top, pad_left), the border written
 *           as exact 0.0f by the same launch (F.pad of the normalised frames, pad_divide_by: common/utils.py:397-410).
 * At the same size the sRGB transfer is read from a 256-entry table built per workgroup by the function the resize path evaluates.
 * FGVC_ERR_INVALID_ARG for a null pointer, a non-positive size or a negative pad, and for a shape beyond the launch grid: T > 65535,
 * more than 262140 padded rows (four per workgroup on a 16-bit grid axis), a padded width of 2^30 or more, a padded plane of 2^31 pixels
 * or more -- all before any launch.  No workspace, no atomics. */
int fgvc_frames_rgb8_to_lab_f32(const uint8_t* frames, int T, int h0, int w0, int64_t stride_t, int64_t stride_y, int64_t stride_x,
                                int64_t stride_c, int h, int w, int pad_left, int pad_right, int pad_top, int pad_bottom, float* out,
                                void* stream);

/* ---- The input stage for 8-bit YUV 4:2:0 video: what decoders hand out (NV12, I420; NV21 / YV12 with u and v
 * swapped) -> the network's planar f32 input, or packed RGB bytes, one launch each.  Per frame what datasets.preprocess_yuv420_frames and
 * datasets.yuv420_to_rgb8 define.
 *   y [T][h0][w0] bytes by two BYTE strides (frame, row; columns adjacent); u, v [T][ch][cw] bytes, ch = (h0 + 1) / 2, cw = (w0 + 1) / 2, by
 *           three strides (frame, row, pixel), the same for both: pixel stride 1 for I420's planes, 2 for NV12's pairs (v = u + 1).
 *   Chroma at luma pixel (x, y): bilinear and edge clamped at sx = x / 2 (FGVC_YUV_SITING_LEFT: MPEG-2, H.264, HEVC) or x / 2 - 0.25
 *           (FGVC_YUV_SITING_CENTER: JPEG, MPEG-1), sy = y / 2 - 0.25 for both; exact in f32 (quarter weights, byte samples).
 *   Decode, every f32 operation rounded and none fused: yy = cy (Y - y_off), cb = U' - 128, cr = V' - 128, R = yy + crv cr,
 *           G = (yy + cgu cb) + cgv cr, B = yy + cbu cb -- on the 0..255 scale, neither clamped nor rounded.  The six coefficients come by
 *           value (ops.yuv_coefficients computes them in double from the matrix and the range and rounds once).
 *   ..._to_lab_f32: then exactly fgvc_frames_rgb8_to_lab_f32's steps in its arithmetic (resize of the unclamped R'G'B' with double
 *           coordinates, / 255 and clamp, sRGB -> Lab, normalise, zero border); out as there.  The sRGB transfer is evaluated per value.
 *   ..._to_rgb8: rint (half to even) of clamp(R'G'B', 0, 255); out [T][h0][w0][3] bytes, contiguous.
 * FGVC_ERR_INVALID_ARG for a null pointer, a non-positive size, a negative pad, a siting other than the two, and a shape beyond the launch
 * grid (as fgvc_frames_rgb8_to_lab_f32; source sides below 2^30) -- all before any launch.  No workspace, no atomics, no LDS.  These two
 * entries launch the fixed-format instances of csrc/input_yuv.hip's kernels (nothing of the format is an argument). */
#define FGVC_YUV_SITING_LEFT 0
#define FGVC_YUV_SITING_CENTER 1
int fgvc_frames_yuv420_to_lab_f32(const uint8_t* y, const uint8_t* u, const uint8_t* v, int T, int h0, int w0, int64_t y_stride_t,
                                  int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, float y_off, float cy,
                                  float crv, float cgu, float cgv, float cbu, int siting, int h, int w, int pad_left, int pad_right,
                                  int pad_top, int pad_bottom, float* out, void* stream);
int fgvc_frames_yuv420_to_rgb8(const uint8_t* y, const uint8_t* u, const uint8_t* v, int T, int h0, int w0, int64_t y_stride_t,
                               int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, float y_off, float cy, float crv,
                               float cgu, float cgv, float cbu, int siting, uint8_t* out, void* stream);

/* ---- The input stage for planar and semi-planar Y'CbCr at 8 to 16 bits, 4:2:0 / 4:2:2 / 4:4:4: the two entries above
 * generalised.  Per frame what datasets.preprocess_yuv_frames and datasets.yuv_to_rgb8 define.
 *   sample_bytes 1 | 2: the planes hold uint8_t or (host-endian) uint16_t words; EVERY stride is in samples.  A sample is
 *           (word >> shift) & (2^depth - 1), depth 8..16, shift 0..(8 sample_bytes - depth): P010 is depth 10, shift 6 (its low six bits are
 *           ignored), yuv420p10le depth 10, shift 0 (bits above the depth are masked off).
 *   sub_x, sub_y 1 | 2: chroma planes u, v [T][ch][cw], ch = ceil(h0 / sub_y), cw = ceil(w0 / sub_x), by (frame, row, pixel) strides as above.
 *           A subsampled axis is interpolated as above (vertically between the rows, horizontally by `siting`); a full-resolution axis takes
 *           the sample at the luma index, unchanged (`siting` is not used where sub_x = 1).
 *   Decode: yy = cy (Y - y_off), cb = U' - c_off, cr = V' - c_off, then as above: the seven coefficients come by value
 *           (ops.yuv_coefficients_depth).  At depth 8 with sub_x = sub_y = 2 the outputs equal the 8-bit entries' bit for bit -- from the
 *           run-time-format instances of the same kernels (csrc/input_yuv.hip): the entry chooses the instance, the values never do.
 * FGVC_ERR_INVALID_ARG as above, and for sample_bytes other than 1 or 2, a depth outside 8..16, depth + shift beyond the sample's bits, a
 * negative shift, sub_x / sub_y other than 1 or 2, a 16-bit plane at an odd address -- all before any launch.  No workspace, no atomics, no
 * LDS. */
int fgvc_frames_yuvp_to_lab_f32(const void* y, const void* u, const void* v, int sample_bytes, int depth, int shift, int sub_x, int sub_y, int T,
                                int h0, int w0, int64_t y_stride_t, int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y,
                                int64_t c_stride_x, float y_off, float cy, float c_off, float crv, float cgu, float cgv, float cbu, int siting,
                                int h, int w, int pad_left, int pad_right, int pad_top, int pad_bottom, float* out, void* stream);
int fgvc_frames_yuvp_to_rgb8(const void* y, const void* u, const void* v, int sample_bytes, int depth, int shift, int sub_x, int sub_y, int T,
                             int h0, int w0, int64_t y_stride_t, int64_t y_stride_y, int64_t c_stride_t, int64_t c_stride_y,
                             int64_t c_stride_x, float y_off, float cy, float c_off, float crv, float cgu, float cgv, float cbu, int siting,
                             uint8_t* out, void* stream);

/* ---- The output stage for 8-bit YUV 4:2:0 video, the mirror image of fgvc_frames_yuv420_to_rgb8: RGB bytes -> Y'CbCr
 * planes in one launch for all T frames; per frame what datasets.rgb8_to_yuv420 defines, byte for byte.
 *   frames [T][h0][w0][3] bytes by four BYTE strides (frame, row, pixel, channel): packed pixels are (.., .., 3, 1), planar frames
 *           (.., w0, 1, h0 w0); a time slice or a cropped window is read in place.
 *   y [T][h0][w0] by two strides (frame, row; columns adjacent); u, v [T][ch][cw], ch = (h0 + 1) / 2, cw = (w0 + 1) / 2, by three strides
 *           (frame, row, pixel), the same for both: pixel stride 1 for I420's planes, 2 for NV12's pairs (v = u + 1; NV21: u = v + 1).
 *   Every f32 operation rounded, none fused, all values on the 0..255 scale; lum(R, G, B) = (kr R + kg G) + kb B:
 *           Y = y_off + sy lum(R, G, B) at every pixel;
 *           chroma sample (j, i) from the R, G, B bytes filtered first (exact: eighths on bytes) over the rows 2 j and min(2 j + 1, h0 - 1) --
 *           FGVC_YUV_SITING_CENTER: columns 2 i and min(2 i + 1, w0 - 1), the four added and x 0.25; FGVC_YUV_SITING_LEFT: columns
 *           max(2 i - 1, 0), 2 i, min(2 i + 1, w0 - 1) with weights 1, 2, 1, the two rows added and x 0.125 --
 *           L = lum(Rm, Gm, Bm), U = 128 + cu (Bm - L), V = 128 + cv (Rm - L);
 *           each byte rint (half to even) of the value clamped to [0, 255].
 *           The seven coefficients come by value (ops.rgb_to_yuv_coefficients computes them in double and rounds once).
 * The outputs must not overlap the frames or each other.  With T = 0 nothing is launched.  FGVC_ERR_INVALID_ARG for a null pointer, T < 0, a
 * non-positive size, a siting other than the two, output rows, samples or frames that overlap by their strides, and a shape beyond the launch
 * grid (T <= 65535, rows <= 65535 fgvc_yuv_out_tile_rows(), columns < 2^30) -- all before any launch.  No workspace, no atomics, no LDS.  The
 * two tile functions give the luma rows and columns one workgroup owns (tests place shapes one past them). */
int fgvc_frames_rgb8_to_yuv420(const uint8_t* frames, int T, int h0, int w0, int64_t stride_t, int64_t stride_y, int64_t stride_x,
                               int64_t stride_c, uint8_t* y, int64_t y_stride_t, int64_t y_stride_y, uint8_t* u, uint8_t* v,
                               int64_t c_stride_t, int64_t c_stride_y, int64_t c_stride_x, float kr, float kg, float kb, float y_off, float sy,
                               float cu, float cv, int siting, void* stream);
int fgvc_yuv_out_tile_rows(void);
int fgvc_yuv_out_tile_cols(void);

/* ---- DAVIS J&F on the device: the integer pixel counts that metrics.db_eval_iou and metrics.f_measure divide.
 *   gt, pred [T][h][w] uint8 object ids, 0 = background.  For object o = 1 .. n_objects: G = (gt == o), S = (pred == o); an id above
 *           n_objects belongs to no object (metrics.davis_masks_to_objects).
 *   counts [T][n_objects][6] int64: |G & S|, |G | S|, |b(S)|, |b(G)|, |b(S) & dil(b(G))|, |b(G) & dil(b(S))|.
 * b(.) is metrics._seg2bmap: a pixel is a boundary pixel when it differs from its east, south or south-east neighbour, neighbours outside
 * the image counting as 0; then the last row compares east only, the last column south only, and the bottom-right corner is never one.
 * dil(B)(p) holds when some q INSIDE the image has B(q) and |p - q|^2 <= radius^2 (scipy's binary_dilation with metrics._disk and a zero
 * border; nothing wraps across a row's end).  Every element of `counts` is written by the call (it clears them on `stream`, then adds
 * integers: deterministic).  1 <= radius <= 64, 0 <= n_objects <= 255; with T = 0 or n_objects = 0 nothing is launched.
 * FGVC_ERR_UNSUPPORTED for a radius above 64; FGVC_ERR_INVALID_ARG for a null pointer, a negative size, radius < 1, n_objects outside
 * 0 .. 255 and a frame of 2^31 pixels or more.  fgvc_jf_tile_rows(): the rows one workgroup owns (tests put mask edges on its multiples). */
int fgvc_jf_counts_u8(const uint8_t* gt, const uint8_t* pred, int T, int h, int w, int n_objects, int radius, int64_t* counts, void* stream);
int fgvc_jf_tile_rows(void);

/* ---- Objects as boxes: per frame and id, the object's area, box, coordinate sums and border count, all T frames in
 * one launch; metrics.object_stats_host word for word.
 *   ids   [T][h][w] uint8 through its own frame and row strides in bytes (pixels are packed: a time slice or a window is read in place).
 *   stats [T][n_ids][8] int64.  For frame t and id o = 0 .. n_ids - 1 (the background, id 0, has its row like any other), over the pixels
 *         with ids[t][y][x] == o:  0 area,  1 x0 = min x,  2 y0 = min y,  3 x1 = max x + 1,  4 y1 = max y + 1,  5 sum of x,  6 sum of y,
 *         7 border = the number of those pixels with x == 0, x == w - 1, y == 0 or y == h - 1.  An id with no pixel on a frame: eight
 *         zeros.  A pixel whose id is n_ids or more is counted nowhere.
 * Every element of `stats` is written by one plain store (nothing to clear, no global atomic, no workspace): integer sums, minima and
 * maxima, the same in any order.  Runs on `stream`; the entry neither allocates nor synchronises.  FGVC_ERR_INVALID_ARG, with a message
 * naming the argument, for a null ids or stats, n_ids outside 1 .. 256, T, h or w below 1, h w max(h, w) of 2^62 or more, a row stride below w
 * or a negative frame stride -- all before any launch. */
int fgvc_seg_object_stats_u8(const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y, int T, int h, int w, int n_ids, int64_t* stats,
                             void* stream);

/* ---- Connected components of id maps: labels, and the cleaning rule on top of them (drop small components or all but
 * the largest of an id, then fill holes); metrics.components_host and metrics.clean_masks_host word for word.
 *   ids    [T][h][w] uint8 through its own frame and row strides in bytes (pixels are packed).
 *   labels [T][h][w] int32, contiguous.  Two pixels of a frame belong together when they carry one id and are neighbours: 4- or 8-neighbours
 *          (`connectivity`) for a non-zero id, always 4-neighbours for id 0.  A pixel's label is the smallest index y * w + x of its
 *          component; with background == 0 the pixels of id 0 get -1.  Three launches (tile, seam, flatten); no workspace.
 * fgvc_seg_clean_u8: out = fill(drop(ids)) per frame.  Drop: a component of an id 1 .. n_ids - 1 becomes 0 when its area is below min_area,
 * and with keep_largest also when it is not the largest of its id on the frame (equal areas: the smaller root wins); ids >= n_ids are copied
 * and take part in nothing.  Fill (fill_holes, on the map after the drop): a 4-connected component of id 0 with no pixel on the frame's outermost
 * rows and columns, whose 4-neighbours that are not background all carry one id o < n_ids, and of at most max_hole_area pixels (negative: any
 * area), becomes o.  frame_flags [T] uint8 or null: a frame whose flag is 0 is copied and its stats are zero.
 *   out    [T][h][w] uint8 through its own strides; may be ids itself (same strides), must not overlap it otherwise.
 *   stats  [T][n_ids][4] int64: components of the id before the drop, components kept, pixels dropped, pixels filled with the id.
 *   workspace: at least fgvc_seg_clean_workspace_bytes(T, h, w, n_ids) bytes of device memory, 8-byte aligned, owned by the caller.  The kernels
 *          write every word of it they later read: nothing has to be cleared, and what it held before cannot matter.
 * Every element of out, stats and labels is written.  Four launches, five with keep_largest, four more with fill_holes, all on `stream`; the
 * entries neither allocate nor synchronise, and no kernel waits for another workgroup.  All atomics are integer: the outputs do not depend on
 * the order of arrival.  FGVC_ERR_INVALID_ARG, with a message naming the argument, for a null pointer, n_ids outside 1 .. 256, T, h or w below 1,
 * a frame of 2^31 pixels or more, a connectivity other than 4 or 8, a row stride below w, a negative frame stride, overlapping frames of out,
 * other strides for an in-place out, a negative min_area, a flag that is neither 0 nor 1, a workspace that is misaligned or too small;
 * FGVC_ERR_UNSUPPORTED for 2^31 tiles or more -- all before any launch.  The two tile functions give the rows and columns one workgroup labels
 * in LDS (tests put components on their multiples). */
int fgvc_seg_components_i32(const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y, int T, int h, int w, int connectivity, int background,
                            int32_t* labels, void* stream);
int fgvc_seg_clean_u8(const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y, int T, int h, int w, int n_ids, int connectivity, int min_area,
                      int keep_largest, int fill_holes, int64_t max_hole_area, const uint8_t* frame_flags, uint8_t* out, int64_t out_stride_t,
                      int64_t out_stride_y, int64_t* stats, void* workspace, size_t workspace_bytes, void* stream);
size_t fgvc_seg_clean_workspace_bytes(int T, int h, int w, int n_ids);
int fgvc_seg_ccl_tile_rows(void);
int fgvc_seg_ccl_tile_cols(void);

/* ---- Object crops: windows that follow each object, and their anti-aliased resampling onto a fixed size.
 * fgvc_seg_object_windows_i64: metrics.object_windows_host word for word, one launch.
 *   stats   [T][n_ids][8] int64 as fgvc_seg_object_stats_u8 writes them;  objects [M] int32 on the device, the ids to follow (an id outside
 *           0 .. n_ids - 1 gets eight zeros);  windows [T][M][8] int64, every word written.
 *   All arithmetic is int64; fdiv is floor and cdiv ceiling division, both right for negative numerators.  For frame t and id o:
 *   U = {u : |u - t| <= smooth, 0 <= u < T, area[u][o] > 0}; area[t][o] == 0: eight zeros.  Otherwise n = |U|, Wm = max_U (x1 - x0),
 *   Wp = max(min_side, Wm + 2 cdiv(Wm pad_q, 1024)), Hm and Hp likewise; if Wp size_h < Hp size_w then Wp = cdiv(Hp size_w, size_h) else
 *   Hp = cdiv(Wp size_h, size_w); wx0 = fdiv(sum_U (x0 + x1) - n Wp, 2 n), wx1 = wx0 + Wp, y likewise; never clamped to the frame.
 *   Words 0 .. 3: (wx0, wy0, wx1, wy1) in mask pixels; words 4 .. 7: (fdiv(wx0 frame_w, mask_w), fdiv(wy0 frame_h, mask_h),
 *   cdiv(wx1 frame_w, mask_w), cdiv(wy1 frame_h, mask_h)) in frame pixels.
 *   FGVC_ERR_INVALID_ARG, naming the argument, for size outside 1 .. 1024, pad_q outside 0 .. 4096, min_side outside 1 .. 32768, smooth
 *   outside 0 .. 2^20 - 1, a mask or frame side outside 1 .. 32768, a null pointer -- all before the launch.
 * fgvc_frames_object_crops_u8: viz.crop_windows_host byte for byte, two launches (plan, resample).
 *   frames  [T][H][W][3] uint8 RGB through its own frame, row, pixel and channel strides in bytes (a view is read in place).
 *   windows [T][M][window_words] int64, window_words 8 (as above: words 4 .. 7 are resampled, words 0 .. 3 sample the ids) or 4
 *           ((x0, y0, x1, y1), both spaces equal).
 *   crops   [T][M][size_h][size_w][3] uint8;  masks [T][M][size_h][size_w] uint8 or null (then ids is null too).
 *   Per axis with window [a0, a1) and n outputs, in float64, every operation rounded, none contracted, left to right: scale = (a1 - a0) / n,
 *   fs = max(scale, 1), inv = 1 / fs; for output j: center = a0 + (j + 0.5) scale, lo = floor(center - fs + 0.5), hi = floor(center + fs
 *   + 0.5); taps i = lo .. hi - 1 in increasing order: a = |(i - center + 0.5) inv|, v_i = a < 1 ? 1 - a : 0, ww = the sum of the v_i in
 *   that order, k_i = v_i / ww (ww != 0), K_i = int(0.5 + k_i 2^22).  Horizontal pass, then vertical, with a uint8 intermediate:
 *   tmp = clip8((2^21 + sum_i K_i src_i) >> 22), out = clip8((2^21 + sum_i K_i tmp_i) >> 22); src outside the frame is the fill byte of
 *   its channel; lo and hi are not clipped to the frame.  Masks: mx = wx0 + fdiv((2 xx + 1) (wx1 - wx0), 2 size_w), my likewise, in mask
 *   space; 255 where (my, mx) is inside the map and ids[t][my][mx] == objects[j], else 0.
 *   A window is resampled when x1 > x0, y1 > y0, every coordinate is below 2^30 in magnitude and, per axis,
 *   2 ceil(max(a1 - a0, n) / n) + 2 <= max_taps (4 .. 256); any other window gives a crop of the fill colour and a mask of zeros.
 *   workspace: at least fgvc_frames_object_crops_workspace_bytes(T, M, size_h, size_w, max_taps) bytes of device memory, 4-byte aligned,
 *   owned by the caller: the coefficient table.  The plan pass writes every word the resample pass reads; nothing has to be cleared.
 *   Every byte of crops and masks has one writer; no atomics; both launches on `stream`; the entry neither allocates nor synchronises.
 *   FGVC_ERR_INVALID_ARG, naming the argument, for H or W outside 1 .. 32768, window_words other than 4 or 8, size outside 1 .. 1024,
 *   max_taps outside 4 .. 256, a fill that is no byte, ids without masks or masks without ids, a null or misaligned pointer, an ids row
 *   stride below mask_w, a workspace that is too small -- all before any launch. */
int fgvc_seg_object_windows_i64(const int64_t* stats, int T, int n_ids, const int32_t* objects, int M, int size_h, int size_w, int pad_q,
                                int min_side, int smooth, int mask_h, int mask_w, int frame_h, int frame_w, int64_t* windows, void* stream);
size_t fgvc_frames_object_crops_workspace_bytes(int T, int M, int size_h, int size_w, int max_taps);
int fgvc_frames_object_crops_u8(const uint8_t* frames, int T, int H, int W, int64_t frames_stride_t, int64_t frames_stride_y,
                                int64_t frames_stride_x, int64_t frames_stride_c, const int64_t* windows, int window_words, int M, int size_h,
                                int size_w, int fill_r, int fill_g, int fill_b, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                                int mask_h, int mask_w, const int32_t* objects, int max_taps, uint8_t* crops, uint8_t* masks, void* workspace,
                                size_t workspace_bytes, void* stream);

/* ---- Render: mask overlay and point icons onto uint8 RGB video, all T frames in one launch; fgvc_amd/viz.py's host
 * backend bit for bit.
 *   frames, out [T][h][w][3] uint8, each through its own frame and row strides in bytes (pixels are packed: 3 bytes); `out` may be `frames`
 *           itself (same strides) -- a pixel depends on its own input pixel and on ids only -- and must not overlap it otherwise.
 *   ids     [T][h][w] uint8 through its own frame and row strides, or null (no overlay).  k = ids[t][y][x] > 0:
 *           out_c = (frame_c (256 - alpha) + palette[k][c] alpha + 128) >> 8, alpha 0 .. 256, palette [256][3] uint8; with contour != 0 a
 *           pixel whose left, right, upper or lower in-image neighbour has another id takes palette[k][c] unblended.  k == 0: unchanged.
 *   tracks  float64, (x, y) of point i on frame t at tracks[i * tracks_stride_p + t * tracks_stride_t + {0, 1}] (strides in doubles), or
 *           null / P == 0 (no points); visibles uint8 at [i * visibles_stride_p + t * visibles_stride_t], non-zero = drawn, null = all;
 *           colors [P][3] uint8; icon [(2 r + 1)^2] float64, the dot's opacity (viz.icon_table: computed once on the host).
 *           After the overlay every visible point with finite coordinates is blended in INDEX ORDER onto the pixels its window covers:
 *           x = track_x + 0.5 clamped to [0, w], x1 = floor(x), x2 = x1 + 1 (y alike); a = py + r + 1 - y1, b = px + r + 1 - x1 in
 *           [0, 2 r + 1]; with I = icon, zero outside,
 *             patch = I(a,b)(x2-x)(y2-y) + I(a-1,b)(x2-x)(y-y1) + I(a,b-1)(x-x1)(y2-y) + I(a-1,b-1)(x-x1)(y-y1)
 *             v_c = (1 - patch) v_c + patch colors[i][c], truncated towards zero to uint8 after every point
 *           in float64 without contraction, products and sums left to right (the reference's paint_point_track, gathered per pixel).
 * Neither ids nor tracks: a copy.  No workspace, no atomics; runs on `stream`.  FGVC_ERR_UNSUPPORTED for a radius above 31;
 * FGVC_ERR_INVALID_ARG for a null pointer, a negative size, a frame of 2^29 pixels or more, alpha outside 0 .. 256, radius < 1, row strides
 * below a row's bytes, overlapping rows or frames of `out`, tracks or icon not 8-byte aligned -- all before any launch.  With T, h or w = 0
 * nothing is launched.  The two tile functions give the rows and columns one workgroup owns (tests put points and contours on their multiples). */
int fgvc_render_frames_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                          int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                          const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                          int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                          const uint8_t* colors, int P, int radius, const double* icon, void* stream);
int fgvc_render_tile_rows(void);
int fgvc_render_tile_cols(void);

/* ---- Motion trails: the renderer above with every point's last `trail` steps drawn as anti-aliased line segments
 * between the overlay and the dots, still one launch; fgvc_amd/viz.py's host backend bit for bit.  Every argument up to `icon` is the
 * renderer's, except: tracks must not be null when P > 0, and icon == null leaves the dots out (radius is then ignored).
 *   trail   L, 1 .. 64.  On frame t point i has the segments s = max(0, t - L) .. t - 1, drawn oldest first, points in index order;
 *           segment s joins A = tracks[i][s] + 0.5 and B = tracks[i][s + 1] + 0.5 (pixel (px, py) is the point (px, py)) and is drawn only
 *           if both ends are visible and all four track coordinates are below 2^20 in magnitude (NaN and the infinities are not).
 *           Ends are not clamped to the image.
 *   linewidth 1 .. 16; ro2 = ro ro and g = 1 / (ro2 - ri ri) with ro = linewidth / 2 + 0.5, ri = max(linewidth / 2 - 0.5, 0), made once by
 *           the caller (viz.trail_consts) so that both backends use the same two doubles.
 *   fade    [trail] float64 in [0, 1], by age t - 1 - s;  time_colors [T - 1][3] uint8, the colour of segment s, or null: colors[i].
 *           Per pixel, float64 without contraction, products and sums left to right, d = B - A, L2 = dx dx + dy dy:
 *             u = 0 if L2 == 0 else min(max(((px - ax) dx + (py - ay) dy) / L2, 0), 1)
 *             ex = px - (ax + u dx), ey = py - (ay + u dy), cov = min(max((ro2 - (ex ex + ey ey)) g, 0), 1), op = cov fade[t - 1 - s]
 *             v_c = (1 - op) v_c + op colour_c, truncated towards zero to uint8 after every segment; cov <= 0: unchanged.
 * Errors as the renderer's, and FGVC_ERR_INVALID_ARG for trail or linewidth out of range, a null fade table, neither colour table, negative
 * frame strides of tracks or visibles, fade not 8-byte aligned; FGVC_ERR_UNSUPPORTED for P trail >= 2^30.  No workspace, no atomics. */
int fgvc_render_trails_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                          int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                          const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                          int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                          const uint8_t* colors, int P, int radius, const double* icon, int trail, double linewidth, double ro2, double g,
                          const double* fade, const uint8_t* time_colors, void* stream);

/* ---- Pose: the renderer above with the joints' heat maps and the skeleton's limbs drawn between the overlay and the
 * dots -- overlay, heat, limbs, dots -- still one launch; fgvc_amd/viz.py's host backend bit for bit.  Every argument up to `icon` is the
 * renderer's, except: icon == null leaves the dots out (radius and colors are then ignored).
 *   heat    [T][K][h][w] float32 or (heat_f64 != 0) float64, element (t, k, y, x) at heat[t stride_t + k stride_k + y stride_y + x] (strides in
 *           elements), or null: no maps; 1 <= K <= 256; heat_colors [K][3] uint8.  Per pixel, for k = 0 .. K - 1 in order:
 *             a = min(max(v heat_gain, 0), 1) heat_alpha, v widened to double; not a > 0 (zero, negative, NaN): unchanged; else
 *             v_c = (1 - a) v_c + a colour_c, truncated towards zero to uint8 after every map.
 *   skeleton [E][2] int32 joint indices in 0 .. P - 1 (an edge with an index outside is not drawn), limb_colors [E][3] uint8.  On frame t
 *           edge e = (a, b) is the trail's segment from tracks[a][t] + 0.5 to tracks[b][t] + 0.5, drawn in edge order only if both ends are
 *           visible on t and all four coordinates are below 2^20 in magnitude; its opacity is cov limb_alpha.  limb_width 1 .. 16 with
 *           ro2 and g as fgvc_render_trails_u8's linewidth (viz.trail_consts).
 * Errors as the renderer's, and FGVC_ERR_INVALID_ARG for K, heat_gain (finite, > 0), heat_alpha, limb_alpha (0 .. 1) or limb_width out of
 * range, a null colour table, negative strides, a misaligned heat or skeleton.  No workspace, no atomics. */
int fgvc_render_pose_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                        int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                        const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                        int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                        const uint8_t* colors, int P, int radius, const double* icon, const int32_t* skeleton, int E,
                        const uint8_t* limb_colors, double limb_width, double ro2, double g, double limb_alpha, const void* heat, int heat_f64,
                        int K, int64_t heat_stride_t, int64_t heat_stride_k, int64_t heat_stride_y, const uint8_t* heat_colors,
                        double heat_gain, double heat_alpha, void* stream);

/* ---- Boxes and id tags: the renderer above with every object's box drawn between the overlay and the dots -- overlay,
 * boxes, dots -- still one launch; fgvc_amd/viz.py's host backend bit for bit.  Every argument up to `icon` is the renderer's.
 *   boxes   [T][N][4] int32 (x0, y0, x1, y1), half-open, frame t at boxes + t boxes_stride_t (in int32s); 0 <= N <= 255.  On frame t the boxes
 *           are drawn in index order; box i draws nothing when x1 <= x0 or y1 <= y0, when box_visibles[t box_visibles_stride_t + i] == 0
 *           (null: all are drawn), or when a coordinate is 2^20 or more in magnitude.  Otherwise, with bw = box_width (1 .. 16),
 *           a = box_alpha (0 .. 256) and C = box_colors[i] ([N][3] uint8), each step on the pixels inside the frame:
 *   ring    the pixels of [x0 - bw, x1 + bw) x [y0 - bw, y1 + bw) that are not in the box: v_c = (v_c (256 - a) + C_c a + 128) >> 8.
 *   tag     when box_labels ([N] int32 in 0 .. 999; null: no tags) is given: label has d decimal digits, s = label_scale (1 .. 4),
 *           tw = (6 d + 1) s, th = 9 s;  ty = y0 - bw - th, or y0 when that is negative;  tx = x0 - bw, or max(w - tw, 0) when
 *           x0 - bw + tw > w.  The pixels of [tx, tx + tw) x [ty, ty + th) blend as the ring's do.
 *   digits  tag pixel (px, py) is the tag's own pixel u = (px - tx) / s, r = (py - ty) / s (integer division); for 1 <= r <= 7 and u >= 1
 *           with g = (u - 1) / 6, cc = (u - 1) % 6 < 5: where bit 4 - cc of row r - 1 of the glyph (digits [10][7] uint8, one byte a row) of the
 *           label's digit g from the left is set, the pixel becomes white (255) if 299 C_r + 587 C_g + 114 C_b < 128000,
 *           else black (0), opaque.
 * Errors as the renderer's, and FGVC_ERR_INVALID_ARG for N, box_width, box_alpha or label_scale out of range, null boxes or box_colors with
 * N > 0, labels without the digits table, negative frame strides, misaligned boxes or labels.  No workspace, no atomics. */
int fgvc_render_boxes_u8(const uint8_t* frames, int64_t frames_stride_t, int64_t frames_stride_y, uint8_t* out, int64_t out_stride_t,
                         int64_t out_stride_y, int T, int h, int w, const uint8_t* ids, int64_t ids_stride_t, int64_t ids_stride_y,
                         const uint8_t* palette, int alpha, int contour, const double* tracks, int64_t tracks_stride_p,
                         int64_t tracks_stride_t, const uint8_t* visibles, int64_t visibles_stride_p, int64_t visibles_stride_t,
                         const uint8_t* colors, int P, int radius, const double* icon, const int32_t* boxes, int64_t boxes_stride_t,
                         const uint8_t* box_visibles, int64_t box_visibles_stride_t, const uint8_t* box_colors, int N, int box_width,
                         int box_alpha, const int32_t* box_labels, int label_scale, const uint8_t* digits, void* stream);

/* ---- A6: coarse-to-fine refine (local_attention.py:721-880), fine stage.
 *   coarse_arg [T][HW] int32: per key slot and query, the coarse cell picked by the coarse stage
 *                             (fgvc_pair_topk_f32 with topk=1 on the coarse features)
 *   qfine [sH*sW][Cf], kfine [T][sH*sW][Cf] normalised channels-last, vfine [T][sH*sW][P]
 *   out [HW][P]; idx_out/logit_out [HW][topk] (idx = t*(2Rf+1)^2 + tap) */
int fgvc_c2f_refine_f32(const int32_t* coarse_arg, const float* qfine, const float* kfine,
                        const float* vfine, int T, int H, int W, int scale, int Cf, int P, int Rf,
                        int topk, float temperature, float* out, int32_t* idx_out, float* logit_out,
                        void* stream);
/* ... with the weights of the reference's `mode`: FGVC_WEIGHT_SOFTMAX, or FGVC_WEIGHT_COSINE = clamp(affinity, 0)^2, not normalised
 * (local_attention.py:858-861) */
int fgvc_c2f_refine_mode_f32(const int32_t* coarse_arg, const float* qfine, const float* kfine, const float* vfine, int T,
                             int H, int W, int scale, int Cf, int P, int Rf, int topk, float temperature, int weight_mode,
                             float* out, int32_t* idx_out, float* logit_out, void* stream);

/* ---- A1 glue: inference BatchNorm2d (+ residual) (+ ReLU) fused over an NCHW activation
 * replaces the BN / `out += identity` / ReLU modules around every convolution of the ResNet
 * (resnet.py:54-116, mmcv ConvModule conv->BN->ReLU).  y = (x-mean[c])*rsqrt(var[c]+eps)*gamma[c]+beta[c]
 * [+ residual] [ReLU].  x, residual (nullable), out: [N][C][HW] f32; out may alias x. */
int fgvc_bn_act_f32(const float* x, const float* residual, const float* mean, const float* var,
                    const float* gamma, const float* beta, float eps, int relu, float* out, int N, int C,
                    int HW, void* stream);

/* ---- A1 on the bf16 matrix pipe: the encoder's stride-1 3x3 / 1x1 convolutions (resnet.py:16-116, mmcv ConvModule =
 * conv -> BN(eval) [-> + identity] [-> ReLU]) as an implicit GEMM over activations and weights stored as (hi, lo) bf16
 * pairs; hi*hi + hi*lo + lo*hi accumulate in f32 (error ~1e-7 relative, the size of f32 rounding noise).
 *   "padded split NHWC" activations: x[n][Hp][Wp][C/32][hi 32 ch | lo 32 ch] bf16, image at (1,1) inside a ZERO border
 *       that the caller provides once (the kernels only ever write the H x W interior);
 *       Hp >= 8*ceil(H/8)+2, Wp >= 32*ceil(W/32)+8.
 *   weights w[KS*KS][Cin/32][Cout][hi 32 ci | lo 32 ci] bf16 with BatchNorm folded in (w * gamma / sqrt(var + eps)),
 *       tap = ky*KS + kx; bias[Cout] = beta - mean * gamma / sqrt(var + eps)   (fgvc_amd/ops.py: prepare_conv_split).
 *   residual: NULL or dense NHWC f32 [n][H][W][Cout] (= a channels_last NCHW tensor, what MIOpen reads/writes without a
 *       layout conversion);  outputs (either may be NULL): y_split (padded split NHWC, the next convolution's input)
 *       and y_f32 (dense NHWC f32: residual of the next block / final features).
 * Cin % 32 == 0, Cout % 64 == 0, KS in {1, 3}, stride 1, zero padding KS/2. */
int fgvc_nchw_to_split_nhwc_f32(const float* in /* [N][C][H][W] */, uint16_t* out_split /* or NULL */,
                                float* out_f32 /* dense NHWC f32, or NULL */, int N, int C, int H, int W,
                                int Hp, int Wp, void* stream);
/* dense NHWC f32 x[n][H][W][C] -> padded split NHWC; relu != 0 applies max(x, 0) first and writes it back to x in place
 * (the tail of a MIOpen convolution with folded BatchNorm run on channels_last tensors) */
int fgvc_nhwc_to_split_f32(float* x, uint16_t* out_split, int N, int C, int H, int W, int Hp, int Wp, int relu,
                           void* stream);
int fgvc_conv_split_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual,
                        uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp, int Cin, int Cout,
                        int KS, int relu, void* stream);
/* The same convolution with the operand format spelled out (round 3).  A split activation tensor keeps its shape and its 128 bytes
 * per (pixel, 32-channel chunk) in every format; FGVC_ACT_*:
 *   BF16X2  [hi 32 x bf16 | lo 32 x bf16], x = hi + lo                                      3 bf16 products per f32-grade product
 *   F16F8   [h 32 x f16 | l8 32 x e4m3 | h8 32 x e4m3]: h = f16(s x), l8 = e4m3(8 (s x - h)), h8 = e4m3(h / 128), s a per-tensor
 *           power of two (`*_scale_log2`) that puts the tensor's largest values around 2^8           2 products (f16 + one K-64 fp8 MFMA)
 *   F16X2   [h 32 x f16 | l 32 x f16], l = f16(s x - h)                                     3 f16 products, ~2^-22 per term
 *   F16F6   (round 4) [h 32 x f16 | 4 x 16 B]: the FP6 (e2m3) forms of the residual and of h, 32 elements each under one E8M0 scale:
 *           slot 4 = l6 bytes 0-15, slot 5 = h6 bytes 0-15, slot 6 = [l6 bytes 16-23 | scale byte | 0], slot 7 = the same for h6;
 *           l6 = e2m3(f16(2^11 (s x - h)) / 2^sl) with byte 127 + sl - 11, h6 = e2m3(h / 2^sh) with byte 127 + sh, 2^s the smallest
 *           power of two that keeps the block at or below 7.5; element e = channel e in bits [6 e, 6 e + 6)     1.5 products (f16 + one K-64
 *           FP6 MFMA at twice the fp8 rate).  Weights (ops.prepare_conv_split_f16): h6 in slots 4 / 6, l6 in 5 / 7.
 * `in_fmt` is the format of x AND of w (weights: ops.prepare_conv_split(fmt=...): F16F8 rows are [h | h8 = e4m3(h / 4) | l8 =
 * e4m3(512 l)] with h = f16(s_w w)); in_scale_log2 = log2(s_x s_w); out_fmt / out_scale_log2 describe y_split (what the NEXT
 * layer reads); *overflow (device word, required for an f16-format output) is OR-ed with 1 when |s_out y| exceeds 65504. */
#define FGVC_ACT_BF16X2 0
#define FGVC_ACT_F16F8 1
#define FGVC_ACT_F16X2 2
#define FGVC_ACT_F16F6 3
int fgvc_conv_split_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual,
                            uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp, int Cin, int Cout,
                            int KS, int relu, int in_fmt, int in_scale_log2, int out_fmt, int out_scale_log2, int* overflow,
                            void* stream);
/* A BasicBlock's second convolution with the block's PROJECTION SHORTCUT folded in (round 4; resnet.py:96-106 `identity =
 * self.downsample(x) ... out += identity` for a stride-1 1 x 1 projection): y = conv3x3(x, w) + conv1x1(x2, w2) + bias [+ residual]
 * [ReLU], Cout = 256.  x2 is a second padded split NHWC tensor of the same H x W with Cin2 channels, w2 the [1][Cin2/32][256] rows
 * of the projection (BatchNorm folded; ops.prepare_conv_split*), in the SAME format as x / w and scaled so that s_x2 s_w2 = s_x s_w =
 * 2^in_scale_log2 (both products accumulate in one set of sums: the projection costs Cin2 / 32 extra stages of the 9 Cin / 32, its
 * own launch and the dense f32 copy of the identity disappear); bias = the sum of both folded biases. */
int fgvc_conv_split_proj_fmt_f32(const uint16_t* x, const uint16_t* w, const uint16_t* x2, const uint16_t* w2, const float* bias,
                                 const float* residual, uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp, int Cin,
                                 int Cin2, int relu, int in_fmt, int in_scale_log2, int out_fmt, int out_scale_log2, int* overflow,
                                 void* stream);
/* The trunk's LAST convolution writing the pair kernel's feature bank itself (round 4): fgvc_conv_split_fmt_f32 for Cout = 256, KS = 3 whose
 * epilogue -- + bias [+ residual] [ReLU] -- goes on to L2-normalise every pixel's 256 channels (normalize = 1: F.normalize(dim = C),
 * local_attention.py:312-318) and stores them as rows of fgvc_split_f16f6p: bank [N][H*W][1024 B], byte for byte what
 * fgvc_normalize_split_f16f6p_nhwc_f32 makes of the dense f32 output the plain entry point would have written (same association of
 * the sum of squares, same conversions) -- that output and the normalise pass's read of it never touch memory. */
int fgvc_conv_split_bank_f16f6p_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, void* bank,
                                    int N, int H, int W, int Hp, int Wp, int Cin, int KS, int relu, int in_fmt, int in_scale_log2,
                                    int normalize, void* stream);
/* ... as rows of fgvc_split_f16f6x: bank [N][H*W][2048 B], the normalised f32 channels in the second KiB (what the refining merge reads) */
int fgvc_conv_split_bank_f16f6x_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, void* bank,
                                    int N, int H, int W, int Hp, int Wp, int Cin, int KS, int relu, int in_fmt, int in_scale_log2,
                                    int normalize, void* stream);
/* fgvc_conv_split_f32 for Cin = Cout = 64, 3x3 (ResNet layer 1: the largest activations of the trunk), as persistent
 * workgroups that keep the folded weights in registers instead of re-streaming them per tile.  Same tensors and epilogue;
 * weights in MFMA-operand order:
 *   w[2 output tiles][9 taps][2 chunks][2 k-steps][hi | lo][lane = 32 * (k >> 3 & 1) + cout % 32][k & 7]   (ops.prepare_conv64). */
int fgvc_conv64_split_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual, uint16_t* y_split,
                          float* y_f32, int N, int H, int W, int Hp, int Wp, int relu, void* stream);
/* ... with the residual (resnet.py:96-106 `identity = x ... out += identity`) given EITHER as dense NHWC f32 (`residual`) OR as a padded split NHWC
 * tensor of x's geometry (`residual_split`: the identity is then hi + lo, the value the block's first convolution multiplied;
 * the producer of the identity need not write an f32 copy of it).  At most one of the two. */
/* ... and with the operand formats of fgvc_conv_split_fmt_f32: in_fmt / out_fmt FGVC_ACT_BF16X2 or FGVC_ACT_F16F8 (the f16 + fp8
 * arithmetic of the wide layers: a third fewer matrix passes; weights from ops.prepare_conv64_f16: per (output tile, tap, chunk)
 * 4 KiB = [f16 k-step 0 | f16 k-step 1][64 lanes][16 B] then [64 lanes][h8 16 B | l8 16 B]); in_scale_log2 = log2(s_x s_w);
 * residual_split only with bf16x2 tensors. */
int fgvc_conv64_split_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual,
                              const uint16_t* residual_split, uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp,
                              int relu, int in_fmt, int in_scale_log2, int out_fmt, int out_scale_log2, int* overflow, void* stream);
int fgvc_conv64_probe(int64_t* out32);   /* debug: s_memtime sums of one workgroup (conv64_variant = 8) */
int fgvc_conv64_split_res_f32(const uint16_t* x, const uint16_t* w, const float* bias, const float* residual,
                              const uint16_t* residual_split, uint16_t* y_split, float* y_f32, int N, int H, int W, int Hp, int Wp,
                              int relu, void* stream);
/* The stride-2 members of the same family: the 3x3 / stride 2 / zero padding 1 convolution that opens a down-sampling
 * stage and its 1x1 / stride 2 projection (resnet.py:54-76 conv1 of the first BasicBlock, :288-296 downsample), BatchNorm
 * folded, + bias (+ ReLU).  x: padded split NHWC of the H x W input; outputs for the Ho x Wo = ((H-1)/2+1) x ((W-1)/2+1)
 * result: y_split (padded split NHWC, Hop x Wop) and / or y_f32 (dense NHWC f32); bias as for fgvc_conv_split_f32;
 * weights: the same folded (hi, lo) values in MFMA-operand order, one contiguous KiB per operand:
 *   w[KS*KS][Cin/32][Cout/32][hi k 0-15 | hi k 16-31 | lo k 0-15 | lo k 16-31][lane = 32 * (k >> 3 & 1) + cout % 32][k & 7]
 *   (k = input channel within the 32-channel chunk; fgvc_amd/ops.py: prepare_conv_s2).
 * Cin % 32 == 0, Cout % 32 == 0, KS in {1, 3}. */
int fgvc_conv_s2_split_f32(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N,
                           int H, int W, int Hp, int Wp, int Cin, int Cout, int KS, int Hop, int Wop, int relu,
                           void* stream);
/* ... with y_split in any FGVC_ACT_* format (x and w stay BF16X2: these layers read layer 1's output) */
int fgvc_conv_s2_split_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N,
                               int H, int W, int Hp, int Wp, int Cin, int Cout, int KS, int Hop, int Wop, int relu, int out_fmt,
                               int out_scale_log2, int* overflow, void* stream);
/* ... and the block's 1x1 / stride 2 PROJECTION of the same input in the same launch (KS = 3 only; w2, bias2, y2_f32 all null: exactly
 * fgvc_conv_s2_split_fmt_f32): y2_f32 = conv1x1s2(x, w2) + bias2 [ReLU if relu2], dense NHWC f32 [N][Ho][Wo][Cout], w2 in the KS = 1
 * operand order.  The projection reads the 3x3 kernel's centre tap, which is already staged; both outputs equal the two separate
 * launches bit for bit.  Cout2 != Cout or KS != 3 with a projection: FGVC_ERR_UNSUPPORTED. */
int fgvc_conv_s2_split_proj_fmt_f32(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32,
                                    const uint16_t* w2, const float* bias2, float* y2_f32, int N, int H, int W, int Hp, int Wp, int Cin,
                                    int Cout, int KS, int Cout2, int Hop, int Wop, int relu, int relu2, int out_fmt, int out_scale_log2,
                                    int* overflow, void* stream);
/* The stem: 7x7 / stride 2 / zero padding 3 convolution of 3-channel frames to 64 channels, BatchNorm folded, + bias
 * (+ ReLU) (resnet.py:457-466 with pool_type 'none'), from the f32 NCHW frames x[N][3][H][W] to y_f32 (dense NHWC f32
 * [N][Ho][Wo][64]) and / or y_split (padded split NHWC, Hop x Wop); Ho x Wo = ((H-1)/2+1) x ((W-1)/2+1).
 *   w: folded (hi, lo) bf16 weights in MFMA-operand order, K laid out per kernel row as k = 4 kx + c (c = 3 and kx = 7: zero):
 *      w[7 ky][2 k-steps][2 output tiles][hi | lo][lane = 32 * (k >> 3 & 1) + cout % 32][k & 7]   (ops.prepare_stem7);
 *   bias[64] = beta - mean * gamma / sqrt(var + eps). */
int fgvc_stem7_split_f32(const float* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N, int H,
                         int W, int Hop, int Wop, int relu, void* stream);
/* ... with the split output in the format the first block's kernel reads (FGVC_ACT_BF16X2 or FGVC_ACT_F16F8 at scale 2^out_scale_log2) */
int fgvc_stem7_split_fmt_f32(const float* x, const uint16_t* w, const float* bias, uint16_t* y_split, float* y_f32, int N, int H,
                             int W, int Hop, int Wop, int relu, int out_fmt, int out_scale_log2, int* overflow, void* stream);
/* dense NHWC f32 -> [n][H*W][C] f32, rows L2-normalised if `normalize` (the output layout of
 * fgvc_normalize_chw_to_hwc_f32) */
int fgvc_normalize_nhwc_f32(const float* in, float* out, int N, int C, int H, int W, int normalize, void* stream);
/* the same rows and / or their (hi, lo) bf16 split [n][H*W][hi C | lo C] (= fgvc_split_bf16 of them, what
 * fgvc_corr_volume_bf16x3 reads) in ONE pass over the trunk output; either output may be NULL */
int fgvc_normalize_split_nhwc_f32(const float* in, float* out_f32, uint16_t* out_split, int N, int C, int H, int W,
                                  int normalize, void* stream);
/* the same with the split in the (h, l) f16 form of fgvc_split_f16x2 (what fgvc_pair_topk_f16x3 reads) */
int fgvc_normalize_split_f16x2_nhwc_f32(const float* in, float* out_f32, uint16_t* out_split, int N, int C, int H, int W,
                                        int normalize, void* stream);
/* ... and straight into the rows of fgvc_split_f16f6p (what fgvc_pair_topk_f16f6 reads): rows [N][H*W][1024] bytes, C == 256 */
int fgvc_normalize_split_f16f6p_nhwc_f32(const float* in, uint8_t* rows, int N, int C, int H, int W, int normalize, void* stream);
/* ... and into the 2 KiB rows of fgvc_split_f16f6x (the same 1 KiB + the normalised f32 channels) */
int fgvc_normalize_split_f16f6x_nhwc_f32(const float* in, uint8_t* rows, int N, int C, int H, int W, int normalize, void* stream);

/* ---- A3: initial labels  g = exp(-((x*s-cx)^2+(y*s-cy)^2)/(2 sigma^2)) on the feature grid
 * replaces vanilla_tracker.py:204-221 ([::stride] subsample of the full-resolution Gaussian).
 *   points [P][2] f32 = (x, y);  out [Hf*Wf][P] */
int fgvc_gaussian_labels_f32(const float* points, int P, int Hf, int Wf, int stride, float sigma,
                             float* out, void* stream);

/* ---- A8 + A9: bilinear upsample (align_corners=False) fused with the top-5 soft-argmax read-out
 * replaces vanilla_tracker.py:396-400 and :172-191 (no (T,P,h,w) tensor, no D2H copy, no argsort).
 *   labels [n_frames][Hf*Wf][P];  gauss_points: if non-NULL, frame 0 is read out from the analytic
 *   full-resolution Gaussian of these points instead (vanilla_tracker.py:329,322).
 *   coords [n_frames][P][2] f64 = (x, y); (-1,-1) where the map is all zero.
 *   workspace: caller-owned device scratch of fgvc_softargmax_workspace_bytes(n_frames, P) bytes.
 *   A bilinear sample never exceeds the largest of its four coarse corners, so only the coarse cells whose corner maximum
 *   reaches the 5th largest value found around the coarse maximum are upsampled (exactly the pixels a full scan would
 *   select from); maps with negative labels or too flat for the work lists are scanned in full, in row bands. */
size_t fgvc_softargmax_workspace_bytes(int n_frames, int P);
int fgvc_softargmax_top5_f32(const float* labels, int n_frames, int Hf, int Wf, int P, int h, int w,
                             const float* gauss_points, float sigma, double* coords, void* workspace,
                             void* stream);

/* ---- Segmentation masks (semi-supervised VOS, vanilla_tracker.py:663-830).  The propagation itself is fgvc_propagate_topk_f32
 * with P = C channels; these are the two ends of the path and the hard-propagation step.
 *
 * Frame-0 labels: the padded index map (hp, wp) uint8 is sampled to the feature grid (Hf, Wf) by Pillow's NEAREST rule
 * (pil_nearest_interpolate, common/utils.py:39: the source coordinate is a running double sum of in/out, truncated) and one-hot
 * encoded.  fgvc_seg_max_label_u8 writes max(sampled map) to out[0] (int32; C = 1 + that, as F.one_hot infers it);
 * fgvc_seg_onehot_labels_u8 writes out [Hf*Wf][C] f32 (an id >= C gives a zero row). */
int fgvc_seg_max_label_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, int32_t* out, void* stream);
int fgvc_seg_onehot_labels_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, int C, float* out, void* stream);

/* Hard propagation: out[r] = one_hot(argmax_c in[r][c]) for rows r < rows; the first maximum wins.  `out` may be `in`. */
int fgvc_seg_hard_onehot_f32(const float* in, int rows, int C, float* out, void* stream);

/* Read-out of n frames: labels [n][Hf*Wf][C] f32 -> masks [n][h0][w0] uint8 =
 *   argmax_C normalise( bilinear_{h0,w0}( crop_{top,left,h,w}( bilinear_{hp,wp}(labels) ) ) )       (align_corners=False)
 * evaluated per output pixel from the feature grid (no (C, hp, wp) map); normalise (norm != 0) = per (frame, channel)
 * (x - min) / (max - min + 1e-12) where max > 0, else x, min / max over the whole output frame; the first maximum wins.
 * workspace: caller-owned device scratch of fgvc_seg_readout_workspace_bytes(n, C) bytes.  1 <= C <= 256. */
size_t fgvc_seg_readout_workspace_bytes(int n, int C);
int fgvc_seg_readout_u8(const float* labels, int n, int Hf, int Wf, int C, int hp, int wp, int top, int left, int h, int w, int h0,
                        int w0, int norm, uint8_t* masks, void* workspace, void* stream);

/* Annotations at any frame (test_cfg.refs).  fgvc_seg_label_set_u8: the ids present in the map sampled to (Hf, Wf) by the same Pillow
 * NEAREST rule, as a 256-bit set out[8] (uint32: bit id % 32 of word id / 32); one launch, one workgroup.
 * fgvc_seg_inject_labels_u8: rows [Hf*Wf][C] f32, in place: a cell whose sampled id is in `set` (8 uint32 on the device) becomes
 * one_hot(id, C) (an id >= C: a zero row); every other cell keeps its values.  1 <= C <= 256. */
int fgvc_seg_label_set_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, uint32_t* out, void* stream);
int fgvc_seg_inject_labels_u8(const uint8_t* map, int hp, int wp, int Hf, int Wf, int C, const uint32_t* set, float* rows, void* stream);

/* fgvc_seg_readout_u8 with the confidence of every pixel: masks are fgvc_seg_readout_u8's bytes (one device function computes both);
 * conf [n][h0][w0] uint8 = rint(255 * clamp(best - second, 0, 1)) with best / second the two largest of the values the argmax compares
 * (normalised where norm applies; C == 1 gives 255); stats [n][C][2] int64 = per frame and id the pixel count and the sum of its conf
 * bytes (integer atomics: order-independent; cleared here).  workspace as fgvc_seg_readout_u8's. */
int fgvc_seg_readout_conf_u8(const float* labels, int n, int Hf, int Wf, int C, int hp, int wp, int top, int left, int h, int w, int h0,
                             int w0, int norm, uint8_t* masks, uint8_t* conf, int64_t* stats, void* workspace, void* stream);

/* ---- Soft first-frame labels read out as joint coordinates (the JHMDB / BADJA heat-map form: vanilla_tracker.py:700-716 with a 4-D
 * map, :770-784, img2coord :172-191, :814-818).  The map (K, hm, wm) f32 or f64 lies at (top, left) of its zero padding to (hp, wp)
 * (its own pad_divide_by, :672); the padding is implicit, no padded copy is made.  Propagation is fgvc_propagate_topk_f32 with P = K.
 *
 * Bank row 0 (:706-711): out [Hf*Wf][K] f32 = bilinear(padded map -> (Hf, Wf)) (align_corners=False) computed in the map's dtype,
 * rounded once to f32. */
int fgvc_seg_soft_labels_f32(const float* map, int K, int hm, int wm, int hp, int wp, int top, int left, int Hf, int Wf, float* out,
                             void* stream);
int fgvc_seg_soft_labels_f64(const double* map, int K, int hm, int wm, int hp, int wp, int top, int left, int Hf, int Wf, float* out,
                             void* stream);

/* Coordinates of T frames: coords [2][K][T] f64 (x row, then y row), the reference's img2coord of
 *   frame 0:   bilinear_{h0,w0}(padded map) in the map's dtype, NOT unpadded (:712-716); map0 is f64 if map0_f64, else f32;
 *   frame f>0: bilinear_{h0,w0}(crop_{top,left,hm,wm}(bilinear_{hp,wp}(bank[f]))) in f32 (fgvc_seg_readout_u8's composed taps);
 * bank [T][Hf*Wf][K] f32 (row 0 is not read).  Per map: the top 5 values (descending, the higher flat index first among equals),
 * v / (sum5 + 1e-9) in f64 if f64_arith (np.stack of a float64 frame 0) else in f32, x = sum (idx % w0) * v, y = sum (idx / w0) * v
 * in f64; a map whose sum is 0 gives (-1, -1).  The sum is accumulated in f64, lane-strided per row band and then over a tree and
 * the bands (for non-negative maps: sum == 0 <=> max == 0).  No full-resolution map is built.  workspace: caller-owned device
 * scratch of fgvc_heatmap_coords_workspace_bytes(T, K) bytes; no atomics, nothing to clear.  1 <= K <= 256, 5 <= h0*w0. */
size_t fgvc_heatmap_coords_workspace_bytes(int T, int K);
int fgvc_heatmap_coords_f32(const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm, int wm, int hp,
                            int wp, int top, int left, int h0, int w0, int f64_arith, double* coords, void* workspace, void* stream);

/* fgvc_heatmap_coords_f32 with each map's peak: coords as above, bit for bit, and peak [K][T] f64, the largest value of the field that
 * fgvc_softmap_readout_f32 writes for that map (the first of its top five), widened to f64: frame 0 in the map's dtype, later frames f32. */
int fgvc_heatmap_coords_peak_f32(const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm, int wm, int hp,
                                 int wp, int top, int left, int h0, int w0, int f64_arith, double* coords, double* peak, void* workspace,
                                 void* stream);

/* The maps themselves, frames [f_begin, f_end) of the stack the reference returns without `coords` (:770-784, :800-803), channel-first:
 *   out [f_end - f_begin][K][h0][w0], f32 or (out_f64 != 0) f64;
 *   frame 0:   bilinear_{h0,w0}(padded map) in the map's dtype, NOT unpadded (:712-716);
 *   frame f>0: bilinear_{h0,w0}(crop_{top,left,hm,wm}(bilinear_{hp,wp}(bank[f]))) in f32;
 * every value is the one fgvc_heatmap_coords_f32 evaluates for that pixel, bit for bit (the same device functions).  out_f64: frames
 * >= 1 are the f32 values widened, frame 0 keeps the map's precision (np.stack of a float64 frame 0 with float32 frames, :803);
 * out_f64 == 0 with an f64 map rounds frame 0 once to f32.  bank [T][Hf*Wf][K] f32 (row 0 is not read; may be NULL when f_end <= 1),
 * map0 as above.  A workgroup stages the feature-grid footprint of an 8 x 64 output tile in LDS and writes row-contiguous runs.
 * No workspace, no atomics.  1 <= K <= 256, 0 <= f_begin < f_end <= T. */
int fgvc_softmap_readout_f32(const float* bank, const void* map0, int map0_f64, int T, int Hf, int Wf, int K, int hm, int wm, int hp,
                             int wp, int top, int left, int h0, int w0, int f_begin, int f_end, int out_f64, void* out, void* stream);

/* ---- Edge-aware mask read-out (test_cfg.readout = dict(type='guided'); the float64 statement of the rule is
 * engine.guided_readout_host).  guide [n][3][hp][wp] f32: the padded Lab-normalised frames the encoder read, finite values.  The feature
 * grid must divide the padded frame: hp % Hf == 0 and wp % Wf == 0.
 *
 * fgvc_guide_cells_f32: cells [n][Hf*Wf][3] f32 = the mean of the guide over each cell's (hp / Hf) x (wp / Wf) pixel block. */
int fgvc_guide_cells_f32(const float* guide, int n, int hp, int wp, int Hf, int Wf, float* cells, void* stream);

/* Read-out of n frames: labels [n][Hf*Wf][C] f32 -> masks [n][h0][w0] uint8.  Per output pixel (y, x):
 *   py = clamp((y + 0.5) h / h0 - 0.5, 0, h - 1) + top (px alike), I = the guide sampled bilinearly at (py, px),
 *   fy = (py + 0.5) Hf / hp - 0.5 (fx alike), centre cell (floor(fy + 0.5), floor(fx + 0.5));
 *   over the (2 radius + 1)^2 cells (i, j) around the centre cell that lie inside the grid:
 *     e = ((i - fy)^2 + (j - fx)^2) / (2 sigma_space^2) + |I - cells[i][j]|^2 / (2 sigma_range^2),   w = exp(-(e - min e));
 *   value_c = sum(w L_c) / sum(w), with L_c the labels normalised (norm != 0) per (frame, channel) by (x - min) / (max - min + 1e-12)
 *   where max > 0, min / max taken over the FEATURE GRID (fgvc_seg_readout_u8 takes them over its interpolated map);
 *   id = argmax_c value_c, the first maximum wins.
 * f32 arithmetic; one launch for all frames after the two small pre-passes; no [n][C][h0][w0] map is written.
 * The _conf form adds conf and stats as fgvc_seg_readout_conf_u8 defines them (conf = rint(255 clamp(best - second, 0, 1)), 255 where
 * C == 1; stats [n][C][2] int64 = pixel count and conf sum per id, cleared here).
 * cells: fgvc_guide_cells_f32's output for the same guide.  workspace: fgvc_seg_readout_guided_workspace_bytes(n, C) bytes of device
 * scratch.  1 <= C <= 256, 1 <= radius <= 3, sigmas positive and finite.  An output so much smaller than the frame that one
 * fgvc_guided_tile_rows() x fgvc_guided_tile_cols() tile's footprint of cells does not fit the LDS is refused (FGVC_ERR_UNSUPPORTED). */
size_t fgvc_seg_readout_guided_workspace_bytes(int n, int C);
int fgvc_seg_readout_guided_u8(const float* labels, const float* guide, const float* cells, int n, int Hf, int Wf, int C, int hp, int wp,
                               int top, int left, int h, int w, int h0, int w0, int norm, int radius, double sigma_space,
                               double sigma_range, uint8_t* masks, void* workspace, void* stream);
int fgvc_seg_readout_guided_conf_u8(const float* labels, const float* guide, const float* cells, int n, int Hf, int Wf, int C, int hp,
                                    int wp, int top, int left, int h, int w, int h0, int w0, int norm, int radius, double sigma_space,
                                    double sigma_range, uint8_t* masks, uint8_t* conf, int64_t* stats, void* workspace, void* stream);
/* the main kernel's output tile and the number of label channels it stages at a time (for tests that straddle them) */
int fgvc_guided_channel_chunk(void);
int fgvc_guided_tile_rows(void);
int fgvc_guided_tile_cols(void);

/* Fusing a forward and a backward label sweep between annotated frames (test_cfg.refs fuse='linear'; engine.fuse_refs_host is the rule in
 * float64).  ONE launch for n_items frames.  fw [n_fw][HW][C], bw [n_bw][HW][C] and out [n_out][HW][C] are f32 stacks of row blocks;
 * items [n_items][4] int32 on the device holds per item the frame index into fw, into bw and into out, and the bits of an f32 weight w.
 * Per cell of item i:  a = argmax_C fw[items[i][0]][cell], b = argmax_C bw[items[i][1]][cell] (the first maximum wins);
 *   out[items[i][2]][cell][c] = fma(w, x, fl((fl(1 - w)) * y)) in f32 (1 - w is rounded once per item);
 *   counts[i] (int64, cleared on `stream` by this call) = the number of cells with a != b: integer atomics, the same on every run.
 * out may be fw itself where every item's out index is its fw index (each element is read and written by the same lane); apart from that
 * the output blocks must overlap neither each other nor a block that any item reads.  An item with an index outside its stack writes
 * nothing.  The rows are ASSUMED FINITE (the sweeps produce no other): on a row with a NaN the kernel's arg-maximum keeps the first
 * element it compared, where torch.argmax and the float64 rule take the NaN, so nothing is promised for counts or rows there.
 * With n_items = 0 nothing is launched.  FGVC_ERR_INVALID_ARG for a null pointer, n_items outside 0 .. 65535, an empty stack,
 * HW < 1 or C outside 1 .. 256.  No workspace. */
int fgvc_seg_fuse_rows_f32(const float* fw, const float* bw, float* out, const int32_t* items, int n_items, int n_fw, int n_bw, int n_out,
                           int HW, int C, int64_t* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* FGVC_HIP_H */
