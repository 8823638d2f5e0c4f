"""Tensor-level wrappers over the C ABI (include/fgvc_hip.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every kernel is
libfgvc_hip.so.  Inputs must live on a ROCm device; nothing falls back to torch ops.

Layouts: features channels-last (frames, HW, C); labels pixel-major (frames, HW, P);
top-k lists (…, HW, k) in canonical order (score desc, index asc).
"""
from __future__ import annotations

import ctypes as C
import functools
import math
import struct
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from . import _lib
from ._lib import NO_LIMIT, PAIR_MASKED, WEIGHT_COSINE, WEIGHT_RAW, WEIGHT_SOFTMAX  # noqa: F401


@dataclass(frozen=True)
class MaskSpec:
    """keep <=> dy^2+dx^2 <= r2max and |dy| <= ry and |dx| <= rx   (offset = key - query)."""
    r2max: int = NO_LIMIT
    ry: int = NO_LIMIT
    rx: int = NO_LIMIT

    @property
    def is_none(self) -> bool:
        return self.r2max >= NO_LIMIT and self.ry >= NO_LIMIT and self.rx >= NO_LIMIT

    @staticmethod
    def none() -> "MaskSpec":
        return MaskSpec()

    @staticmethod
    def circle(radius: float) -> "MaskSpec":
        """sqrt(dy^2+dx^2) < radius in float32 (affinity_utils.py:98-109, local_attention.py:463-467)."""
        return MaskSpec(r2max=max(_lib.load().fgvc_r2max_for_radius(float(radius)), 0) if radius > 0 else 0)

    @staticmethod
    def square(neighbor_range) -> "MaskSpec":
        """|dy| <= nr_h//2, |dx| <= nr_w//2 (affinity_utils.py:86-96)."""
        nr = (neighbor_range, neighbor_range) if isinstance(neighbor_range, int) else tuple(neighbor_range)
        return MaskSpec(ry=nr[0] // 2, rx=nr[1] // 2)

    @staticmethod
    def from_neighbor_range(neighbor_range, mode: str = "circle") -> "MaskSpec":
        if neighbor_range is None:
            return MaskSpec.none()
        if mode == "circle":
            return MaskSpec.circle(neighbor_range // 2)
        if mode == "square":
            return MaskSpec.square(neighbor_range)
        raise ValueError(mode)


def set_option(name: str, value: int) -> None:
    """fgvc_set_option: process-wide tuning / ablation knobs (include/fgvc_hip.h lists them), e.g. set_option("readout_prune", 0)."""
    _lib.call("fgvc_set_option", name.encode(), int(value))


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)      # the current stream's handle without building a Stream object


def _stream(t: torch.Tensor):
    """hipStream_t of torch's current stream on t's device.  Called once per launch: the small clips are host-bound (32 launches per
    encoder call at 26 us each), and torch.cuda.current_stream() was a fifth of that."""
    if _raw_stream is not None:
        idx = t.device.index
        return C.c_void_p(_raw_stream(torch.cuda.current_device() if idx is None else idx))
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _chk(t: torch.Tensor, dtype, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.FgvcHipError(f"{name} must be on the GPU (fgvc_amd has no CPU path)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.contiguous()


MFMA_CHANNELS = (32, 64, 128, 256)   # channel counts fgvc_pair_topk_f32 / fgvc_corr_volume_f32 are built for


def padded_channels(c: int) -> int:
    for m in MFMA_CHANNELS:
        if c <= m:
            return m
    raise _lib.FgvcHipError(f"C={c} > {MFMA_CHANNELS[-1]} channels is not supported by the correlation kernels")


def normalize_to_hwc(x: torch.Tensor, normalize: bool = True, pad: bool = False) -> torch.Tensor:
    """(n, C, H, W) or (n, C, HW) f32 NCHW -> (n, HW, C') L2-normalised over C (eps 1e-12).
    pad=True rounds C' up to a kernel-supported channel count with zero channels."""
    x = _chk(x, torch.float32, "x")
    n, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    Co = padded_channels(Cc) if pad else Cc
    out = torch.empty((n, HW, Co), device=x.device, dtype=torch.float32)
    _lib.call("fgvc_normalize_chw_to_hwc_f32", _ptr(x), _ptr(out), n, Cc, HW, int(normalize), Co, _stream(x))
    return out


def make_pairs(pairs, device, masked=True) -> torch.Tensor:
    """[(query_frame, key_frame[, masked])...] -> int32 (n,4) device tensor."""
    rows = []
    for p in pairs:
        m = masked if len(p) < 3 else p[2]
        rows.append((int(p[0]), int(p[1]), PAIR_MASKED if m else 0, 0))
    t = torch.tensor(rows, dtype=torch.int32, device=device).reshape(-1, 4)
    t._fgvc_rows = rows                      # host copy: pair_runs() groups the pairs without a device read-back
    return t


def pair_runs(pairs: torch.Tensor) -> Optional[torch.Tensor]:
    """Runs of consecutive pairs with one query frame and one mask flag, as fgvc_pair_topk_f16x3_runs takes them: int32 (n_runs, 2)
    = (first pair, count) on the pairs' device, longest runs first.  None when the pairs were not built by make_pairs() (no host
    copy to group by).  Cached on the tensor."""
    rows = getattr(pairs, "_fgvc_rows", None)
    if rows is None or len(rows) != pairs.shape[0]:
        return None
    cached = getattr(pairs, "_fgvc_runs", None)
    if cached is None:
        runs, i = [], 0
        while i < len(rows):
            j = i
            while j + 1 < len(rows) and rows[j + 1][0] == rows[i][0] and rows[j + 1][2] == rows[i][2]:
                j += 1
            runs.append((i, j - i + 1))
            i = j + 1
        runs.sort(key=lambda r: -r[1])
        cached = torch.tensor(runs, dtype=torch.int32, device=pairs.device).reshape(-1, 2)
        pairs._fgvc_runs = cached
    return cached


def pair_topk(qfeat: torch.Tensor, kfeat: torch.Tensor, pairs: torch.Tensor, Hq: int, Wq: int, Hk: int, Wk: int,
              mask: MaskSpec, topk: int, validate: bool = True,
              dense_mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Windowed correlation + top-k per (query frame, key frame) pair.
    qfeat (nq, HqWq, C), kfeat (nk, HkWk, C), pairs int32 (n,4).
    Returns idx (n, HqWq, topk) int32 (key pixel, -1 = none), score (n, HqWq, topk) f32 raw dot."""
    qfeat, kfeat = _chk(qfeat, torch.float32, "qfeat"), _chk(kfeat, torch.float32, "kfeat")
    pairs = _chk(pairs, torch.int32, "pairs")
    assert qfeat.shape[1] == Hq * Wq and kfeat.shape[1] == Hk * Wk and qfeat.shape[2] == kfeat.shape[2]
    n = pairs.shape[0]
    if n and validate:
        # host-side operand check before a hand-written kernel indexes with these (costs a sync;
        # callers that built `pairs` on the host from known-good frame numbers pass validate=False)
        lim = pairs[:, :2].amax(0).tolist()
        assert lim[0] < qfeat.shape[0] and lim[1] < kfeat.shape[0] and int(pairs[:, :2].min()) >= 0, "pair out of range"
    if dense_mask is not None:
        dense_mask = _chk(dense_mask.to(torch.bool), torch.bool, "dense_mask")
        assert dense_mask.shape == (Hk * Wk, Hq * Wq) and mask.is_none
    idx = torch.empty((n, Hq * Wq, topk), device=qfeat.device, dtype=torch.int32)
    score = torch.empty((n, Hq * Wq, topk), device=qfeat.device, dtype=torch.float32)
    _lib.call("fgvc_pair_topk_f32", _ptr(qfeat), _ptr(kfeat), _ptr(pairs), n, qfeat.shape[2], Hq, Wq, Hk, Wk,
              mask.r2max, mask.ry, mask.rx, topk, _ptr(dense_mask), _ptr(idx), _ptr(score), _stream(qfeat))
    return idx, score


def pair_topk_split(qsplit: torch.Tensor, ksplit: torch.Tensor, pairs: torch.Tensor, Hq: int, Wq: int, Hk: int,
                    Wk: int, mask: MaskSpec, topk: int, validate: bool = True,
                    all_masked: bool = False, fmt: str = "f16", use_runs: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """pair_topk() on the 16-bit matrix pipe (fgvc_pair_topk_f16x3): qsplit (nq, HqWq, 2, 256), ksplit (nk, HkWk, 2, 256) int16 =
    split_f16x2() of L2-NORMALISED features.  Same outputs as pair_topk().  all_masked=True: the caller built `pairs` with
    PAIR_MASKED on every row (then only the mask's reach, not the whole key grid, must fit the kernel's block list).
    `fmt` names the operand format: "f16" = split_f16x2() rows -> fgvc_pair_topk_f16x3; "f16f6" = split_f16f6p() rows ->
    fgvc_pair_topk_f16f6; "f16f6x" = split_f16f6x() rows (frames, HW, 4, 256) -> fgvc_pair_topk_f16f6x (the same kernel at a row stride
    of 2 KiB).  split_f16x2() and split_f16f6p() rows have ONE shape and dtype: the caller's `fmt` is all that tells them apart."""
    if fmt not in ("f16", "f16f6", "f16f6x"):
        raise ValueError(f"pair_topk_split: fmt={fmt!r} ('f16': split_f16x2 operands, 'f16f6': split_f16f6p operands, 'f16f6x': split_f16f6x operands)")
    if fmt != "f16" and not (all_masked and pair_blocks_reached(mask) <= PAIR_F16F6_MAX_BLOCKS):
        raise ValueError(f"pair_topk_split(fmt={fmt!r}): every pair must be masked (all_masked=True) by an analytic mask that reaches at most "
                         f"{PAIR_F16F6_MAX_BLOCKS} key blocks per query tile; use fmt='f16'")
    sym = {"f16": "fgvc_pair_topk_f16x3", "f16f6": "fgvc_pair_topk_f16f6", "f16f6x": "fgvc_pair_topk_f16f6x"}[fmt]
    qsplit, ksplit = _chk(qsplit, torch.int16, "qsplit"), _chk(ksplit, torch.int16, "ksplit")
    pairs = _chk(pairs, torch.int32, "pairs")
    parts = 4 if fmt == "f16f6x" else 2          # a bank says whether its rows are 2 KiB (f16f6x): a mismatch would be read as garbage, not refused
    assert qsplit.dim() == 4 and ksplit.dim() == 4 and qsplit.shape[2] == parts and ksplit.shape[2] == parts, \
        f"pair_topk_split(fmt={fmt!r}): operands must be (frames, HW, {parts}, 256) int16, got {tuple(qsplit.shape)} / {tuple(ksplit.shape)}"
    assert qsplit.shape[1] == Hq * Wq and ksplit.shape[1] == Hk * Wk and qsplit.shape[3] == ksplit.shape[3]
    n = pairs.shape[0]
    if n and validate:
        lim = pairs[:, :2].amax(0).tolist()
        assert lim[0] < qsplit.shape[0] and lim[1] < ksplit.shape[0] and int(pairs[:, :2].min()) >= 0, "pair out of range"
        assert not all_masked or bool((pairs[:, 2] & PAIR_MASKED).all()), "all_masked=True but a pair is not masked"
    idx = torch.empty((n, Hq * Wq, topk), device=qsplit.device, dtype=torch.int32)
    score = torch.empty((n, Hq * Wq, topk), device=qsplit.device, dtype=torch.float32)
    runs = pair_runs(pairs) if (use_runs and n) else None
    if runs is not None:            # a query frame's pairs in one workgroup (query prologue once, the key-block ring never drains)
        _lib.call(sym + "_runs", _ptr(qsplit), _ptr(ksplit), _ptr(pairs), n, qsplit.shape[3], Hq, Wq, Hk, Wk,
                  mask.r2max, mask.ry, mask.rx, topk, int(all_masked), _ptr(runs), runs.shape[0], _ptr(idx), _ptr(score),
                  _stream(qsplit))
        return idx, score
    _lib.call(sym, _ptr(qsplit), _ptr(ksplit), _ptr(pairs), n,
              qsplit.shape[3], Hq, Wq, Hk, Wk, mask.r2max, mask.ry, mask.rx, topk, int(all_masked), _ptr(idx), _ptr(score),
              _stream(qsplit))
    return idx, score


def pair_f16x3_timed_out() -> bool:
    """True if a wave of an earlier fgvc_pair_topk_f16x3 launch gave up waiting on its key-block ring (a kernel bug: its spins are
    bounded so that it cannot hang the GPU; the workgroup then writes poison lists -- index 0, score +inf, NaN weights after the
    merge -- so the results cannot pass for valid ones).  Read-and-clear; synchronises the device."""
    return _lib.load().fgvc_pair_topk_f16x3_timed_out() != 0


PAIR_LIST_CAP = 4096   # key blocks (4x8 pixels) one query tile may visit in fgvc_pair_topk_f16x3 (csrc/pair_topk_v5.hip)


def pair_blocks_needed(Hk: int, Wk: int, mask: Optional[MaskSpec] = None, all_masked: bool = False) -> int:
    """Key blocks a 8x16-pixel query tile of fgvc_pair_topk_f16x3 may have to list (pair_topk_v5_launch's own check):
    the blocks within the mask's reach when every pair is masked, the whole key grid otherwise."""
    whole = -(-Hk // 4) * -(-Wk // 8)
    if not all_masked or mask is None or mask.is_none:
        return whole
    rr = math.isqrt(mask.r2max) if mask.r2max < NO_LIMIT else NO_LIMIT
    reach_y, reach_x = min(mask.ry, rr, Hk), min(mask.rx, rr, Wk)
    return min(-(-Hk // 4), (7 + 2 * reach_y) // 4 + 2) * min(-(-Wk // 8), (15 + 2 * reach_x) // 8 + 2)


PAIR_F16F6_MAX_BLOCKS = 64   # key blocks one query tile may visit in fgvc_pair_topk_f16f6 (6 bits of a selection key name the block)


def pair_blocks_reached(mask: Optional[MaskSpec]) -> int:
    """Key blocks (4 x 8 pixels) an interior 8 x 16 query tile reaches under `mask` (csrc/pair_topk_v7.hpp: pair_v7_blocks_reached, the
    same arithmetic); a huge number when there is no analytic mask.  Cached per mask; a reach whose bounding box alone holds more than
    4 x 64 blocks is answered without counting (the only question asked of the result is `<= 64`)."""
    if mask is None or mask.is_none:
        return 1 << 30
    return _pair_blocks_reached(int(mask.r2max), int(mask.ry), int(mask.rx))


@functools.lru_cache(maxsize=256)
def _pair_blocks_reached(r2max: int, ry: int, rx: int) -> int:
    mask = MaskSpec(r2max, ry, rx)
    rr = math.isqrt(mask.r2max) if mask.r2max < NO_LIMIT else NO_LIMIT
    reach_y, reach_x = min(mask.ry, rr), min(mask.rx, rr)
    if reach_y > 4096 or reach_x > 4096:
        return 1 << 30
    if (2 * reach_y // 4) * (2 * reach_x // 8) > 4 * PAIR_F16F6_MAX_BLOCKS and mask.r2max >= reach_y * reach_y + reach_x * reach_x:
        return 1 << 30                                  # a rectangle (no disc cutting its corners) far beyond the bound: no loop
    QBH, QBW = 4, 8
    ny, nx = (2 * QBH - 1 + 2 * reach_y) // QBH + 2, (2 * QBW - 1 + 2 * reach_x) // QBW + 2
    TY0, TX0 = (reach_y // QBH + 1) * QBH, (reach_x // QBW + 1) * QBW
    count = 0
    for by in range(ny + reach_y // QBH + 2):
        for bx in range(nx + reach_x // QBW + 2):
            hit = False
            for b in range(4):
                wy0, wx0, ky0, kx0 = TY0 + (b & 1) * QBH, TX0 + (b >> 1) * QBW, by * QBH, bx * QBW
                dy = max(0, ky0 - (wy0 + QBH - 1), wy0 - (ky0 + QBH - 1))
                dx = max(0, kx0 - (wx0 + QBW - 1), wx0 - (kx0 + QBW - 1))
                hit = hit or (dy * dy + dx * dx <= mask.r2max and dy <= mask.ry and dx <= mask.rx)
            count += hit
    return count


def pair_f16f6_ok(C: int, Hk: int, Wk: int, topk: int, normalized: bool, dense_mask=None, mask: Optional[MaskSpec] = None,
                  all_masked: bool = False) -> bool:
    """Whether fgvc_pair_topk_f16f6 applies: what split_path_ok() asks, every pair masked, and a mask reach of at most 64 key blocks."""
    return (split_path_ok(C, Hk, Wk, topk, normalized, dense_mask, mask, all_masked) and all_masked
            and pair_blocks_reached(mask) <= PAIR_F16F6_MAX_BLOCKS)


def split_path_ok(C: int, Hk: int, Wk: int, topk: int, normalized: bool, dense_mask=None, mask: Optional[MaskSpec] = None,
                  all_masked: bool = False) -> bool:
    """Whether fgvc_pair_topk_f16x3 applies: 256 channels, top-k <= 10, analytic mask, L2-normalised rows (its
    fixed-point keys assume |q.k| <= 1) and at most 4096 key blocks per query tile (pair_blocks_needed)."""
    return (normalized and C == 256 and 1 <= topk <= 10 and dense_mask is None
            and pair_blocks_needed(Hk, Wk, mask, all_masked) <= PAIR_LIST_CAP and Hk < 16384 and Wk < 32768)


def pair_topk_auto(qfeat: torch.Tensor, kfeat: torch.Tensor, pairs: torch.Tensor, Hq: int, Wq: int, Hk: int, Wk: int,
                   mask: MaskSpec, topk: int, normalized: bool, precision: str = "auto", validate: bool = True,
                   dense_mask: Optional[torch.Tensor] = None, all_masked: bool = False,
                   split_fmt: str = "f16") -> Tuple[torch.Tensor, torch.Tensor]:
    """pair_topk() with the kernel chosen by `precision`:
      "f32"   fgvc_pair_topk_f32 (f32 MFMA);
      "split" fgvc_pair_topk_f16x3 on split_f16x2() of the features; raises when it does not apply;
      "auto"  "split" where split_path_ok(), else "f32".
    qfeat/kfeat are the f32 channels-last features either way (the split costs one extra pass over them)."""
    if precision not in ("auto", "f32", "split"):
        raise ValueError(f"precision={precision!r}")
    ok = split_path_ok(qfeat.shape[2], Hk, Wk, topk, normalized, dense_mask, mask, all_masked)
    use_split = precision == "split" or (precision == "auto" and ok)
    if not use_split:
        return pair_topk(qfeat, kfeat, pairs, Hq, Wq, Hk, Wk, mask, topk, validate, dense_mask)
    if not ok:
        raise ValueError("the split pair kernels need C == 256, topk <= 10, an analytic mask, normalised features and "
                         f"<= {PAIR_LIST_CAP} key blocks per query tile")
    if split_fmt not in ("f16", "f16f6", "f16f6x"):
        raise ValueError(f"split_fmt={split_fmt!r}")
    if split_fmt != "f16" and not pair_f16f6_ok(qfeat.shape[2], Hk, Wk, topk, normalized, dense_mask, mask, all_masked):
        if precision == "split":
            raise ValueError("fgvc_pair_topk_f16f6 needs every pair masked by an analytic mask within 64 key blocks of a query tile")
        split_fmt = "f16"                         # "auto": the three-product kernel takes what the f16 + FP6 one cannot
    splitter = {"f16": split_f16x2, "f16f6": split_f16f6p, "f16f6x": split_f16f6x}[split_fmt]      # the rows the kernel of `split_fmt` reads
    ks = splitter(kfeat)
    qs = ks if qfeat is kfeat else splitter(qfeat)
    return pair_topk_split(qs, ks, pairs, Hq, Wq, Hk, Wk, mask, topk, validate, all_masked, fmt=split_fmt)


def merge_topk(pair_idx: torch.Tensor, pair_score: torch.Tensor, slot_pair: torch.Tensor, HWk: int, topk: int,
               temperature: float, mode: str = "softmax", validate: bool = True):
    """slot_pair int32 (n_out, T): pair feeding key slot t of output frame f (-1 unused).
    Returns idx (n_out, HWq, k) int32 = slot*HWk + pixel, logit, weight."""
    pair_idx, pair_score = _chk(pair_idx, torch.int32, "pair_idx"), _chk(pair_score, torch.float32, "pair_score")
    slot_pair = _chk(slot_pair, torch.int32, "slot_pair")
    assert pair_idx.shape == pair_score.shape and pair_idx.shape[2] == topk
    n_out, T = slot_pair.shape
    if validate:
        assert int(slot_pair.max()) < pair_idx.shape[0]
    HWq = pair_idx.shape[1]
    wm = {"softmax": WEIGHT_SOFTMAX, "cosine": WEIGHT_COSINE}[mode]
    idx = torch.empty((n_out, HWq, topk), device=pair_idx.device, dtype=torch.int32)
    logit = torch.empty((n_out, HWq, topk), device=pair_idx.device, dtype=torch.float32)
    weight = torch.empty_like(logit)
    _lib.call("fgvc_merge_topk_f32", _ptr(pair_idx), _ptr(pair_score), _ptr(slot_pair), n_out, T, HWq, HWk, topk,
              float(temperature), wm, _ptr(idx), _ptr(logit), _ptr(weight), _stream(pair_idx))
    return idx, logit, weight


def propagate_topk(labels: torch.Tensor, slot_frame: torch.Tensor, idx: torch.Tensor, weight: torch.Tensor,
                   Hq: int, Wq: int, Hk: int, Wk: int, window_L: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels (n_frames, HkWk, P), slot_frame int32 (T,), idx/weight (HqWq, k) -> (HqWq, P)."""
    labels = _chk(labels, torch.float32, "labels")
    slot_frame = _chk(slot_frame, torch.int32, "slot_frame")
    idx, weight = _chk(idx, torch.int32, "idx"), _chk(weight, torch.float32, "weight")
    P, k = labels.shape[2], idx.shape[-1]
    assert labels.shape[1] == Hk * Wk and idx.shape[-2] == Hq * Wq and idx.shape == weight.shape
    if out is None:
        out = torch.empty((Hq * Wq, P), device=labels.device, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.shape == (Hq * Wq, P) and out.dtype == torch.float32
    _lib.call("fgvc_propagate_topk_f32", _ptr(labels), _ptr(slot_frame), slot_frame.numel(), _ptr(idx), _ptr(weight),
              Hq, Wq, Hk, Wk, P, k, window_L, _ptr(out), _stream(labels))
    return out


def split_bf16(feat: torch.Tensor) -> torch.Tensor:
    """(…, C) f32 -> (…, 2, C) int16 holding bf16 bit patterns: hi = bf16(x), lo = bf16(x - hi)."""
    feat = _chk(feat, torch.float32, "feat")
    Cc = feat.shape[-1]
    n = feat.numel() // Cc
    out = torch.empty((*feat.shape[:-1], 2, Cc), device=feat.device, dtype=torch.int16)
    _lib.call("fgvc_split_bf16", _ptr(feat), _ptr(out), n, Cc, _stream(feat))
    return out


def split_f16x2(feat: torch.Tensor) -> torch.Tensor:
    """(…, C) f32 L2-normalised rows -> (…, 2, C) int16 holding f16 bit patterns: h = f16(2^14 x), l = f16(2^14 x - h), the
    operand format of fgvc_pair_topk_f16x3."""
    feat = _chk(feat, torch.float32, "feat")
    Cc = feat.shape[-1]
    n = feat.numel() // Cc
    out = torch.empty((*feat.shape[:-1], 2, Cc), device=feat.device, dtype=torch.int16)
    _lib.call("fgvc_split_f16x2", _ptr(feat), _ptr(out), n, Cc, _stream(feat))
    return out


def split_f16f6p(feat: torch.Tensor) -> torch.Tensor:
    """(…, 256) f32 L2-normalised rows -> (…, 2, 256) int16 = the 1 KiB rows of fgvc_split_f16f6p (h = f16(256 x) + FP6 forms of h
    and of the residual with their block scales, laid out for the lanes of fgvc_pair_topk_f16f6; opaque bytes in the shape and dtype
    of split_f16x2()'s output, so that a feature bank travels and is sliced the same way in either format)."""
    feat = _chk(feat, torch.float32, "feat")
    assert feat.shape[-1] == 256, "fgvc_split_f16f6p: 256 channels"
    n = feat.numel() // 256
    out = torch.empty((*feat.shape[:-1], 2, 256), device=feat.device, dtype=torch.int16)
    _lib.call("fgvc_split_f16f6p", _ptr(feat), _ptr(out), n, 256, _stream(feat))
    return out


def split_f16f6x(feat: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(…, 256) f32 L2-normalised rows -> (…, 4, 256) int16 = 2 KiB per pixel: [the row of split_f16f6p() | the 256 f32 channels
    themselves].  The bank of the default configuration (round 5): fgvc_pair_topk_f16f6x multiplies the first KiB, the refining merge
    (merge_refine_topk) re-scores near-ties exactly from the second; one tensor, sliced and sent like any other bank."""
    feat = _chk(feat, torch.float32, "feat")
    assert feat.shape[-1] == 256, "fgvc_split_f16f6x: 256 channels"
    n = feat.numel() // 256
    if out is None:
        out = torch.empty((*feat.shape[:-1], 4, 256), device=feat.device, dtype=torch.int16)
    else:       # rows of the caller's bank (clip sharding: a halo frame arrives as its f32 channels and is split into its bank rows here)
        assert out.dtype == torch.int16 and tuple(out.shape) == (*feat.shape[:-1], 4, 256) and out.is_contiguous() and out.device == feat.device
    _lib.call("fgvc_split_f16f6x", _ptr(feat), _ptr(out), n, 256, _stream(feat))
    return out


def bank_format(bank: torch.Tensor, declared: str = "f16") -> str:
    """What a feature bank holds, from the tensor itself where it says so: f32 rows (…, C) -> "f32"; int16 (…, 4, 256) -> "f16f6x" (no other
    format has four 512-byte parts); int16 (…, 2, C): `declared` -- split_f16x2() and split_f16f6p() rows are both two 512-byte parts and
    cannot be told apart ("f16" | "f16f6" | "bf16": the caller's word, checked for shape only)."""
    if bank.dtype == torch.float32:
        return "f32"
    if bank.dtype == torch.int16 and bank.dim() >= 3 and bank.shape[-2] == 4 and bank.shape[-1] == 256:
        return "f16f6x"
    if bank.dtype == torch.int16 and bank.dim() >= 3 and bank.shape[-2] == 2:
        if declared == "f16f6x":
            raise ValueError("a (…, 2, C) int16 bank cannot be in the f16f6x format (2 KiB rows: (…, 4, 256))")
        return declared
    raise TypeError(f"not a feature bank: {bank.dtype} {tuple(bank.shape)}")


def exact_rows(bank: torch.Tensor):
    """(tensor, byte offset, frame bytes, row bytes) of the EXACT f32 rows inside a bank (frames, HW, …): an f32 bank (frames, HW, 256) or
    the second KiB of split_f16f6x() rows."""
    assert bank.is_contiguous() and bank.dim() in (3, 4)
    if bank.dtype == torch.float32:
        assert bank.shape[-1] == 256
        return bank, 0, bank.shape[1] * 1024, 1024
    assert bank_format(bank) == "f16f6x"
    return bank, 1024, bank.shape[1] * 2048, 2048


def f32_of_f16f6x(bank: torch.Tensor) -> torch.Tensor:
    """The f32 channels of split_f16f6x() rows as a (…, 256) f32 VIEW of the bank's second KiB."""
    assert bank_format(bank) == "f16f6x"
    return bank[..., 2:, :].view(torch.float32).flatten(-2)      # (…, 2, 128) f32 -> (…, 256): the two parts are adjacent in memory


REFINE_EPS = 2e-5   # |fgvc_pair_topk_f16f6 score - exact product| assumed by the refining merge, raw dot-product units (2.9e-4 logit at tau = 0.07);
                    # measured on the fixtures and at 480p: 7e-6 (tests/test_gpu_refine.py holds every launch's scores to half of this)


def merge_refine_workspace(n_out: int, HWq: int, device) -> torch.Tensor:
    nbytes = _lib.load().fgvc_merge_refine_workspace_bytes(int(n_out), int(HWq))
    return torch.empty(((nbytes + 15) // 16) * 4, dtype=torch.int32, device=device)


def merge_refine_topk(pair_idx: torch.Tensor, pair_score: torch.Tensor, slot_pair: torch.Tensor, pairs: torch.Tensor,
                      q_bank: torch.Tensor, k_bank: torch.Tensor, Hq: int, Wq: int, Hk: int, Wk: int, mask: MaskSpec, topk: int,
                      temperature: float, mode: str = "softmax", eps: float = REFINE_EPS, workspace: Optional[torch.Tensor] = None):
    """merge_topk() behind the approximate scores of fgvc_pair_topk_f16f6, index-exact: candidates whose approximate scores are within
    2 eps of a neighbour are re-scored from the exact rows of `q_bank` / `k_bank` (f32 (frames, HW, 256), or split_f16f6x() banks),
    queries whose window the pair lists do not close are recomputed from every candidate under `mask`.
    Returns idx, logit, weight as merge_topk(), and the int32 statistics {work items (queries re-scored + sampled), of them from scratch,
    candidates re-scored, from-scratch queries beyond the scan queue (slow path), f32 bits of the largest |approximate - exact| score
    among the re-scored candidates, the same over the UNBIASED sample (round 6: every listed entry of a pseudo-random 1/64 of the queries
    whose order needed no re-scoring), entries in that sample, queries in it (counted in the first word too)} as a device tensor (8,) (a view of the workspace: read it before the next
    call that uses the same workspace; refine_max_error() / refine_sample_error() decode words 4 and 5)."""
    pair_idx, pair_score = _chk(pair_idx, torch.int32, "pair_idx"), _chk(pair_score, torch.float32, "pair_score")
    slot_pair, pairs = _chk(slot_pair, torch.int32, "slot_pair"), _chk(pairs, torch.int32, "pairs")
    assert pair_idx.shape == pair_score.shape and pair_idx.shape[2] == topk and pair_idx.shape[1] == Hq * Wq and pairs.shape[0] == pair_idx.shape[0]
    n_out, T = slot_pair.shape
    qb, qo, qfb, qrb = exact_rows(q_bank)
    kb, ko, kfb, krb = exact_rows(k_bank)
    assert qb.is_cuda and kb.is_cuda and qb.shape[1] == Hq * Wq and kb.shape[1] == Hk * Wk
    wm = {"softmax": WEIGHT_SOFTMAX, "cosine": WEIGHT_COSINE}[mode]
    dev = pair_idx.device
    idx = torch.empty((n_out, Hq * Wq, topk), device=dev, dtype=torch.int32)
    logit = torch.empty((n_out, Hq * Wq, topk), device=dev, dtype=torch.float32)
    weight = torch.empty_like(logit)
    need = _lib.load().fgvc_merge_refine_workspace_bytes(int(n_out), int(Hq * Wq))
    if workspace is None or workspace.numel() * workspace.element_size() < need or workspace.device != dev:
        workspace = merge_refine_workspace(n_out, Hq * Wq, dev)
    _lib.call("fgvc_merge_refine_topk_f32", _ptr(pair_idx), _ptr(pair_score), _ptr(slot_pair), _ptr(pairs),
              C.c_void_p(qb.data_ptr() + qo), C.c_int64(qfb), qrb, C.c_void_p(kb.data_ptr() + ko), C.c_int64(kfb), krb,
              n_out, T, Hq, Wq, Hk, Wk, 256, topk, float(temperature), wm, float(eps), mask.r2max, mask.ry, mask.rx,
              _ptr(idx), _ptr(logit), _ptr(weight), _ptr(workspace), _stream(pair_idx))
    return idx, logit, weight, workspace.view(torch.int32)[:8]


def refine_max_error(stats: torch.Tensor) -> float:
    """The largest |approximate - exact| score (dot-product units) the refining merge saw among the candidates it re-scored: `eps` as
    measured on that call's data.  Synchronises (reads the device counters)."""
    e = stats[4:6].cpu().view(torch.float32) if stats.numel() >= 6 else stats[4:5].cpu().view(torch.float32)
    return float(e.max())                 # (both samples: the clustered candidates' and the unbiased one's -- the bound must hold for either)


def refine_sample_error(stats: torch.Tensor):
    """(largest |approximate - exact| over the unbiased sample, entries in it): refine_max_error() over candidates the refining merge did
    NOT need to re-score -- every listed entry, inside the window or not, of 1/64 of the queries whose order was proven as it stood."""
    if stats.numel() < 8:
        return None, 0
    c = stats[:8].cpu()
    return float(c[5:6].view(torch.float32)[0]), int(c[6])


def refine_counts(stats: torch.Tensor) -> dict:
    """The refining merge's counters by name (synchronises)."""
    c = stats.cpu().tolist()
    smp_q = c[7] if len(c) >= 8 else 0
    return dict(queries_rescored=c[0] - smp_q, of_them_from_scratch=c[1], candidates_rescored=c[2], beyond_scan_queue=c[3],
                sampled_queries=smp_q, sampled_entries=c[6] if len(c) >= 7 else 0)


def unsplit_f16f6p(split: torch.Tensor) -> torch.Tensor:
    """The h part of split_f16f6p() rows as f32: (…, 2, 256) int16 -> (…, 256) = h / 256 (an 11-bit approximation of the rows: tests)."""
    b = split.contiguous().view(torch.uint8).reshape(*split.shape[:-2], 1024)
    return b[..., :512].contiguous().view(torch.float16).float() * (1.0 / 256.0)


def split_f16f8(feat: torch.Tensor) -> torch.Tensor:
    """(…, C) f32 L2-normalised rows -> (…, 4 C) uint8: per pixel [h = f16(256 x) | h8 = e4m3(h) | l8 = e4m3(256 (256 x - h))],
    the operand format of fgvc_corr_volume_f16f8."""
    feat = _chk(feat, torch.float32, "feat")
    Cc = feat.shape[-1]
    n = feat.numel() // Cc
    out = torch.empty((*feat.shape[:-1], 4 * Cc), device=feat.device, dtype=torch.uint8)
    _lib.call("fgvc_split_f16f8", _ptr(feat), _ptr(out), n, Cc, _stream(feat))
    return out


def split_f16f6(feat: torch.Tensor) -> torch.Tensor:
    """(…, 256) f32 L2-normalised rows -> (…, 1024) uint8: per pixel [h = f16(256 x) | h6 | l6 | scales | pad] with h6 / l6 the
    block-scaled e2m3 forms of h and of its residual (one E8M0 scale per 32 channels; layout: csrc/corr_volume_f6.hip),
    the operand format of fgvc_corr_volume_f16f6."""
    feat = _chk(feat, torch.float32, "feat")
    Cc = feat.shape[-1]
    n = feat.numel() // Cc
    out = torch.empty((*feat.shape[:-1], 4 * Cc), device=feat.device, dtype=torch.uint8)
    _lib.call("fgvc_split_f16f6", _ptr(feat), _ptr(out), n, Cc, _stream(feat))
    return out


def corr_volume(qfeat: torch.Tensor, kfeat: torch.Tensor, temperature: float = 1.0, precision: str = "f32",
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Dense volume vol[key j][query i] = <k_j, q_i>/temperature, (HWk, HWq) f32.
    precision 'f32': qfeat (HWq,C), kfeat (HWk,C) f32.  'bf16x3' / 'bf16': the split_bf16() forms (HW,2,C).
    'f16f6' / 'f16f8': the split_f16f6() / split_f16f8() forms (HW, 4C) uint8 of L2-normalised rows, C == 256 (parity-grade;
    f16f6 is the fastest)."""
    HWq, HWk, Cc = qfeat.shape[0], kfeat.shape[0], qfeat.shape[-1]
    if out is None:
        out = torch.empty((HWk, HWq), device=qfeat.device, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.shape == (HWk, HWq) and out.dtype == torch.float32
    if precision == "f32":
        qfeat, kfeat = _chk(qfeat, torch.float32, "qfeat"), _chk(kfeat, torch.float32, "kfeat")
        _lib.call("fgvc_corr_volume_f32", _ptr(qfeat), _ptr(kfeat), Cc, HWq, HWk, float(temperature), _ptr(out),
                  _stream(qfeat))
    elif precision in ("f16f8", "f16f6"):
        qfeat, kfeat = _chk(qfeat, torch.uint8, "qfeat"), _chk(kfeat, torch.uint8, "kfeat")
        assert qfeat.dim() == 2 and qfeat.shape[1] % 4 == 0 and kfeat.shape[1] == qfeat.shape[1]
        _lib.call("fgvc_corr_volume_" + precision, _ptr(qfeat), _ptr(kfeat), qfeat.shape[1] // 4, HWq, HWk, float(temperature), _ptr(out),
                  _stream(qfeat))
    elif precision in ("bf16x3", "bf16"):
        qfeat, kfeat = _chk(qfeat, torch.int16, "qfeat"), _chk(kfeat, torch.int16, "kfeat")
        assert qfeat.dim() == 3 and qfeat.shape[1] == 2
        _lib.call("fgvc_corr_volume_" + precision, _ptr(qfeat), _ptr(kfeat), Cc, HWq, HWk, float(temperature),
                  _ptr(out), _stream(qfeat))
    else:
        raise ValueError(precision)
    return out


def dense_attend(qfeat: torch.Tensor, kfeat: torch.Tensor, labels: torch.Tensor, Hq: int, Wq: int, Hk: int, Wk: int,
                 mask: MaskSpec, temperature: float, mode: str = "softmax", non_mask_len: int = 0,
                 dense_mask: Optional[torch.Tensor] = None, precision: str = "f32") -> torch.Tensor:
    """topk=None branch (local_attention.py:376-383): weights over every unmasked key of every key slot.
    qfeat (HWq, C) f32 rows, kfeat (T, HWk, C), labels (T, HWk, P) -> (HWq, P).  One HWk x HWq volume slab lives at a time
    (fgvc_corr_volume_f32 for C = 32, 64, 128 or 256, or _bf16x3 with precision='bf16x3' for C = 64, 128 or 256 -- any other
    width is refused), streamed once by fgvc_dense_attend_f32.
    mode: 'softmax' | 'cosine' (clamp(min=0)^2) | 'raw' (the affinity itself is the weight: local_square_attention, :38-103)."""
    qfeat, kfeat = _chk(qfeat, torch.float32, "qfeat"), _chk(kfeat, torch.float32, "kfeat")
    labels = _chk(labels, torch.float32, "labels")
    T, HWk, P = labels.shape
    HWq = qfeat.shape[0]
    assert HWq == Hq * Wq and HWk == Hk * Wk and kfeat.shape[:2] == (T, HWk) and 0 <= non_mask_len <= T
    dev = qfeat.device
    wm = {"softmax": WEIGHT_SOFTMAX, "cosine": WEIGHT_COSINE, "raw": WEIGHT_RAW}[mode]
    ns = _lib.load().fgvc_dense_attend_splits(HWq, HWk)
    state = torch.empty((ns, HWq, P + 2), device=dev, dtype=torch.float32)
    vol = torch.empty((HWk, HWq), device=dev, dtype=torch.float32)
    if precision == "bf16x3":
        qs, ks = split_bf16(qfeat), split_bf16(kfeat)
    if dense_mask is not None:
        dense_mask = _chk(dense_mask.to(torch.bool), torch.bool, "dense_mask")
        assert dense_mask.shape == (HWk, HWq) and mask.is_none
    for t in range(T):
        if precision == "bf16x3":
            corr_volume(qs, ks[t], temperature, "bf16x3", out=vol)
        else:
            corr_volume(qfeat, kfeat[t], temperature, "f32", out=vol)
        masked = t >= non_mask_len
        if dense_mask is not None and masked:
            vol.masked_fill_(~dense_mask, float("-inf"))             # a user's arbitrary mask tensor: applied to the slab as given
        _lib.call("fgvc_dense_attend_f32", _ptr(vol), _ptr(labels[t]), Hq, Wq, Hk, Wk, P, int(masked and not mask.is_none),
                  min(mask.r2max, NO_LIMIT), min(mask.ry, NO_LIMIT), min(mask.rx, NO_LIMIT), wm, int(t == 0), _ptr(state), ns,
                  _stream(qfeat))
    out = torch.empty((HWq, P), device=dev, dtype=torch.float32)
    _lib.call("fgvc_dense_attend_finish_f32", _ptr(state), ns, HWq, P, wm, _ptr(out), _stream(qfeat))
    return out


def dense_propagate(aff: torch.Tensor, labels: torch.Tensor, topk: Optional[int] = None) -> torch.Tensor:
    """`propagate` for a GIVEN dense affinity (affinity_utils.py:33-50): aff (HWk, HWq) f32, labels (HWk, P) f32 -> (HWq, P)
    = labels^T-weighted column sums; topk: weights max(aff - k-th largest of the column, 0), normalised by their sum (:36-44).
    One streaming pass over `aff` per 32 label channels (fgvc_dense_propagate_f32) + one for the thresholds (fgvc_dense_kth_f32)."""
    aff, labels = _chk(aff, torch.float32, "aff"), _chk(labels, torch.float32, "labels")
    HWk, HWq = aff.shape
    assert labels.shape[0] == HWk and labels.dim() == 2
    P = labels.shape[1]
    dev = aff.device
    ns = _lib.load().fgvc_dense_attend_splits(HWq, HWk)
    thr = None
    if topk is not None:
        if not 1 <= topk <= min(64, HWk):
            raise _lib.FgvcHipError(f"propagate: topk={topk} outside 1..min(64, HWk)")
        part = torch.empty((ns, HWq, 16 if topk <= 16 else 64), device=dev, dtype=torch.float32)
        thr = torch.empty((HWq,), device=dev, dtype=torch.float32)
        _lib.call("fgvc_dense_kth_f32", _ptr(aff), HWk, HWq, int(topk), _ptr(part), ns, _ptr(thr), _stream(aff))
    out = torch.empty((HWq, P), device=dev, dtype=torch.float32)
    for p0 in range(0, P, 32):
        lab = labels[:, p0:p0 + 32].contiguous()
        pp = lab.shape[1]
        state = torch.empty((ns, HWq, pp + 2), device=dev, dtype=torch.float32)
        o = torch.empty((HWq, pp), device=dev, dtype=torch.float32)
        _lib.call("fgvc_dense_propagate_f32", _ptr(aff), _ptr(lab), HWk, HWq, pp, _ptr(thr), _ptr(state), ns, _ptr(o), _stream(aff))
        out[:, p0:p0 + pp] = o
    return out


def local_corr_topk(qfeat: torch.Tensor, kfeat: torch.Tensor, H: int, W: int, R: int, topk: int,
                    temperature: float, normalized: bool = False, split_fmt: str = "f16", presplit: bool = False):
    """A7: qfeat (1, HW, C), kfeat (K, HW, C) -> idx (HW,k) int32 = slot*(2R+1)^2 + tap, logit, weight.
    normalized=True (rows are L2-normalised) lets C == 256 / k <= 10 run on the 16-bit matrix pipe (fgvc_local_corr_topk_f16x3).
    presplit=True (round 6): qfeat / kfeat ARE split_f16x2() banks (1, HW, 2, 256) / (K, HW, 2, 256) int16 of normalised rows -- a tracker
    splits a frame once when it enters its bank, not once per query frame that correlates with it (at 480 x 854 the split of seven frames
    was 0.96 of the 4.2 ms this call took: tools/bench_cfg3.py)."""
    if presplit:
        qs, ks = _chk(qfeat, torch.int16, "qfeat"), _chk(kfeat, torch.int16, "kfeat")
        assert qs.dim() == 4 and ks.dim() == 4 and qs.shape[2:] == (2, 256) and ks.shape[2:] == (2, 256) and qs.shape[1] == ks.shape[1] == H * W
        if not split_path_ok(256, H, W, topk, True, None, MaskSpec(ry=R, rx=R), True):
            raise ValueError("local_corr_topk(presplit=True): the 16-bit local-window path needs topk <= 10 and a window within its block list")
        K, dev = ks.shape[0], qs.device
        pairs = make_pairs([(0, t) for t in range(K)], dev)
        ws_i = torch.empty((K, H * W, topk), device=dev, dtype=torch.int32)
        ws_s = torch.empty((K, H * W, topk), device=dev, dtype=torch.float32)
        idx = torch.empty((H * W, topk), device=dev, dtype=torch.int32)
        logit = torch.empty((H * W, topk), device=dev, dtype=torch.float32)
        weight = torch.empty_like(logit)
        _lib.call("fgvc_local_corr_topk_f16x3", _ptr(qs), _ptr(ks), _ptr(pairs), K, 256, H, W, R, topk,
                  float(temperature), _ptr(ws_i), _ptr(ws_s), _ptr(idx), _ptr(logit), _ptr(weight), _stream(qs))
        return idx, logit, weight
    qfeat, kfeat = _chk(qfeat, torch.float32, "qfeat"), _chk(kfeat, torch.float32, "kfeat")
    K = kfeat.shape[0]
    dev = qfeat.device
    if split_fmt != "f16":
        raise ValueError(f"split_fmt={split_fmt!r} (only 'f16')")
    if split_path_ok(qfeat.shape[-1], H, W, topk, normalized, None, MaskSpec(ry=R, rx=R), True):
        qs, ks = split_f16x2(qfeat), split_f16x2(kfeat)
        pairs = make_pairs([(0, t) for t in range(K)], dev)
        ws_i = torch.empty((K, H * W, topk), device=dev, dtype=torch.int32)
        ws_s = torch.empty((K, H * W, topk), device=dev, dtype=torch.float32)
        idx = torch.empty((H * W, topk), device=dev, dtype=torch.int32)
        logit = torch.empty((H * W, topk), device=dev, dtype=torch.float32)
        weight = torch.empty_like(logit)
        _lib.call("fgvc_local_corr_topk_f16x3", _ptr(qs), _ptr(ks), _ptr(pairs), K, qfeat.shape[-1], H, W, R, topk,
                  float(temperature), _ptr(ws_i), _ptr(ws_s), _ptr(idx), _ptr(logit), _ptr(weight), _stream(qfeat))
        return idx, logit, weight
    pairs = make_pairs([(0, t) for t in range(K)], dev)
    ws_i = torch.empty((K, H * W, topk), device=dev, dtype=torch.int32)
    ws_s = torch.empty((K, H * W, topk), device=dev, dtype=torch.float32)
    idx = torch.empty((H * W, topk), device=dev, dtype=torch.int32)
    logit = torch.empty((H * W, topk), device=dev, dtype=torch.float32)
    weight = torch.empty_like(logit)
    _lib.call("fgvc_local_corr_topk_f32", _ptr(qfeat), _ptr(kfeat), _ptr(pairs), K, qfeat.shape[-1], H, W, R, topk,
              float(temperature), _ptr(ws_i), _ptr(ws_s), _ptr(idx), _ptr(logit), _ptr(weight), _stream(qfeat))
    return idx, logit, weight


def local_merge_plan(pair_idx: torch.Tensor, pair_score: torch.Tensor, slot_pair: torch.Tensor, H: int, W: int, R: int, topk: int,
                     temperature: float, out: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None):
    """The merge of local_corr_topk() for many output frames in one launch (fgvc_local_merge_plan_f32): pair_idx / pair_score
    (n_pairs, HW, topk) from pair_topk() / pair_topk_split() under MaskSpec(ry=R, rx=R), slot_pair int32 (n_rows, max_slots) = pair of
    key slot j of row r (-1: none).  Returns idx (n_rows, HW, topk) int32 = j*(2R+1)^2 + tap, logit, weight -- or writes `out`."""
    pair_idx, pair_score = _chk(pair_idx, torch.int32, "pair_idx"), _chk(pair_score, torch.float32, "pair_score")
    slot_pair = _chk(slot_pair, torch.int32, "slot_pair")
    assert pair_idx.shape == pair_score.shape and pair_idx.shape[1:] == (H * W, topk) and slot_pair.dim() == 2
    n_rows, max_slots = slot_pair.shape
    if out is None:
        idx = torch.empty((n_rows, H * W, topk), device=pair_idx.device, dtype=torch.int32)
        logit = torch.empty((n_rows, H * W, topk), device=pair_idx.device, dtype=torch.float32)
        out = (idx, logit, torch.empty_like(logit))
    for t, dt in zip(out, (torch.int32, torch.float32, torch.float32)):
        assert t.is_contiguous() and t.dtype == dt and t.shape == (n_rows, H * W, topk) and t.device == pair_idx.device
    _lib.call("fgvc_local_merge_plan_f32", _ptr(pair_idx), _ptr(pair_score), pair_idx.shape[0], _ptr(slot_pair), n_rows, max_slots, H, W,
              R, topk, float(temperature), _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream(pair_idx))
    return out


def topk_coord(idx: torch.Tensor, weight: torch.Tensor, H: int, W: int, R: int, scale: int) -> torch.Tensor:
    """A7 get_coord: (HW,k) window lists of ONE key slot -> (HW,2) expected (x,y) image coordinates."""
    idx, weight = _chk(idx, torch.int32, "idx"), _chk(weight, torch.float32, "weight")
    assert idx.shape == weight.shape == (H * W, idx.shape[1])
    out = torch.empty((H * W, 2), device=idx.device, dtype=torch.float32)
    _lib.call("fgvc_topk_coord_f32", _ptr(idx), _ptr(weight), H, W, R, idx.shape[1], scale, _ptr(out), _stream(idx))
    return out


def topk_coord_rows(idx: torch.Tensor, weight: torch.Tensor, H: int, W: int, R: int, scale: int) -> torch.Tensor:
    """topk_coord() for many single-slot rows in one launch: (rows, HW, k) lists -> (rows, HW, 2) fields, (x, y) interleaved."""
    idx, weight = _chk(idx, torch.int32, "idx"), _chk(weight, torch.float32, "weight")
    assert idx.dim() == 3 and idx.shape == weight.shape and idx.shape[1] == H * W
    out = torch.empty((idx.shape[0], H * W, 2), device=idx.device, dtype=torch.float32)
    if idx.shape[0]:
        _lib.call("fgvc_topk_coord_rows_f32", _ptr(idx), _ptr(weight), idx.shape[0], H, W, R, idx.shape[2], int(scale), _ptr(out), _stream(idx))
    return out


def cycle_chase(fields: torch.Tensor, traj: torch.Tensor, start_xy: torch.Tensor, scale: int, H: int, W: int):
    """Walk predicted positions back to their query frame through a chain of coordinate fields (fgvc_cycle_chase_f32).
    fields (n, HW, 2) f32: fields[j] maps a position in frame s + 1 + j to frame s + j (topk_coord_rows); traj (n, P, 2) = the predicted
    (x, y) of frames s + 1 .. s + n (any float dtype: chased in f32, as the reference's forward warping does); start_xy (P, 2) = the query
    points.  Returns back (n, P, 2) f32 = where each position lands in frame s, err (n, P) f32 = its distance from the query point;
    a non-finite position at any hop, or the (-1, -1) of an all-zero map, gives back = NaN and err = +inf."""
    fields = _chk(fields, torch.float32, "fields")
    traj = _chk(traj.to(torch.float32), torch.float32, "traj")
    start_xy = _chk(start_xy.to(torch.float32), torch.float32, "start_xy")
    n, P = traj.shape[0], traj.shape[1]
    assert fields.shape == (n, H * W, 2) and traj.shape == (n, P, 2) and start_xy.shape == (P, 2)
    back = torch.empty((n, P, 2), device=traj.device, dtype=torch.float32)
    err = torch.empty((n, P), device=traj.device, dtype=torch.float32)
    if n and P:
        _lib.call("fgvc_cycle_chase_f32", _ptr(fields), _ptr(traj), _ptr(start_xy), n, P, H, W, int(scale), _ptr(back), _ptr(err),
                  _stream(traj))
    return back, err


FLOW_MODES = {"consistency": 0, "fb_abs": 1}       # FGVC_FLOW_CONSISTENCY, FGVC_FLOW_FB_ABS


def flow_from_lists(idx: torch.Tensor, weight: torch.Tensor, Hf: int, Wf: int, R: int, scale: int, size: Tuple[int, int],
                    pad: Tuple[int, int] = (0, 0), renorm: bool = True, out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Single-slot window lists -> dense flow (fgvc_flow_from_lists_f32), every row in one launch.  idx / weight (rows, Hf*Wf, k) as
    run_local_affinity returns them; `size` = the network size (h, w), `pad` = (left, top) of the padded frame the features were taken
    from (a feature cell sits on padded pixel cell * scale).  Returns flow (rows, 2, h, w) f32 in pixels, channel 0 = x, and valid
    (rows, h, w) uint8.  renorm: divide a cell's coordinate sum by its weight sum (taps outside the image dropped) before the cell's own
    coordinate is subtracted; False keeps get_coord's sum, whose zero-padded taps pull towards the origin.  `out`: (flow, valid) to write
    into, contiguous and of exactly those shapes and dtypes."""
    idx, weight = _chk(idx, torch.int32, "idx"), _chk(weight, torch.float32, "weight")
    assert idx.dim() == 3 and idx.shape == weight.shape and idx.shape[1] == Hf * Wf
    (h, w), (left, top) = (int(v) for v in size), (int(v) for v in pad)
    rows = idx.shape[0]
    if out is None:
        out = (torch.empty((rows, 2, h, w), device=idx.device, dtype=torch.float32),
               torch.empty((rows, h, w), device=idx.device, dtype=torch.uint8))
    flow, valid = out
    for t, dt, shp in ((flow, torch.float32, (rows, 2, h, w)), (valid, torch.uint8, (rows, h, w))):
        if not (t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shp and t.device == idx.device):
            raise ValueError(f"out: contiguous {dt} of shape {shp} on {idx.device}, got {t.dtype} {tuple(t.shape)}")
    if rows:
        _lib.call("fgvc_flow_from_lists_f32", _ptr(idx), _ptr(weight), rows, Hf, Wf, int(R), idx.shape[2], int(scale), int(bool(renorm)),
                  h, w, left, top, _ptr(flow), _ptr(valid), _stream(idx))
    return flow, valid


def _flow_mode(mode: str) -> int:
    if mode == "range_map":
        raise NotImplementedError("fgvc_amd: occlusion mode 'range_map' is a scatter-add whose threshold depends on the summation order; "
                                  "only 'consistency' and 'fb_abs' are built")
    if mode not in FLOW_MODES:
        raise ValueError(f"mode={mode!r}: one of {tuple(FLOW_MODES)} ('range_map' is not built)")
    return FLOW_MODES[mode]


def flow_consistency(flow_fw: torch.Tensor, flow_bw: torch.Tensor, mode: str = "consistency", diff: float = 1.5):
    """Both directions of the reference's occlusion_estimation in one launch (fgvc_flow_consistency_f32): flows (n, 2, h, w) f32 ->
    occ_fw, occ_bw (n, 1, h, w) f32, 1 = consistent.  mode 'consistency' | 'fb_abs' (`diff` is read by 'fb_abs' only)."""
    m = _flow_mode(mode)
    flow_fw, flow_bw = _chk(flow_fw, torch.float32, "flow_fw"), _chk(flow_bw, torch.float32, "flow_bw")
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2 or flow_bw.shape != flow_fw.shape:
        raise ValueError(f"flow_fw / flow_bw: two (n, 2, h, w) tensors, got {tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}")
    n, _, h, w = flow_fw.shape
    occ_fw = torch.empty((n, 1, h, w), device=flow_fw.device, dtype=torch.float32)
    occ_bw = torch.empty_like(occ_fw)
    if occ_fw.numel():
        _lib.call("fgvc_flow_consistency_f32", _ptr(flow_fw), _ptr(flow_bw), n, h, w, m, float(diff), _ptr(occ_fw), _ptr(occ_bw),
                  _stream(flow_fw))
    return occ_fw, occ_bw


def warp(feat: torch.Tensor, flow: torch.Tensor, align_corners: bool = False, use_mask: bool = True) -> torch.Tensor:
    """The reference's Warp.forward(feat, flow) with mode='bilinear', padding_mode='zeros' (fgvc_warp_f32): feat (N, C, H, W) f32,
    flow (N, 2, H, W) f32 -> (N, C, H, W)."""
    feat, flow = _chk(feat, torch.float32, "feat"), _chk(flow, torch.float32, "flow")
    if feat.dim() != 4 or flow.dim() != 4 or flow.shape[1] != 2 or flow.shape[0] != feat.shape[0] or flow.shape[2:] != feat.shape[2:]:
        raise ValueError(f"feat (N, C, H, W) and flow (N, 2, H, W), got {tuple(feat.shape)} and {tuple(flow.shape)}")
    N, Cn, H, W = feat.shape
    out = torch.empty_like(feat)
    if out.numel():
        _lib.call("fgvc_warp_f32", _ptr(feat), _ptr(flow), N, Cn, H, W, int(bool(align_corners)), int(bool(use_mask)), _ptr(out),
                  _stream(feat))
    return out


CHAIN_VISIBILITIES = {"frame": 0, "consistency": 1}       # FGVC_CHAIN_FRAME, FGVC_CHAIN_CONSISTENCY


def flow_chain(flow_fw: torch.Tensor, flow_bw: torch.Tensor, query: torch.Tensor, ok_fw: Optional[torch.Tensor] = None,
               ok_bw: Optional[torch.Tensor] = None, visibility: str = "frame", out=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Query points tracked through a clip in both time directions by chaining its flow (fgvc_flow_chain_f32), one launch: the reference's
    RAFT.forward_test chain (raft.py:247-289) bit for bit.  flow_fw / flow_bw (T-1, 2, h, w) f32 as forward_test_flow returns them at
    step = 1; query (P, 3) f32 = (t, x, y) (any strides: a contiguous copy is chained); ok_fw / ok_bw (T-1, h, w) uint8, needed by
    visibility='consistency' (a frame is visible while it is inside the frame and every hop from the query frame started inside it on a
    set mask pixel) and not read by 'frame' (inside the frame, per frame).  Returns traj (T, P, 2) f32 and vis (T, P) uint8.  A position
    that is non-finite or beyond 2^23 ends its side of the track in NaN, invisible; so does a query time that is no integer of [0, T).
    T = 1 returns the query points, P = 0 empty tensors without a launch.  `out`: (traj, vis) to write into, contiguous and of exactly
    those shapes and dtypes."""
    if visibility not in CHAIN_VISIBILITIES:
        raise ValueError(f"visibility={visibility!r}: one of {tuple(CHAIN_VISIBILITIES)}")
    flow_fw, flow_bw = _chk(flow_fw, torch.float32, "flow_fw"), _chk(flow_bw, torch.float32, "flow_bw")
    query = _chk(query, torch.float32, "query")
    if flow_fw.dim() != 4 or flow_fw.shape[1] != 2 or flow_bw.shape != flow_fw.shape:
        raise ValueError(f"flow_fw / flow_bw: two (T-1, 2, h, w) tensors, got {tuple(flow_fw.shape)} and {tuple(flow_bw.shape)}")
    if query.dim() != 2 or query.shape[1] != 3:
        raise ValueError(f"query: (P, 3) = (t, x, y), got {tuple(query.shape)}")
    n, _, h, w = flow_fw.shape
    T, P, dev = n + 1, query.shape[0], flow_fw.device
    if visibility == "consistency":
        if ok_fw is None or ok_bw is None:
            raise ValueError("visibility='consistency' needs ok_fw and ok_bw, (T-1, h, w) uint8")
        ok_fw, ok_bw = _chk(ok_fw, torch.uint8, "ok_fw"), _chk(ok_bw, torch.uint8, "ok_bw")
        if tuple(ok_fw.shape) != (n, h, w) or tuple(ok_bw.shape) != (n, h, w):
            raise ValueError(f"ok_fw / ok_bw: two ({n}, {h}, {w}) tensors, got {tuple(ok_fw.shape)} and {tuple(ok_bw.shape)}")
    else:
        ok_fw = ok_bw = None
    if out is None:
        out = (torch.empty((T, P, 2), device=dev, dtype=torch.float32), torch.empty((T, P), device=dev, dtype=torch.uint8))
    traj, vis = out
    for t, dt, shp in ((traj, torch.float32, (T, P, 2)), (vis, torch.uint8, (T, P))):
        if not (t.is_contiguous() and t.dtype == dt and tuple(t.shape) == shp and t.device == dev):
            raise ValueError(f"out: contiguous {dt} of shape {shp} on {dev}, got {t.dtype} {tuple(t.shape)}")
    if P:
        _lib.call("fgvc_flow_chain_f32", _ptr(flow_fw if n else None), _ptr(flow_bw if n else None), _ptr(ok_fw if n else None),
                  _ptr(ok_bw if n else None), _ptr(query), T, P, h, w, CHAIN_VISIBILITIES[visibility], _ptr(traj), _ptr(vis), _stream(query))
    return traj, vis


def c2f_refine(coarse_arg: torch.Tensor, qfine: torch.Tensor, kfine: torch.Tensor, vfine: torch.Tensor, H: int,
               W: int, scale: int, Rf: int, topk: int, temperature: float, mode: str = "softmax"):
    """A6 fine stage. coarse_arg int32 (T, HW); qfine (sHsW, Cf); kfine (T, sHsW, Cf); vfine (T, sHsW, P); mode "softmax" or
    "cosine" (clamp(affinity, 0)^2, local_attention.py:858-861)."""
    coarse_arg = _chk(coarse_arg, torch.int32, "coarse_arg")
    qfine, kfine = _chk(qfine, torch.float32, "qfine"), _chk(kfine, torch.float32, "kfine")
    vfine = _chk(vfine, torch.float32, "vfine")
    T, Cf, P = kfine.shape[0], kfine.shape[-1], vfine.shape[-1]
    assert coarse_arg.shape == (T, H * W) and kfine.shape[1] == H * W * scale * scale == vfine.shape[1]
    assert int(coarse_arg.min()) >= 0 and int(coarse_arg.max()) < H * W
    dev = qfine.device
    out = torch.empty((H * W, P), device=dev, dtype=torch.float32)
    idx = torch.empty((H * W, topk), device=dev, dtype=torch.int32)
    logit = torch.empty((H * W, topk), device=dev, dtype=torch.float32)
    _lib.call("fgvc_c2f_refine_mode_f32", _ptr(coarse_arg), _ptr(qfine), _ptr(kfine), _ptr(vfine), T, H, W, scale, Cf, P,
              Rf, topk, float(temperature), {"softmax": WEIGHT_SOFTMAX, "cosine": WEIGHT_COSINE}[mode], _ptr(out), _ptr(idx), _ptr(logit),
              _stream(qfine))
    return out, idx, logit


def bn_act(x: torch.Tensor, bn: "torch.nn.BatchNorm2d", residual: Optional[torch.Tensor] = None, relu: bool = True,
           inplace: bool = True) -> torch.Tensor:
    """Inference BatchNorm2d (+ residual) (+ ReLU) in one pass over a contiguous NCHW f32 tensor."""
    x = _chk(x, torch.float32, "x")
    N, Cc = x.shape[0], x.shape[1]
    HW = x[0, 0].numel()
    if residual is not None:
        residual = _chk(residual, torch.float32, "residual")
        assert residual.shape == x.shape
    out = x if inplace else torch.empty_like(x)
    _lib.call("fgvc_bn_act_f32", _ptr(x), _ptr(residual), _ptr(bn.running_mean), _ptr(bn.running_var),
              _ptr(bn.weight), _ptr(bn.bias), float(bn.eps), int(relu), _ptr(out), N, Cc, HW, _stream(x))
    return out


# ---- encoder convolutions on the bf16 pipe (fgvc_conv_split_f32) ---------------------------------------------------
def conv_pad_dims(H: int, W: int) -> Tuple[int, int]:
    """(Hp, Wp) of the zero-bordered "padded split NHWC" activation buffers for an H x W image."""
    return 8 * (-(-H // 8)) + 2, 32 * (-(-W // 32)) + 8


def _split_pair(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return hi, lo


def prepare_conv_split(weight: torch.Tensor, bn: "torch.nn.BatchNorm2d") -> Tuple[torch.Tensor, torch.Tensor]:
    """Fold eval-mode BatchNorm into a conv weight (Cout, Cin, KS, KS) and lay it out for fgvc_conv_split_f32:
    returns (w int16 [KS*KS][Cin/32][Cout][64] = (hi 32 ci | lo 32 ci) bf16 bit patterns, bias f32 [Cout])."""
    Cout, Cin, KS, _ = weight.shape
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
    w = weight.float() * scale.view(-1, 1, 1, 1)
    bias = (bn.bias - bn.running_mean * scale).float().contiguous()
    w = w.permute(2, 3, 1, 0).reshape(KS * KS, Cin // 32, 32, Cout).permute(0, 1, 3, 2).contiguous()   # [tap][chunk][co][32 ci]
    hi, lo = _split_pair(w)
    packed = torch.cat([hi, lo], dim=-1).contiguous().view(torch.int16)
    return packed, bias


# formats of the encoder's split activation / weight tensors (include/fgvc_hip.h: FGVC_ACT_*) and the fixed power-of-two scales of the
# e4m3 parts of the F16F8 form (csrc/common.hpp: F8_AX ...): h8 = e4m3(h 2^-A), l8 = e4m3(l 2^B)
ACT_BF16X2, ACT_F16F8, ACT_F16X2, ACT_F16F6 = 0, 1, 2, 3
ACT_FMT = {"bf16x3": ACT_BF16X2, "f16f8": ACT_F16F8, "f16x3": ACT_F16X2, "f16f6": ACT_F16F6}
F8_AX, F8_BX, F8_AW, F8_BW = 7, 3, 2, 9
F16_TARGET_LOG2 = 8            # a calibrated tensor's largest value sits at ~2^8 of the f16 range (top 2^16): 2^7-2^8 of headroom


def act_scale_log2(amax: float, target_log2: int = F16_TARGET_LOG2) -> int:
    """log2 of the power-of-two scale that puts a tensor whose largest magnitude is `amax` at (2^(target-1), 2^target] in f16
    (default (2^7, 2^8]; ResNet's canonical calibration asks for 2^6: 2^10 of headroom)."""
    return _pow2_exponent(amax, target_log2)


def _pow2_exponent(amax: float, target_log2: int) -> int:
    """e with amax * 2^e in (2^(target-1), 2^target]; 0 for an all-zero tensor (a zero-initialised residual branch: any scale
    represents it exactly); clamped to +-45 so that the combined exponents stay inside the C ABI's range; a tensor holding inf /
    NaN is an error, not a scale."""
    amax = float(amax)
    if not math.isfinite(amax):
        raise ValueError("a tensor with inf / NaN values has no f16 scale")
    if amax <= 0.0:
        return 0
    return max(-45, min(45, target_log2 - int(math.ceil(math.log2(amax)))))


def _e2m3_blocks(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(..., 32) f32 holding f16 values -> (24 bytes per block (..., 24) uint8, field (...,) int32): the block's FP6 (e2m3) string as
    v_cvt_scalef32_pk32_fp6_f16 writes it (element e in bits [6 e, 6 e + 6), round to nearest even) under the scale 2^(field - 127) =
    the smallest power of two that keeps the block's largest magnitude at or below 7.5 (csrc/common.hpp: split_f16f6_chunk)."""
    m = x.abs().amax(-1).float().contiguous()
    mb = m.view(torch.int32)
    field = ((mb >> 23) - 2 + ((mb & 0x7FFFFF) > 0x700000).to(torch.int32)).clamp(min=32)
    y = x.float() * torch.exp2((127 - field).float()).unsqueeze(-1)              # exact: a power of two
    a = y.abs().clamp(max=7.5)
    step = torch.where(a < 2, 0.125, torch.where(a < 4, 0.25, 0.5))
    r = (torch.round(a / step) * step).clamp(max=7.5)                            # torch.round: half to even
    code = torch.where(r < 2, 8 * r, torch.where(r < 4, 8 + 4 * r, 16 + 2 * r)).to(torch.int32) | ((y < 0).to(torch.int32) << 5)
    c = code.reshape(*code.shape[:-1], 8, 4)
    w24 = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    by = torch.stack([w24 & 255, (w24 >> 8) & 255, (w24 >> 16) & 255], dim=-1).reshape(*code.shape[:-1], 24).to(torch.uint8)
    return by, field


def _e2m3_decode(by: torch.Tensor, field: torch.Tensor) -> torch.Tensor:
    """The inverse of _e2m3_blocks on its grid: (..., 24) uint8, (...,) scale fields -> (..., 32) f32."""
    b = by.to(torch.int32).reshape(*by.shape[:-1], 8, 3)
    w24 = b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)
    code = torch.stack([(w24 >> (6 * i)) & 63 for i in range(4)], dim=-1).reshape(*by.shape[:-1], 32)
    e, mnt = (code >> 3) & 3, (code & 7).float()
    mag = torch.where(e == 0, mnt * 0.125, (1.0 + mnt * 0.125) * torch.exp2((e - 1).float()))
    val = torch.where((code & 32) != 0, -mag, mag)
    return val * torch.exp2((field.to(torch.int32) - 127).float()).unsqueeze(-1)


def _f16f6_slots(h: torch.Tensor, l: torch.Tensor, first: str) -> torch.Tensor:
    """h (..., 32) f16, l (..., 32) f32 = the exact residuals -> the 128-byte rows (..., 128) uint8 of format ACT_F16F6:
    [h 64 B | slot 4, 5: the main 16 bytes of the two FP6 blocks | slot 6, 7: their 8-byte tails + scale byte + zeros]; `first` names the
    block in slots 4 / 6 ("l": activations, "h": weights)."""
    h6, fh = _e2m3_blocks(h.float())
    l6, fl = _e2m3_blocks((l * 2048.0).to(torch.float16).float())
    fl = fl - 11

    def tail(b6, f):
        t = torch.zeros((*b6.shape[:-1], 16), dtype=torch.uint8, device=b6.device)
        t[..., :8] = b6[..., 16:]
        t[..., 8] = f.to(torch.uint8)
        return t
    A, B = ((l6, fl), (h6, fh)) if first == "l" else ((h6, fh), (l6, fl))
    return torch.cat([h.contiguous().view(torch.uint8).reshape(*h.shape[:-1], 64), A[0][..., :16], B[0][..., :16], tail(*A), tail(*B)], dim=-1)


def prepare_conv_split_f16(weight: torch.Tensor, bn: "torch.nn.BatchNorm2d", fmt: int, force_exp: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """prepare_conv_split for the f16 operand forms: returns (w int16 [KS*KS][Cin/32][Cout][64] -- 128-byte rows in format `fmt` --,
    bias f32 [Cout], log2 of the weights' scale s_w).  ACT_F16F8 rows: [h = f16(s_w w) 32 | h8 = e4m3(h / 4) 32 B | l8 = e4m3(512 (s_w w - h))
    32 B]; ACT_F16X2 rows: [h 32 | l = f16(s_w w - h) 32]; ACT_F16F6 rows: [h 32 | the block-scaled FP6 forms of h (slots 4, 6) and of
    the residual (slots 5, 7): csrc/common.hpp]; s_w = the power of two that puts max|w| at (2^9, 2^10], or 2^force_exp."""
    assert fmt in (ACT_F16F8, ACT_F16X2, ACT_F16F6)
    Cout, Cin, KS, _ = weight.shape
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
    w = weight.detach().float() * scale.view(-1, 1, 1, 1)
    bias = (bn.bias - bn.running_mean * scale).detach().float().contiguous()
    w = w.permute(2, 3, 1, 0).reshape(KS * KS, Cin // 32, 32, Cout).permute(0, 1, 3, 2).contiguous()   # [tap][chunk][co][32 ci]
    e = _pow2_exponent(float(w.abs().max()), 10)
    if force_exp is not None:         # (a projection folded into another convolution's sums shares that convolution's combined scale)
        e = int(force_exp)
        assert float(w.abs().max()) * 2.0 ** e < 32768.0, "prepare_conv_split_f16: the forced scale leaves the f16 range"
    ws = w * (2.0 ** e)
    h = ws.to(torch.float16)
    l = ws - h.float()                                                  # exact in f32
    if fmt == ACT_F16X2:
        packed = torch.cat([h, l.to(torch.float16)], dim=-1).contiguous().view(torch.int16)
        return packed, bias, e
    if fmt == ACT_F16F6:
        return _f16f6_slots(h, l, "h").contiguous().view(torch.int16), bias, e
    h8 = (h.float() * 2.0 ** -F8_AW).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    l8 = (l * 2.0 ** F8_BW).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    packed = torch.cat([h.contiguous().view(torch.uint8), h8.view(torch.uint8), l8.view(torch.uint8)], dim=-1).contiguous()   # 64 + 32 + 32 B
    return packed.view(torch.int16), bias, e


def prepare_conv64(weight: torch.Tensor, bn: "torch.nn.BatchNorm2d") -> Tuple[torch.Tensor, torch.Tensor]:
    """Folded weights (64, 64, 3, 3) for fgvc_conv64_split_f32: prepare_conv_split's values in MFMA-operand order
    [2 output tiles][9 taps][2 chunks][2 k-steps][hi | lo][lane][8]; returns (w int16, bias f32 [64])."""
    assert tuple(weight.shape) == (64, 64, 3, 3)
    packed, bias = prepare_conv_split(weight, bn)                      # [tap 9][chunk 2][Cout 64][part 2 x 32 ci]
    v = packed.view(9, 2, 2, 32, 2, 2, 2, 8)                           # [t][c][ct][n][part][s][h][j]
    v = v.permute(2, 0, 1, 5, 4, 6, 3, 7).contiguous()                 # [ct][t][c][s][part][h][n][j]
    return v.view(2, 9, 2, 2, 2, 64, 8), bias


def prepare_conv64_f16(weight: torch.Tensor, bn: "torch.nn.BatchNorm2d") -> Tuple[torch.Tensor, torch.Tensor, int]:
    """Folded weights (64, 64, 3, 3) for fgvc_conv64_split_fmt_f32 with in_fmt = ACT_F16F8: prepare_conv_split_f16's rows
    ([h 64 B | h8 32 B | l8 32 B] per output channel and 32-channel chunk) in MFMA-operand order, per (output tile, tap, chunk) 4 KiB:
    [f16 k-step 0][64 lanes][16 B], [f16 k-step 1][64 lanes][16 B], then [64 lanes][h8 16 B | l8 16 B] (lane = 32 * half + cout % 32;
    a half's 16 bytes of an fp8 vector are its bytes 16 half .. 16 half + 15).  Returns (w int16 (2, 9, 2, 2048), bias, log2 s_w)."""
    assert tuple(weight.shape) == (64, 64, 3, 3)
    packed, bias, e = prepare_conv_split_f16(weight, bn, ACT_F16F8)      # int16 [tap 9][chunk 2][Cout 64][64]
    rows = packed.view(torch.uint8).view(9, 2, 2, 32, 128)               # [t][c][ct][n][128 B]
    hpart = rows[..., :64].reshape(9, 2, 2, 32, 2, 2, 16)                # [t][c][ct][n][s][half][16 B]
    f16 = hpart.permute(2, 0, 1, 4, 5, 3, 6)                             # [ct][t][c][s][half][n][16]
    h8 = rows[..., 64:96].reshape(9, 2, 2, 32, 2, 16)                    # [t][c][ct][n][half][16]
    l8 = rows[..., 96:128].reshape(9, 2, 2, 32, 2, 16)
    x = torch.stack([h8, l8], dim=-2).permute(2, 0, 1, 4, 3, 5, 6)       # [ct][t][c][half][n][h8 | l8][16]
    out = torch.cat([f16.reshape(2, 9, 2, 2048), x.reshape(2, 9, 2, 2048)], dim=-1).contiguous()   # 2 KiB of f16 fragments + 2 KiB of fp8
    return out.view(torch.int16), bias, e


def prepare_conv_s2(weight: torch.Tensor, bn: "torch.nn.BatchNorm2d") -> Tuple[torch.Tensor, torch.Tensor]:
    """Folded weights for fgvc_conv_s2_split_f32: prepare_conv_split's values in MFMA-operand order
    [KS*KS][Cin/32][Cout/32][hi k0-15 | hi k16-31 | lo k0-15 | lo k16-31][lane = 32 * (k >> 3 & 1) + cout % 32][k & 7]
    (one contiguous KiB per operand); returns (w int16, bias f32 [Cout])."""
    packed, bias = prepare_conv_split(weight, bn)                      # [tap][chunk][Cout][part 2 x 32 ci]
    T, nch, Cout, _ = packed.shape
    assert Cout % 32 == 0
    v = packed.view(T, nch, Cout // 32, 32, 2, 2, 2, 8)                # [t][c][ct][n][part][s][h][j]
    v = v.permute(0, 1, 2, 4, 5, 6, 3, 7).contiguous()                 # [t][c][ct][part][s][h][n][j]
    return v.view(T, nch, Cout // 32, 4, 64, 8), bias


def prepare_stem7(weight: torch.Tensor, bn: "torch.nn.BatchNorm2d") -> Tuple[torch.Tensor, torch.Tensor]:
    """Folded weights (64, 3, 7, 7) for fgvc_stem7_split_f32: per kernel row ky a K block of 32 with k = 4 kx + c (c = 3
    and kx = 7 are zero), as (hi, lo) bf16 in MFMA-operand order [7][2 k-steps][2 output tiles][hi | lo][lane][8];
    returns (w int16, bias f32 [64])."""
    Cout, Cin, KS, _ = weight.shape
    assert (Cout, Cin, KS) == (64, 3, 7)
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).float()
    w = weight.float() * scale.view(-1, 1, 1, 1)
    bias = (bn.bias - bn.running_mean * scale).float().contiguous()
    k = torch.zeros((Cout, 7, 8, 4), device=w.device, dtype=torch.float32)        # [co][ky][kx (8)][c (4)]
    k[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    k = k.reshape(2, 32, 7, 2, 2, 8)                                                # [ct][n][ky][s][h][j]
    k = k.permute(2, 3, 0, 4, 1, 5).contiguous()                                    # [ky][s][ct][h][n][j]
    hi, lo = _split_pair(k)
    packed = torch.stack([hi, lo], dim=3).contiguous()                              # [ky][s][ct][part][h][n][j]
    return packed.view(torch.int16).view(7, 2, 2, 2, 64, 8), bias


def alloc_split_nhwc(N: int, C: int, H: int, W: int, device) -> torch.Tensor:
    Hp, Wp = conv_pad_dims(H, W)
    return torch.zeros((N, Hp, Wp, C // 32, 64), device=device, dtype=torch.int16)


def alloc_nhwc(N: int, C: int, H: int, W: int, device) -> torch.Tensor:
    """Dense NHWC f32 (N,H,W,C): residual / f32 output of conv_split; `.permute(0,3,1,2)` is a channels_last NCHW tensor."""
    return torch.empty((N, H, W, C), device=device, dtype=torch.float32)


def nhwc_to_split(x: torch.Tensor, out: torch.Tensor, relu: bool = False) -> torch.Tensor:
    """dense NHWC f32 (N,H,W,C) -> padded split NHWC `out` (zero border); relu=True applies ReLU to x IN PLACE first."""
    x = _chk(x, torch.float32, "x")
    N, H, W, C = x.shape
    Hp, Wp = conv_pad_dims(H, W)
    assert out.shape == (N, Hp, Wp, C // 32, 64) and out.dtype == torch.int16 and out.is_contiguous()
    _lib.call("fgvc_nhwc_to_split_f32", _ptr(x), _ptr(out), N, C, H, W, Hp, Wp, int(relu), _stream(x))
    return out


def nchw_to_split_nhwc(x: torch.Tensor, out: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None,
                       want_split: bool = True) -> Optional[torch.Tensor]:
    """f32 (N,C,H,W) -> padded split NHWC (N,Hp,Wp,C/32,64) int16 [and/or dense NHWC f32 `out_f32` (N,H,W,C)];
    the split destination must have a zero border (alloc_split_nhwc)."""
    x = _chk(x, torch.float32, "x")
    N, C, H, W = x.shape
    if out is None and want_split:
        out = alloc_split_nhwc(N, C, H, W, x.device)
    Hp, Wp = conv_pad_dims(H, W)
    if out is not None:
        assert out.shape == (N, Hp, Wp, C // 32, 64) and out.dtype == torch.int16 and out.is_contiguous()
    if out_f32 is not None:
        assert out_f32.shape == (N, H, W, C) and out_f32.dtype == torch.float32 and out_f32.is_contiguous()
    _lib.call("fgvc_nchw_to_split_nhwc_f32", _ptr(x), _ptr(out), _ptr(out_f32), N, C, H, W, Hp, Wp, _stream(x))
    return out


def conv_split(x_split: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, H: int, W: int, relu: bool,
               residual: Optional[torch.Tensor] = None, out_split: Optional[torch.Tensor] = None,
               out_f32: Optional[torch.Tensor] = None, in_fmt: int = ACT_BF16X2, in_scale_log2: int = 0,
               out_fmt: int = ACT_BF16X2, out_scale_log2: int = 0, overflow: Optional[torch.Tensor] = None,
               x2_split: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None) -> None:
    """fgvc_conv_split_fmt_f32: y = conv(x, w) + bias [+ residual] [ReLU] into out_split and/or out_f32 (interiors only).
    With `x2_split` / `w2` (fgvc_conv_split_proj_fmt_f32; 3 x 3, 256 output channels): + conv1x1(x2, w2) in the same sums -- a block's
    projection shortcut; x2 in x's format and geometry, w2 (1, Cin2/32, 256, 64) scaled so that s_x2 s_w2 = 2^in_scale_log2 too, `bias`
    the sum of both folded biases.
    in_fmt: ACT_* format of x_split AND w (prepare_conv_split / prepare_conv_split_f16), in_scale_log2 = log2(s_x s_w);
    out_fmt / out_scale_log2: format and scale of out_split; overflow: int32 device word OR-ed with 1 when an f16-format output
    leaves the f16 range."""
    x_split, w = _chk(x_split, torch.int16, "x_split"), _chk(w, torch.int16, "w")
    bias = _chk(bias, torch.float32, "bias")
    N, Hp, Wp, nch, _ = x_split.shape
    taps, nch_w, Cout, _ = w.shape
    assert nch_w == nch and taps in (1, 9) and bias.shape == (Cout,)
    for t, dt, shape in ((residual, torch.float32, (N, H, W, Cout)), (out_f32, torch.float32, (N, H, W, Cout)),
                         (out_split, torch.int16, (N, Hp, Wp, Cout // 32, 64))):
        if t is not None:
            assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == x_split.device, "conv_split buffer"
    if out_fmt != ACT_BF16X2 and out_split is not None:
        assert overflow is not None and overflow.dtype == torch.int32 and overflow.device == x_split.device
    if x2_split is not None:
        x2_split, w2 = _chk(x2_split, torch.int16, "x2_split"), _chk(w2, torch.int16, "w2")
        assert taps == 9 and Cout == 256, "conv_split: a second input goes with the 3 x 3 form of 256 output channels"
        assert tuple(x2_split.shape[:3]) == (N, Hp, Wp) and x2_split.shape[4] == 64 and tuple(w2.shape) == (1, x2_split.shape[3], Cout, 64)
        _lib.call("fgvc_conv_split_proj_fmt_f32", _ptr(x_split), _ptr(w), _ptr(x2_split), _ptr(w2), _ptr(bias), _ptr(residual), _ptr(out_split),
                  _ptr(out_f32), N, H, W, Hp, Wp, nch * 32, x2_split.shape[3] * 32, int(relu), int(in_fmt), int(in_scale_log2), int(out_fmt),
                  int(out_scale_log2), _ptr(overflow), _stream(x_split))
        return
    _lib.call("fgvc_conv_split_fmt_f32", _ptr(x_split), _ptr(w), _ptr(bias), _ptr(residual), _ptr(out_split), _ptr(out_f32),
              N, H, W, Hp, Wp, nch * 32, Cout, 3 if taps == 9 else 1, int(relu), int(in_fmt), int(in_scale_log2), int(out_fmt),
              int(out_scale_log2), _ptr(overflow), _stream(x_split))


def conv_split_to_bank(x_split: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, H: int, W: int, relu: bool, bank: torch.Tensor,
                       residual: Optional[torch.Tensor] = None, in_fmt: int = ACT_BF16X2, in_scale_log2: int = 0,
                       normalize: bool = True) -> torch.Tensor:
    """fgvc_conv_split_bank_f16f6p_f32: conv_split() for Cout = 256 whose epilogue L2-normalises every pixel and writes it as a row of
    split_f16f6p() -- `bank` (N, H*W, 2, 256) int16 (a slice of the tracker's feature bank) -- instead of any dense or split tensor:
    byte for byte normalize_nhwc(out_f32 of conv_split(...), split="f16f6")."""
    x_split, w = _chk(x_split, torch.int16, "x_split"), _chk(w, torch.int16, "w")
    bias = _chk(bias, torch.float32, "bias")
    N, Hp, Wp, nch, _ = x_split.shape
    taps, nch_w, Cout, _ = w.shape
    assert nch_w == nch and taps == 9 and bias.shape == (Cout,) and Cout == 256, "conv_split_to_bank: a 3 x 3 convolution with 256 output channels"
    assert bank.dtype == torch.int16 and tuple(bank.shape) in ((N, H * W, 2, 256), (N, H * W, 4, 256)) and bank.is_contiguous() and bank.device == x_split.device
    if residual is not None:
        assert residual.dtype == torch.float32 and tuple(residual.shape) == (N, H, W, Cout) and residual.is_contiguous()
    # (N, H*W, 4, 256): the 2 KiB rows of split_f16f6x() -- the normalised f32 channels behind every row
    _lib.call("fgvc_conv_split_bank_f16f6x_f32" if bank.shape[2] == 4 else "fgvc_conv_split_bank_f16f6p_f32", _ptr(x_split), _ptr(w), _ptr(bias), _ptr(residual), _ptr(bank), N, H, W, Hp, Wp,
              nch * 32, 3, int(relu), int(in_fmt), int(in_scale_log2), int(normalize), _stream(x_split))
    return bank


def conv64_split(x_split: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, H: int, W: int, relu: bool,
                 residual: Optional[torch.Tensor] = None, out_split: Optional[torch.Tensor] = None,
                 out_f32: Optional[torch.Tensor] = None, residual_split: Optional[torch.Tensor] = None,
                 in_fmt: int = ACT_BF16X2, in_scale_log2: int = 0, out_fmt: int = ACT_BF16X2, out_scale_log2: int = 0,
                 overflow: Optional[torch.Tensor] = None) -> None:
    """conv_split for Cin = Cout = 64, 3x3, with register-resident weights (fgvc_conv64_split_fmt_f32).  in_fmt ACT_BF16X2: w, bias
    from prepare_conv64; ACT_F16F8: from prepare_conv64_f16, in_scale_log2 = log2(s_x) + its log2 s_w.  out_fmt / out_scale_log2 /
    overflow as in conv_split.  The residual is dense NHWC f32 (`residual`) or, for bf16 tensors, a padded split NHWC tensor of
    x_split's shape (`residual_split`: hi + lo is added)."""
    x_split = _chk(x_split, torch.int16, "x_split")
    N, Hp, Wp, nch, _ = x_split.shape
    assert nch == 2 and bias.shape == (64,)
    assert tuple(w.shape) == ((2, 9, 2, 2, 2, 64, 8) if in_fmt == ACT_BF16X2 else (2, 9, 2, 2048)), "conv64_split weights / in_fmt"
    assert residual is None or residual_split is None, "one residual, f32 or split"
    for t, dt, shape in ((residual, torch.float32, (N, H, W, 64)), (out_f32, torch.float32, (N, H, W, 64)),
                         (out_split, torch.int16, (N, Hp, Wp, 2, 64)), (residual_split, torch.int16, (N, Hp, Wp, 2, 64))):
        if t is not None:
            assert t.dtype == dt and tuple(t.shape) == shape and t.is_contiguous() and t.device == x_split.device, "conv64_split buffer"
    _lib.call("fgvc_conv64_split_fmt_f32", _ptr(x_split), _ptr(w), _ptr(bias), _ptr(residual), _ptr(residual_split), _ptr(out_split),
              _ptr(out_f32), N, H, W, Hp, Wp, int(relu), int(in_fmt), int(in_scale_log2), int(out_fmt), int(out_scale_log2),
              _ptr(overflow), _stream(x_split))


def conv_s2_split(x_split: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, H: int, W: int, relu: bool,
                  out_split: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None, out_fmt: int = ACT_BF16X2,
                  out_scale_log2: int = 0, overflow: Optional[torch.Tensor] = None,
                  proj: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None, proj_relu: bool = False) -> None:
    """3x3 / stride 2 / pad 1 or 1x1 / stride 2 convolution + bias (+ ReLU) on the bf16 pipe (fgvc_conv_s2_split_f32).
    x_split: padded split NHWC of the (N, H, W) input; w, bias from prepare_conv_s2; outputs for the
    ((H-1)//2+1, (W-1)//2+1) result: out_split (padded split NHWC) and / or out_f32 (dense NHWC f32).
    proj = (w2, bias2, out2_f32): the block's 1x1 / stride 2 projection of the same input in the same launch (3x3 form only,
    fgvc_conv_s2_split_proj_fmt_f32): w2, bias2 from prepare_conv_s2 of the 1x1 weights with the same Cout, out2_f32 dense NHWC f32;
    both results equal the two separate calls bit for bit."""
    N, Hp, Wp, nch, _ = x_split.shape
    taps, nch_w, n_ct = w.shape[:3]
    Cout = n_ct * 32
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if proj is not None:                       # refused on the host, before anything touches the device
        w2, bias2, out2 = proj
        if taps != 9:
            raise ValueError("conv_s2_split: a projection rides in the 3x3 form only (w has %d taps)" % taps)
        if w2.dim() != 6 or tuple(w2.shape[:2]) != (1, nch) or tuple(w2.shape[3:]) != (4, 64, 8) or w2.dtype != torch.int16:
            raise ValueError("conv_s2_split: proj weights must be prepare_conv_s2's 1x1 form (1, %d, Cout/32, 4, 64, 8) int16, got %s %s"
                             % (nch, tuple(w2.shape), w2.dtype))
        if w2.shape[2] != n_ct or tuple(bias2.shape) != (Cout,):
            raise ValueError("conv_s2_split: the projection's Cout (%d, bias %s) differs from the convolution's %d"
                             % (w2.shape[2] * 32, tuple(bias2.shape), Cout))
        if out2.dtype != torch.float32 or tuple(out2.shape) != (N, Ho, Wo, Cout) or not out2.is_contiguous():
            raise ValueError("conv_s2_split: proj output must be contiguous f32 %s" % ((N, Ho, Wo, Cout),))
    x_split = _chk(x_split, torch.int16, "x_split")
    assert tuple(w.shape[3:]) == (4, 64, 8) and nch_w == nch and taps in (1, 9) and bias.shape == (Cout,)
    Hop, Wop = conv_pad_dims(Ho, Wo)
    if out_split is not None:
        assert out_split.dtype == torch.int16 and tuple(out_split.shape) == (N, Hop, Wop, Cout // 32, 64) and out_split.is_contiguous()
    if out_f32 is not None:
        assert out_f32.dtype == torch.float32 and tuple(out_f32.shape) == (N, Ho, Wo, Cout) and out_f32.is_contiguous()
    if out_fmt != ACT_BF16X2 and out_split is not None:
        assert overflow is not None and overflow.dtype == torch.int32 and overflow.device == x_split.device
    if proj is not None:
        w2, bias2, out2 = _chk(proj[0], torch.int16, "proj w2"), _chk(proj[1], torch.float32, "proj bias2"), proj[2]
        assert out2.device == x_split.device
        _lib.call("fgvc_conv_s2_split_proj_fmt_f32", _ptr(x_split), _ptr(w), _ptr(bias), _ptr(out_split), _ptr(out_f32), _ptr(w2), _ptr(bias2),
                  _ptr(out2), N, H, W, Hp, Wp, nch * 32, Cout, 3, w2.shape[2] * 32, Hop, Wop, int(relu), int(proj_relu), int(out_fmt),
                  int(out_scale_log2), _ptr(overflow), _stream(x_split))
        return
    _lib.call("fgvc_conv_s2_split_fmt_f32", _ptr(x_split), _ptr(w), _ptr(bias), _ptr(out_split), _ptr(out_f32), N, H, W, Hp, Wp,
              nch * 32, Cout, 3 if taps == 9 else 1, Hop, Wop, int(relu), int(out_fmt), int(out_scale_log2), _ptr(overflow),
              _stream(x_split))


def stem7_split(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, relu: bool = True,
                out_split: Optional[torch.Tensor] = None, out_f32: Optional[torch.Tensor] = None, out_fmt: int = ACT_BF16X2,
                out_scale_log2: int = 0, overflow: Optional[torch.Tensor] = None) -> None:
    """7x7 / stride 2 / pad 3 stem (3 -> 64 channels) + bias (+ ReLU) on the bf16 pipe (fgvc_stem7_split_fmt_f32): f32 NCHW
    frames (N, 3, H, W) -> out_f32 (N, Ho, Wo, 64) dense NHWC f32 and / or out_split (padded split NHWC in `out_fmt`: ACT_BF16X2, or
    ACT_F16F8 at scale 2^out_scale_log2 with the overflow word)."""
    x = _chk(x, torch.float32, "x")
    N, C, H, W = x.shape
    assert C == 3 and x.is_contiguous() and tuple(w.shape) == (7, 2, 2, 2, 64, 8) and bias.shape == (64,)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    Hop, Wop = conv_pad_dims(Ho, Wo)
    if out_split is not None:
        assert out_split.dtype == torch.int16 and tuple(out_split.shape) == (N, Hop, Wop, 2, 64) and out_split.is_contiguous()
    if out_f32 is not None:
        assert out_f32.dtype == torch.float32 and tuple(out_f32.shape) == (N, Ho, Wo, 64) and out_f32.is_contiguous()
    _lib.call("fgvc_stem7_split_fmt_f32", _ptr(x), _ptr(w), _ptr(bias), _ptr(out_split), _ptr(out_f32), N, H, W, Hop, Wop,
              int(relu), int(out_fmt), int(out_scale_log2), _ptr(overflow), _stream(x))


def normalize_nhwc(x: torch.Tensor, normalize: bool = True, split=False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dense NHWC f32 (N,H,W,C) -> (N, H*W, C) f32 rows, L2-normalised (the layout of normalize_to_hwc); split=True / "bf16"
    returns split_bf16() of those rows instead, split="f16" their split_f16x2(), (N, H*W, 2, C) int16, produced in the same
    single pass over x.  `out`: write there."""
    fmt = "bf16" if split is True else split
    assert fmt in (False, "bf16", "f16", "f16f6", "f16f6x")
    x = _chk(x, torch.float32, "x")
    N, H, W, C = x.shape
    shape, dt = ((N, H * W, 4 if fmt == "f16f6x" else 2, C), torch.int16) if split else ((N, H * W, C), torch.float32)
    if out is None:
        out = torch.empty(shape, device=x.device, dtype=dt)
    else:
        assert tuple(out.shape) == shape and out.dtype == dt and out.is_contiguous() and out.device == x.device
    if fmt in ("f16f6", "f16f6x"):                    # the rows of split_f16f6p() / split_f16f6x() (fgvc_pair_topk_f16f6's operands), same pass
        assert C == 256
        _lib.call(f"fgvc_normalize_split_{fmt}p_nhwc_f32" if fmt == "f16f6" else "fgvc_normalize_split_f16f6x_nhwc_f32", _ptr(x), _ptr(out), N, C, H, W,
                  int(normalize), _stream(x))
        return out
    _lib.call("fgvc_normalize_split_f16x2_nhwc_f32" if fmt == "f16" else "fgvc_normalize_split_nhwc_f32", _ptr(x),
              _ptr(None if split else out), _ptr(out if split else None), N, C, H, W, int(normalize), _stream(x))
    return out


def unsplit_f16x2(split: torch.Tensor) -> torch.Tensor:
    """(…, 2, C) int16 split_f16x2() features -> (…, C) f32 = (h + l) / 2^14 (2^-22-relative approximation of the rows)."""
    v = split.view(torch.float16).float()
    return (v[..., 0, :] + v[..., 1, :]) * (1.0 / 16384.0)


def unsplit_act(split: torch.Tensor, fmt: int, scale_log2: int = 0) -> torch.Tensor:
    """A padded split NHWC activation tensor (N, Hp, Wp, C/32, 64) int16 in format `fmt` -> (N, Hp, Wp, C) f32 (tests, calibration)."""
    n5 = split.shape
    if fmt == ACT_BF16X2:
        v = split.view(torch.bfloat16).float()
        return (v[..., :32] + v[..., 32:]).reshape(*n5[:3], -1)
    b = split.contiguous().view(torch.uint8).reshape(*n5[:4], 128)
    h = b[..., :64].contiguous().view(torch.float16).float()
    if fmt == ACT_F16X2:
        l = b[..., 64:].contiguous().view(torch.float16).float()
    elif fmt == ACT_F16F6:       # slots 4 / 6: the residual's FP6 block (main, tail + scale byte)
        l = _e2m3_decode(torch.cat([b[..., 64:80], b[..., 96:104]], dim=-1), b[..., 104])
    else:
        l = b[..., 64:96].contiguous().view(torch.float8_e4m3fn).float() * 2.0 ** -F8_BX
    return ((h + l) * 2.0 ** -scale_log2).reshape(*n5[:3], -1)


def unsplit_bf16(split: torch.Tensor) -> torch.Tensor:
    """(…, 2, C) int16 split features -> (…, C) f32 = hi + lo (2^-17-relative approximation of the rows that were split)."""
    v = split.view(torch.bfloat16).float()
    return v[..., 0, :] + v[..., 1, :]


def gaussian_labels(points: torch.Tensor, Hf: int, Wf: int, stride: int, sigma: float = 6.0,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """points (P,2)=(x,y) -> (HfWf, P) initial labels (vanilla_tracker.py:204-221)."""
    points = _chk(points.to(torch.float32), torch.float32, "points")
    P = points.shape[0]
    if out is None:
        out = torch.empty((Hf * Wf, P), device=points.device, dtype=torch.float32)
    _lib.call("fgvc_gaussian_labels_f32", _ptr(points), P, Hf, Wf, stride, float(sigma), _ptr(out), _stream(points))
    return out


def softargmax_top5(labels: torch.Tensor, Hf: int, Wf: int, h: int, w: int,
                    gauss_points: Optional[torch.Tensor] = None, sigma: float = 6.0) -> torch.Tensor:
    """labels (n_frames, HfWf, P) -> coords (n_frames, P, 2) float64 = (x, y)."""
    labels = _chk(labels, torch.float32, "labels")
    n, P = labels.shape[0], labels.shape[2]
    assert labels.shape[1] == Hf * Wf
    if gauss_points is not None:
        gauss_points = _chk(gauss_points.to(torch.float32), torch.float32, "gauss_points")
        assert gauss_points.shape == (P, 2)
    coords = torch.empty((n, P, 2), device=labels.device, dtype=torch.float64)
    ws_bytes = _lib.load().fgvc_softargmax_workspace_bytes(n, P)
    ws = torch.empty((max(ws_bytes, 4) + 3) // 4, device=labels.device, dtype=torch.float32)
    _lib.call("fgvc_softargmax_top5_f32", _ptr(labels), n, Hf, Wf, P, h, w, _ptr(gauss_points), float(sigma),
              _ptr(coords), _ptr(ws), _stream(labels))
    return coords


# ---- segmentation masks (semi-supervised VOS, vanilla_tracker.py:663-830) ------------------------------------------------------------

def pil_nearest_index(n_in: int, n_out: int) -> torch.Tensor:
    """Source rows (or columns) of Pillow's NEAREST resize from n_in to n_out (pil_nearest_interpolate, common/utils.py:39), as
    fgvc_seg_*_u8 compute them: a running double sum of in/out starting at half a step, truncated, clamped to n_in - 1.  (Not
    floor((o + 0.5) * in / out): at 100 -> 27 the two differ where the exact value is an integer.)"""
    a, xo, out = n_in / n_out, n_in / n_out * 0.5, []
    for _ in range(n_out):
        out.append(min(int(xo), n_in - 1))
        xo += a
    return torch.tensor(out, dtype=torch.int64)


def seg_max_label(seg_map: torch.Tensor, Hf: int, Wf: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """seg_map (hp, wp) uint8 -> (1,) int32 on the device: the largest id of the map sampled to (Hf, Wf) by Pillow's NEAREST rule."""
    seg_map = _chk(seg_map, torch.uint8, "seg_map")
    hp, wp = seg_map.shape
    if out is None:
        out = torch.empty((1,), device=seg_map.device, dtype=torch.int32)
    _lib.call("fgvc_seg_max_label_u8", _ptr(seg_map), hp, wp, Hf, Wf, _ptr(out), _stream(seg_map))
    return out


def seg_onehot_labels(seg_map: torch.Tensor, Hf: int, Wf: int, C: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """seg_map (hp, wp) uint8 -> (HfWf, C) f32 = one_hot(pil_nearest(seg_map, (Hf, Wf)), C) (vanilla_tracker.py:700-707)."""
    seg_map = _chk(seg_map, torch.uint8, "seg_map")
    hp, wp = seg_map.shape
    if out is None:
        out = torch.empty((Hf * Wf, C), device=seg_map.device, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.shape == (Hf * Wf, C) and out.dtype == torch.float32
    _lib.call("fgvc_seg_onehot_labels_u8", _ptr(seg_map), hp, wp, Hf, Wf, C, _ptr(out), _stream(seg_map))
    return out


def seg_hard_onehot(labels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels (..., C) f32 -> one_hot(argmax over C) (vanilla_tracker.py:767-769); the first maximum wins.  `out` may be `labels`."""
    labels = _chk(labels, torch.float32, "labels")
    C = labels.shape[-1]
    if out is None:
        out = torch.empty_like(labels)
    else:
        assert out.is_contiguous() and out.shape == labels.shape and out.dtype == torch.float32
    _lib.call("fgvc_seg_hard_onehot_f32", _ptr(labels), labels.numel() // C, C, _ptr(out), _stream(labels))
    return out


def seg_readout(labels: torch.Tensor, Hf: int, Wf: int, pad_shape: Tuple[int, int], pad: Tuple[int, int, int, int],
                out_shape: Tuple[int, int], norm: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """labels (n, HfWf, C) f32 -> masks (n, h0, w0) uint8 (vanilla_tracker.py:773-802): bilinear to pad_shape (hp, wp), unpad by
    pad = (left, right, top, bottom) (pad_divide_by's order), bilinear to out_shape (h0, w0), per-channel min-max normalisation where the
    maximum is > 0 (norm), argmax over C.  Evaluated per output pixel from the feature grid: no (C, hp, wp) map."""
    labels = _chk(labels, torch.float32, "labels")
    n, C = labels.shape[0], labels.shape[2]
    assert labels.shape[1] == Hf * Wf
    (hp, wp), (lw, uw, lh, uh), (h0, w0) = pad_shape, pad, out_shape
    if out is None:
        out = torch.empty((n, h0, w0), device=labels.device, dtype=torch.uint8)
    else:
        assert out.is_contiguous() and out.shape == (n, h0, w0) and out.dtype == torch.uint8
    ws = torch.empty((max(_lib.load().fgvc_seg_readout_workspace_bytes(n, C), 4) + 3) // 4, device=labels.device, dtype=torch.float32)
    _lib.call("fgvc_seg_readout_u8", _ptr(labels), n, Hf, Wf, C, hp, wp, lh, lw, hp - lh - uh, wp - lw - uw, h0, w0, int(bool(norm)),
              _ptr(out), _ptr(ws), _stream(labels))
    return out


def seg_label_set(seg_map: torch.Tensor, Hf: int, Wf: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """seg_map (hp, wp) uint8 -> (8,) int32 on the device: the 256-bit set of the ids present in the map sampled to (Hf, Wf) by Pillow's
    NEAREST rule (bit id % 32 of word id // 32; label_set_ids turns a host copy into a list)."""
    seg_map = _chk(seg_map, torch.uint8, "seg_map")
    hp, wp = seg_map.shape
    if out is None:
        out = torch.empty((8,), device=seg_map.device, dtype=torch.int32)
    else:
        assert out.is_contiguous() and out.shape == (8,) and out.dtype == torch.int32
    _lib.call("fgvc_seg_label_set_u8", _ptr(seg_map), hp, wp, Hf, Wf, _ptr(out), _stream(seg_map))
    return out


def label_set_ids(words) -> List[int]:
    """The ids of a 256-bit set given as 8 int32 / uint32 words (a host tensor or a sequence), ascending."""
    ws = [int(w) & 0xFFFFFFFF for w in (words.tolist() if hasattr(words, "tolist") else words)]
    return [32 * j + b for j, w in enumerate(ws) for b in range(32) if (w >> b) & 1]


def label_set_words(ids) -> torch.Tensor:
    """ids (each 0..255) -> the (8,) int32 host tensor of their 256-bit set (label_set_ids' inverse)."""
    ws = [0] * 8
    for i in ids:
        if not 0 <= int(i) <= 255:
            raise ValueError(f"label_set_words: id {i} outside 0..255")
        ws[int(i) >> 5] |= 1 << (int(i) & 31)
    return torch.tensor([w - (1 << 32) if w >= (1 << 31) else w for w in ws], dtype=torch.int32)


def seg_inject_labels(seg_map: torch.Tensor, Hf: int, Wf: int, C: int, ids: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """rows (HfWf, C) f32, written in place: every cell whose id in pil_nearest(seg_map, (Hf, Wf)) is in the set `ids` ((8,) int32 on the
    device, seg_label_set's layout) becomes one_hot(id, C); every other cell keeps its row.  Returns rows."""
    seg_map = _chk(seg_map, torch.uint8, "seg_map")
    ids = _chk(ids, torch.int32, "ids")
    hp, wp = seg_map.shape
    if not rows.is_cuda:
        raise _lib.FgvcHipError("rows must be on the GPU (fgvc_amd has no CPU path)")
    assert ids.shape == (8,) and rows.is_contiguous() and rows.shape == (Hf * Wf, C) and rows.dtype == torch.float32
    _lib.call("fgvc_seg_inject_labels_u8", _ptr(seg_map), hp, wp, Hf, Wf, C, _ptr(ids), _ptr(rows), _stream(seg_map))
    return rows


def seg_readout_conf(labels: torch.Tensor, Hf: int, Wf: int, pad_shape: Tuple[int, int], pad: Tuple[int, int, int, int],
                     out_shape: Tuple[int, int], norm: bool = True, out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None):
    """seg_readout with the confidence of every pixel: (masks (n, h0, w0) uint8 -- seg_readout's bytes --, conf (n, h0, w0) uint8 =
    rint(255 * clamp(best - second, 0, 1)) of the two largest (normalised) channel values, 255 where C == 1, stats (n, C, 2) int64 = per
    frame and id the pixel count and the sum of that id's conf bytes).  `out` = (masks, conf) to write into."""
    labels = _chk(labels, torch.float32, "labels")
    n, C = labels.shape[0], labels.shape[2]
    assert labels.shape[1] == Hf * Wf
    (hp, wp), (lw, uw, lh, uh), (h0, w0) = pad_shape, pad, out_shape
    if out is None:
        out = (torch.empty((n, h0, w0), device=labels.device, dtype=torch.uint8), torch.empty((n, h0, w0), device=labels.device, dtype=torch.uint8))
    masks, conf = out
    for t in (masks, conf):
        assert t.is_cuda and t.is_contiguous() and t.shape == (n, h0, w0) and t.dtype == torch.uint8
    stats = torch.empty((n, C, 2), device=labels.device, dtype=torch.int64)
    ws = torch.empty((max(_lib.load().fgvc_seg_readout_workspace_bytes(n, C), 4) + 3) // 4, device=labels.device, dtype=torch.float32)
    _lib.call("fgvc_seg_readout_conf_u8", _ptr(labels), n, Hf, Wf, C, hp, wp, lh, lw, hp - lh - uh, wp - lw - uw, h0, w0, int(bool(norm)),
              _ptr(masks), _ptr(conf), _ptr(stats), _ptr(ws), _stream(labels))
    return masks, conf, stats


# ---- edge-aware read-out (test_cfg.readout = dict(type='guided'); engine.guided_readout_host is the rule in float64) ---------------------

def guide_cells(frames: torch.Tensor, Hf: int, Wf: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames (n, 3, hp, wp) f32, the padded Lab-normalised frames -> (n, HfWf, 3) f32: the mean colour of every cell's (hp / Hf) x
    (wp / Wf) pixel block.  (Hf, Wf) must divide (hp, wp)."""
    frames = _chk(frames, torch.float32, "frames")
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise ValueError(f"frames: (n, 3, hp, wp), got {tuple(frames.shape)}")
    n, _, hp, wp = frames.shape
    if out is None:
        out = torch.empty((n, Hf * Wf, 3), device=frames.device, dtype=torch.float32)
    else:
        assert out.is_cuda and out.is_contiguous() and out.shape == (n, Hf * Wf, 3) and out.dtype == torch.float32
    _lib.call("fgvc_guide_cells_f32", _ptr(frames), n, hp, wp, Hf, Wf, _ptr(out), _stream(frames))
    return out


def seg_readout_guided(labels: torch.Tensor, guide: torch.Tensor, Hf: int, Wf: int, pad_shape: Tuple[int, int],
                       pad: Tuple[int, int, int, int], out_shape: Tuple[int, int], norm: bool = True, radius: int = 2,
                       sigma_space: float = 1.0, sigma_range: float = 0.1, conf: bool = False, out=None,
                       cells: Optional[torch.Tensor] = None):
    """The edge-aware read-out: labels (n, HfWf, C) f32 and guide (n, 3, hp, wp) f32 (the padded frames the encoder read, finite) ->
    masks (n, h0, w0) uint8; conf=True: (masks, conf (n, h0, w0) uint8, stats (n, C, 2) int64) as seg_readout_conf defines them.  Every
    output pixel is a joint bilateral combination of the (2 radius + 1)^2 cells around it (engine.guided_readout_host states the rule);
    pad_shape, pad, out_shape and norm as seg_readout takes them, except that norm's extremes are those of the feature grid.
    `out`: masks, or (masks, conf), to write into.  `cells`: guide_cells(guide, Hf, Wf) where the caller already has it."""
    labels = _chk(labels, torch.float32, "labels")
    guide = _chk(guide, torch.float32, "guide")
    n, C = labels.shape[0], labels.shape[2]
    assert labels.shape[1] == Hf * Wf
    (hp, wp), (lw, uw, lh, uh), (h0, w0) = pad_shape, pad, out_shape
    if tuple(guide.shape) != (n, 3, hp, wp):
        raise ValueError(f"guide: ({n}, 3, {hp}, {wp}) to go with the labels and pad_shape, got {tuple(guide.shape)}")
    dev = labels.device
    if cells is None:
        cells = guide_cells(guide, Hf, Wf)
    else:
        cells = _chk(cells, torch.float32, "cells")
        if tuple(cells.shape) != (n, Hf * Wf, 3):
            raise ValueError(f"cells: ({n}, {Hf * Wf}, 3), got {tuple(cells.shape)}")
    outs = (out,) if torch.is_tensor(out) else (tuple(out) if out is not None else ())
    if len(outs) not in (0, 2 if conf else 1):
        raise ValueError("out: masks, or (masks, conf) with conf=True")
    outs = outs or tuple(torch.empty((n, h0, w0), device=dev, dtype=torch.uint8) for _ in range(2 if conf else 1))
    for t in outs:
        assert t.is_cuda and t.is_contiguous() and t.shape == (n, h0, w0) and t.dtype == torch.uint8
    ws = torch.empty((max(_lib.load().fgvc_seg_readout_guided_workspace_bytes(n, C), 4) + 3) // 4, device=dev, dtype=torch.int32)
    head = (_ptr(labels), _ptr(guide), _ptr(cells), n, Hf, Wf, C, hp, wp, lh, lw, hp - lh - uh, wp - lw - uw, h0, w0, int(bool(norm)),
            int(radius), float(sigma_space), float(sigma_range))
    if not conf:
        _lib.call("fgvc_seg_readout_guided_u8", *head, _ptr(outs[0]), _ptr(ws), _stream(labels))
        return outs[0]
    stats = torch.empty((n, C, 2), device=dev, dtype=torch.int64)
    _lib.call("fgvc_seg_readout_guided_conf_u8", *head, _ptr(outs[0]), _ptr(outs[1]), _ptr(stats), _ptr(ws), _stream(labels))
    return outs[0], outs[1], stats


# ---- forward and backward sweeps fused between annotated frames (test_cfg.refs fuse='linear'; engine.fuse_refs_host is the rule) ----------

def _same_storage(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()


def seg_fuse_rows(fw: torch.Tensor, bw: torch.Tensor, fw_index, bw_index, weights, out: Optional[torch.Tensor] = None, out_index=None,
                  counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """One launch for len(weights) items.  fw (n_fw, HW, C), bw (n_bw, HW, C) f32 stacks of row blocks on one device; fw_index, bw_index,
    out_index: per item a frame index into fw, bw and out (host integers); weights: per item a host number w, 0 <= w <= 1, rounded to
    f32.  Item i writes out[out_index[i]] = w fw[fw_index[i]] + (1 - w) bw[bw_index[i]] (fma(w, x, fl(fl(1 - w) y)) in f32) and
    counts[i] = the number of cells whose forward and backward rows have different arg-maxima over C (the first maximum wins).  The
    rows are assumed finite: nothing is promised for a row that holds a NaN (include/fgvc_hip.h).
    out=None: fw itself, in place, with out_index = fw_index; a separate out (n_out, HW, C) must share memory with neither stack, and the
    out indices must differ from each other.  counts: an (n_items,) int64 device tensor to write into.  Returns (out, counts).
    Every refusal (TypeError for a dtype, ValueError for the rest) comes before the launch; nothing is copied except the 16-byte item
    records."""
    for name, t in (("fw", fw), ("bw", bw)) + ((("out", out),) if out is not None else ()):
        if not torch.is_tensor(t):
            raise TypeError(f"seg_fuse_rows: {name}: a tensor, got {type(t).__name__}")
        if t.dtype != torch.float32:
            raise TypeError(f"seg_fuse_rows: {name}: expected torch.float32, got {t.dtype}")
        if t.dim() != 3 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError(f"seg_fuse_rows: {name}: a stack (n, HW, C), got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"seg_fuse_rows: {name} is not contiguous (the kernel addresses the stacks in place; no copy is made)")
    HW, C = int(fw.shape[1]), int(fw.shape[2])
    if not 1 <= C <= 256:
        raise ValueError(f"seg_fuse_rows: C={C} (1 <= C <= 256)")
    if tuple(bw.shape[1:]) != (HW, C) or bw.device != fw.device:
        raise ValueError(f"seg_fuse_rows: bw {tuple(bw.shape)} on {bw.device} against fw's (n, {HW}, {C}) on {fw.device}")
    in_place = out is None or (out.data_ptr() == fw.data_ptr() and out.shape == fw.shape)
    if out is None:
        out, out_index = fw, (fw_index if out_index is None else out_index)
    elif tuple(out.shape[1:]) != (HW, C) or out.device != fw.device:
        raise ValueError(f"seg_fuse_rows: out {tuple(out.shape)} on {out.device} against fw's (n, {HW}, {C}) on {fw.device}")
    if out_index is None:
        raise ValueError("seg_fuse_rows: out_index is needed with out=")
    cols = [list(fw_index), list(bw_index), list(out_index), list(weights)]
    n = len(cols[3])
    if not 1 <= n <= 65535 or any(len(c) != n for c in cols):
        raise ValueError(f"seg_fuse_rows: {[len(c) for c in cols]} fw / bw / out indices and weights (1 .. 65535 items, one of each per item)")
    for name, col, size in (("fw_index", cols[0], fw.shape[0]), ("bw_index", cols[1], bw.shape[0]), ("out_index", cols[2], out.shape[0])):
        for v in col:
            if isinstance(v, bool) or int(v) != v or not 0 <= int(v) < size:
                raise ValueError(f"seg_fuse_rows: {name} {v!r} outside the stack's {size} frames")
    for i, w in enumerate(cols[3]):
        try:                                                               # any real number: a Python, numpy or 0-d tensor scalar
            v = None if isinstance(w, (bool, str, bytes)) else float(w)
        except (TypeError, ValueError):
            v = None
        if v is None or not 0.0 <= v <= 1.0:                               # NaN fails the comparison too
            raise ValueError(f"seg_fuse_rows: weight {w!r} (a number, 0 <= w <= 1)")
        cols[3][i] = v
    if len(set(int(v) for v in cols[2])) != n:
        raise ValueError(f"seg_fuse_rows: out_index {cols[2]} names a block twice")
    if in_place:
        if [int(v) for v in cols[2]] != [int(v) for v in cols[0]]:
            raise ValueError("seg_fuse_rows: out is fw: every item must write the block it reads (out_index == fw_index)")
    elif _same_storage(out, fw):
        raise ValueError("seg_fuse_rows: out shares memory with fw without being fw (pass out=None to write in place)")
    if _same_storage(out, bw):
        raise ValueError("seg_fuse_rows: out shares memory with bw")
    if not fw.is_cuda:                                                     # the argument checks above need no device; the launch does
        raise _lib.FgvcHipError("seg_fuse_rows: the stacks must be on the GPU (fgvc_amd has no CPU path)")
    if counts is None:
        counts = torch.empty((n,), device=fw.device, dtype=torch.int64)
    elif not (torch.is_tensor(counts) and counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and counts.shape == (n,)):
        raise ValueError(f"seg_fuse_rows: counts: a contiguous ({n},) int64 device tensor")
    bits = struct.unpack(f"<{n}i", struct.pack(f"<{n}f", *(float(w) for w in cols[3])))
    items = torch.tensor([[int(a), int(b), int(o), wb] for a, b, o, wb in zip(cols[0], cols[1], cols[2], bits)],
                         dtype=torch.int32).to(fw.device)
    _lib.call("fgvc_seg_fuse_rows_f32", _ptr(fw), _ptr(bw), _ptr(out), _ptr(items), n, fw.shape[0], bw.shape[0], out.shape[0], HW, C,
              _ptr(counts), _stream(fw))
    return out, counts


# ---- soft first-frame labels read out as joint coordinates (JHMDB / BADJA heat maps, vanilla_tracker.py:663-830 with coords=True) ----

def _heat(heat: torch.Tensor) -> torch.Tensor:
    if not heat.is_cuda:
        raise _lib.FgvcHipError("heat must be on the GPU (fgvc_amd has no CPU path)")
    if heat.dtype not in (torch.float32, torch.float64) or heat.dim() != 3:
        raise TypeError(f"heat: expected a (K, h, w) float32 or float64 map, got {tuple(heat.shape)} {heat.dtype}")
    return heat.contiguous()


def seg_soft_labels(heat: torch.Tensor, pad: Tuple[int, int, int, int], Hf: int, Wf: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """heat (K, hm, wm) f32 | f64, the map before its own padding pad = (left, right, top, bottom) -> (HfWf, K) f32 =
    F.interpolate(F.pad(heat, pad), (Hf, Wf), bilinear).float() computed in heat's dtype (vanilla_tracker.py:706-711)."""
    heat = _heat(heat)
    K, hm, wm = heat.shape
    lw, uw, lh, uh = pad
    if out is None:
        out = torch.empty((Hf * Wf, K), device=heat.device, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.shape == (Hf * Wf, K) and out.dtype == torch.float32
    name = "fgvc_seg_soft_labels_f64" if heat.dtype == torch.float64 else "fgvc_seg_soft_labels_f32"
    _lib.call(name, _ptr(heat), K, hm, wm, hm + lh + uh, wm + lw + uw, lh, lw, Hf, Wf, _ptr(out), _stream(heat))
    return out


def heatmap_coords(bank: torch.Tensor, heat: torch.Tensor, Hf: int, Wf: int, pad: Tuple[int, int, int, int],
                   out_shape: Tuple[int, int], f64_arith: Optional[bool] = None, out: Optional[torch.Tensor] = None, peak: bool = False):
    """img2coord of the T frames the reference stacks (vanilla_tracker.py:712-716, :770-784, :803, :814-818) -> (2, K, T) f64.
    Frame 0 = bilinear(F.pad(heat, pad) -> out_shape) in heat's dtype, not unpadded; frame f >= 1 = bilinear to the padded size, unpad,
    bilinear to out_shape, in f32, from bank[f] (T, HfWf, K) f32 (bank[0] is not read).  The top-5 normalisation runs in f64 when
    `f64_arith` (default: heat is float64, as np.stack makes it), else in f32.  No (K, h0, w0) map is built.
    peak=True: (coords, peak (K, T) f64) from fgvc_heatmap_coords_peak_f32: the same coordinates, and every map's largest value, the
    softmap_readout(...).amax((2, 3)) of that map (frame 0 in heat's dtype, later frames f32, widened)."""
    heat = _heat(heat)
    bank = _chk(bank, torch.float32, "bank")
    K, hm, wm = heat.shape
    T = bank.shape[0]
    assert bank.shape[1:] == (Hf * Wf, K), (tuple(bank.shape), Hf, Wf, K)
    lw, uw, lh, uh = pad
    h0, w0 = out_shape
    if f64_arith is None:
        f64_arith = heat.dtype == torch.float64
    if out is None:
        out = torch.empty((2, K, T), device=heat.device, dtype=torch.float64)
    else:
        assert out.is_contiguous() and out.shape == (2, K, T) and out.dtype == torch.float64
    ws = torch.empty((max(_lib.load().fgvc_heatmap_coords_workspace_bytes(T, K), 8) + 7) // 8, device=heat.device, dtype=torch.float64)
    head = (_ptr(bank), _ptr(heat), int(heat.dtype == torch.float64), T, Hf, Wf, K, hm, wm, hm + lh + uh, wm + lw + uw, lh, lw, h0, w0,
            int(bool(f64_arith)), _ptr(out))
    if not peak:
        _lib.call("fgvc_heatmap_coords_f32", *head, _ptr(ws), _stream(heat))
        return out
    pk = torch.empty((K, T), device=heat.device, dtype=torch.float64)
    if T > 0:
        _lib.call("fgvc_heatmap_coords_peak_f32", *head, _ptr(pk), _ptr(ws), _stream(heat))
    return out, pk


def softmap_readout(bank: Optional[torch.Tensor], heat: torch.Tensor, Hf: int, Wf: int, pad: Tuple[int, int, int, int],
                    out_shape: Tuple[int, int], frames: Optional[Tuple[int, int]] = None, out_dtype: Optional[torch.dtype] = None,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Frames [f_begin, f_end) of the stack the reference returns without `coords` (vanilla_tracker.py:770-784, :800-803) ->
    (f_end - f_begin, K, h0, w0): the maps heatmap_coords reads its five values from, written out, bit for bit.  Arguments as
    heatmap_coords'; `frames` defaults to all T of the bank; `out_dtype` float64 | float32 defaults to heat's dtype (np.stack's): frames
    >= 1 are f32 values (widened for a float64 result), frame 0 is computed in heat's dtype and rounded once for a float32 result.
    `bank` may be None when only frame 0 is asked for."""
    heat = _heat(heat)
    K, hm, wm = heat.shape
    if bank is not None:
        bank = _chk(bank, torch.float32, "bank")
        assert bank.shape[1:] == (Hf * Wf, K), (tuple(bank.shape), Hf, Wf, K)
    T = bank.shape[0] if bank is not None else 1
    f_begin, f_end = (0, T) if frames is None else (int(frames[0]), int(frames[1]))
    lw, uw, lh, uh = pad
    h0, w0 = out_shape
    if out_dtype is None:
        out_dtype = out.dtype if out is not None else heat.dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise TypeError(f"out_dtype: float32 or float64, got {out_dtype}")
    shape = (max(f_end - f_begin, 0), K, h0, w0)
    if out is None:
        out = torch.empty(shape, device=heat.device, dtype=out_dtype)
    else:
        assert out.is_contiguous() and tuple(out.shape) == shape and out.dtype == out_dtype and out.device == heat.device
    _lib.call("fgvc_softmap_readout_f32", _ptr(bank), _ptr(heat), int(heat.dtype == torch.float64), T, Hf, Wf, K, hm, wm,
              hm + lh + uh, wm + lw + uw, lh, lw, h0, w0, f_begin, f_end, int(out_dtype == torch.float64), _ptr(out), _stream(heat))
    return out


# ---- the input stage: decoded uint8 RGB frames -> the network's Lab-normalised planar input -------------------

INPUT_LAYOUTS = ("thwc", "tchw")


def _out(out: Optional[torch.Tensor], shape, dtype, device) -> torch.Tensor:
    """A fresh tensor, or the caller's `out` where it is a contiguous one of that shape, dtype and device."""
    if out is None:
        return torch.empty(shape, device=device, dtype=dtype)
    if tuple(out.shape) != tuple(shape) or out.dtype != dtype or out.device != device or not out.is_contiguous():
        raise ValueError(f"out: a contiguous {str(dtype)[6:]} tensor of shape {tuple(shape)} on {device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    return out


def _lab_out(T: int, h0: int, w0: int, size, pad, out, device):
    """`size`, `pad`, `out` of the Lab calls -> (h, w, (left, right, top, bottom), the (T, 3, hp, wp) f32 tensor to write)."""
    h, w = (h0, w0) if size is None else (int(size[0]), int(size[1]))
    left, right, top, bottom = (int(p) for p in pad)
    return h, w, (left, right, top, bottom), _out(out, (T, 3, top + h + bottom, left + w + right), torch.float32, device)


def frames_to_lab(frames_u8: torch.Tensor, size: Optional[Tuple[int, int]] = None, pad: Tuple[int, int, int, int] = (0, 0, 0, 0),
                  layout: str = "thwc", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """uint8 RGB frames (T, h0, w0, 3) ('thwc') or (T, 3, h0, w0) ('tchw') -> (T, 3, hp, wp) f32: per frame exactly
    datasets.preprocess_tapvid_frames (bilinear resize to `size` = (h, w), None = the frames' own; / 255; RGB -> Lab; (x - [50, 0, 0]) /
    [50, 127, 127]) at (top, left) of a border of exact zeros, pad = (left, right, top, bottom) as engine.pad_divide_by returns it
    (F.pad's order) -- one launch of fgvc_frames_rgb8_to_lab_f32.  The frames are read through their own strides: a view (a crop, a
    permuted tensor, a time slice) is not copied.  `out`: a contiguous (T, 3, hp, wp) f32 tensor on the frames' device to write into."""
    if layout not in INPUT_LAYOUTS:
        raise ValueError(f"layout={layout!r}: one of {INPUT_LAYOUTS}")
    if not frames_u8.is_cuda:
        raise _lib.FgvcHipError("frames_u8 must be on the GPU (fgvc_amd has no CPU path)")
    if frames_u8.dtype != torch.uint8:
        raise TypeError(f"frames_u8: expected torch.uint8, got {frames_u8.dtype}")
    if frames_u8.dim() != 4:
        raise ValueError(f"frames_u8: 4 dimensions ({'T, h0, w0, 3' if layout == 'thwc' else 'T, 3, h0, w0'}), got {tuple(frames_u8.shape)}")
    f = frames_u8 if layout == "thwc" else frames_u8.permute(0, 2, 3, 1)              # (T, h0, w0, 3) view either way
    T, h0, w0, ch = f.shape
    if ch != 3:
        raise ValueError(f"frames_u8: 3 channels (RGB) in layout {layout!r}, got {ch} (shape {tuple(frames_u8.shape)})")
    h, w, pad, out = _lab_out(T, h0, w0, size, pad, out, f.device)
    if T == 0:
        return out
    st, sy, sx, sc = f.stride()                                                       # (uint8: elements are bytes)
    _lib.call("fgvc_frames_rgb8_to_lab_f32", _ptr(f), T, h0, w0, st, sy, sx, sc, h, w, *pad, _ptr(out), _stream(f))
    return out


# ---- the input stage for Y'CbCr video: planes -> the network input, or RGB bytes (DESIGN.md sections 19 and 26) ---------------------------
# Two families of entries over one checker and one splitter: yuv_frames_* take 8-bit 4:2:0 planes (YUV_FORMATS) to the fixed-format
# kernels of fgvc_frames_yuv420_*; yuv_planes_* take 8..16 bits, 4:2:0 / 4:2:2 / 4:4:4 (YUV_PIXEL_FORMATS) to fgvc_frames_yuvp_*.

YUV_FORMATS = ("nv12", "i420")
YUV_MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}       # (Kr, Kb)
YUV_RANGES = {"limited": (16.0, 255.0 / 219.0, 255.0 / 224.0), "full": (0.0, 1.0, 1.0)}    # (y_off, cy, sc) at 8 bits
YUV_SITINGS = ("left", "center")                                            # = FGVC_YUV_SITING_LEFT, FGVC_YUV_SITING_CENTER

# ffmpeg's name -> (layout 'planar' | 'semi', sub_x, sub_y, depth, shift, dtype); 16-bit samples are host-endian (little-endian) words.
# 'nv12' and 'i420' stay in YUV_FORMATS and go through the 8-bit 4:2:0 entries.
YUV_PIXEL_FORMATS = {
    "p010": ("semi", 2, 2, 10, 6, torch.uint16), "p012": ("semi", 2, 2, 12, 4, torch.uint16), "p016": ("semi", 2, 2, 16, 0, torch.uint16),
    "yuv420p10": ("planar", 2, 2, 10, 0, torch.uint16), "yuv420p12": ("planar", 2, 2, 12, 0, torch.uint16),
    "yuv422p10": ("planar", 2, 1, 10, 0, torch.uint16), "yuv422p12": ("planar", 2, 1, 12, 0, torch.uint16),
    "yuv444p10": ("planar", 1, 1, 10, 0, torch.uint16), "yuv444p12": ("planar", 1, 1, 12, 0, torch.uint16),
    "yuv422p": ("planar", 2, 1, 8, 0, torch.uint8), "yuv444p": ("planar", 1, 1, 8, 0, torch.uint8),
    "nv16": ("semi", 2, 1, 8, 0, torch.uint8),
}
_YUV420_FORMATS = {"nv12": ("semi", 2, 2, 8, 0, torch.uint8), "i420": ("planar", 2, 2, 8, 0, torch.uint8)}     # YUV_FORMATS in that table's words
_YUV_DTYPES = (torch.uint8, torch.uint16)


def yuv_coefficients_depth(matrix: str = "bt601", range: str = "limited",
                           depth: int = 8) -> Tuple[float, float, float, float, float, float, float]:
    """(y_off, cy, c_off, crv, cgu, cgv, cbu) of R = yy + crv cr, G = (yy + cgu cb) + cgv cr, B = yy + cbu cb with yy = cy (Y - y_off),
    cb = U - c_off, cr = V - c_off for samples of `depth` bits (8..16), R'G'B' on the 0..255 scale: from Kr, Kb of `matrix` ('bt601' |
    'bt709') and, with s = 2^(depth - 8), 'limited' y_off = 16 s, cy = 255 / (219 s), c_off = 128 s, chroma scale 255 / (224 s); 'full'
    y_off = 0, cy = 255 / (2^depth - 1), c_off = 2^(depth - 1), chroma scale 255 / (2^depth - 1).  Computed in float64 as Python floats; the
    kernels take them rounded to f32 once.  The limited-range ones at any depth differ from the 8-bit ones by powers of two."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix={matrix!r}: one of {tuple(YUV_MATRICES)}")
    if range not in YUV_RANGES:
        raise ValueError(f"range={range!r}: one of {tuple(YUV_RANGES)}")
    depth = int(depth)
    if not 8 <= depth <= 16:
        raise ValueError(f"depth={depth}: 8..16")
    kr, kb = YUV_MATRICES[matrix]
    kg = 1.0 - kr - kb
    s = float(1 << (depth - 8))
    if range == "limited":
        y_off, cy, c_off, sc = 16.0 * s, 255.0 / (219.0 * s), 128.0 * s, 255.0 / (224.0 * s)
    else:
        top = float((1 << depth) - 1)
        y_off, cy, c_off, sc = 0.0, 255.0 / top, float(1 << (depth - 1)), 255.0 / top
    return (y_off, cy, c_off, 2.0 * (1.0 - kr) * sc, -2.0 * kb * (1.0 - kb) / kg * sc, -2.0 * kr * (1.0 - kr) / kg * sc, 2.0 * (1.0 - kb) * sc)


def yuv_coefficients(matrix: str = "bt601", range: str = "limited") -> Tuple[float, float, float, float, float, float]:
    """(y_off, cy, crv, cgu, cgv, cbu): yuv_coefficients_depth at 8 bits without its c_off = 128, what the 8-bit 4:2:0 entries take."""
    c = yuv_coefficients_depth(matrix, range, 8)
    return c[:2] + c[3:]


def yuv_packed_rows(fmt: str, h0: int) -> int:
    """Rows of a packed `fmt` frame of h0 luma rows: h0 (1 + 2 / (sub_x sub_y))."""
    _, sx, sy = YUV_PIXEL_FORMATS[fmt][:3]
    return h0 + 2 * h0 // (sx * sy)


def _packed_height(rows: int, k: int) -> int:
    return rows * k // (k + 2) if rows * k % (k + 2) == 0 else -1


def yuv_packed_height(fmt: str, rows: int) -> int:
    """The luma rows h0 of a packed `fmt` frame of `rows` rows (3 h0 / 2, 2 h0 or 3 h0 rows), or -1 where no whole h0 gives them."""
    _, sx, sy = YUV_PIXEL_FORMATS[fmt][:3]
    return _packed_height(rows, sx * sy)


def _packed_shape(fmt: str) -> str:
    _, sx, sy = (_YUV420_FORMATS.get(fmt) or YUV_PIXEL_FORMATS[fmt])[:3]
    return {4: "(T, 3 h0 / 2, w0)", 2: "(T, 2 h0, w0)", 1: "(T, 3 h0, w0)"}[sx * sy]


def _split_planes(frames: torch.Tensor, fmt: str, layout: str, sx: int, sy: int):
    """Packed frames (T, rows, w0) -> the views (y, u, v): what yuv420_planes and yuv_planes share."""
    shape = _packed_shape(fmt)
    if frames.dim() != 3:
        raise ValueError(f"frames: packed {fmt} frames of shape {shape}, got {tuple(frames.shape)}")
    T, rows, w0 = frames.shape
    h0 = _packed_height(rows, sx * sy)
    if h0 <= 0 or w0 == 0 or h0 % sy or w0 % sx:
        even = {(2, 2): " with h0 and w0 even", (2, 1): " with w0 even", (1, 1): ""}[(sx, sy)]
        raise ValueError(f"frames: packed {fmt} frames of shape {shape}{even}, got {tuple(frames.shape)}")
    ch, cw = h0 // sy, w0 // sx
    y, c = frames[:, :h0], frames[:, h0:]
    if layout == "semi":                                                              # ch rows of cw (u, v) pairs
        uv = c.unflatten(2, (cw, 2))
        return y, uv[..., 0], uv[..., 1]
    if sx == 1:                                                                       # a plane's rows are packed rows
        return y, c[:, :ch], c[:, ch:]
    if T > 0 and (c.stride(1), c.stride(2)) != (w0, 1):                               # (a row of the u plane is half a packed row)
        raise ValueError(f"frames: the samples of a packed {fmt} frame must be adjacent (strides (.., {w0}, 1)), got {frames.stride()}; "
                         "pass the planes of a crop instead")
    pl = c.as_strided((T, 2, ch, cw), (c.stride(0), ch * cw, cw, 1), c.storage_offset())
    return y, pl[:, 0], pl[:, 1]


def yuv420_planes(frames: torch.Tensor, fmt: str):
    """Packed 4:2:0 frames (T, 3 h0 / 2, w0) uint8 -- h0 luma rows, then NV12's h0 / 2 rows of interleaved (u, v) pairs or I420's u plane
    and v plane -- -> the views (y (T, h0, w0), u, v (T, h0 / 2, w0 / 2)); nothing is copied.  ValueError unless the rows are a multiple of
    3 and h0, w0 are even (an odd frame has no packed form: pass its planes)."""
    if fmt not in YUV_FORMATS:
        raise ValueError(f"fmt={fmt!r}: one of {YUV_FORMATS}")
    return _split_planes(frames, fmt, *_YUV420_FORMATS[fmt][:3])


def yuv_planes(frames: torch.Tensor, fmt: str):
    """Packed frames (T, rows, w0) of a YUV_PIXEL_FORMATS name, in its dtype -- h0 luma rows, then the chroma as the file's samples follow:
    a planar format's u plane and v plane, a semi-planar one's rows of interleaved (u, v) pairs; rows = h0 (1 + 2 / (sub_x sub_y)) -- -> the
    views (y (T, h0, w0), u, v (T, h0 / sub_y, w0 / sub_x)); nothing is copied.  TypeError for another dtype; ValueError unless the rows are
    whole, the sides even on every subsampled axis and (for subsampled planar chroma) a frame's samples adjacent."""
    if fmt not in YUV_PIXEL_FORMATS:
        raise ValueError(f"fmt={fmt!r}: one of {tuple(YUV_PIXEL_FORMATS)}")
    layout, sx, sy, _, _, dtype = YUV_PIXEL_FORMATS[fmt]
    if frames.dtype != dtype:
        raise TypeError(f"frames: expected {dtype} for {fmt}, got {frames.dtype}")
    return _split_planes(frames, fmt, layout, sx, sy)


def _yuv_plane_args(y, u, v, depth, shift, subsampling, matrix, range, siting, dtypes=_YUV_DTYPES):
    """The checks every YUV input call shares -> the kernel's arguments before (T, h0, w0) -- the format -- and after them: the strides, the
    seven coefficients and the siting.  `dtypes`: what the planes may be (the 8-bit 4:2:0 calls: uint8 alone, at depth 8, shift 0, (2, 2))."""
    for name, p in (("y", y), ("u", u), ("v", v)):
        if not p.is_cuda:
            raise _lib.FgvcHipError(f"{name} must be on the GPU (fgvc_amd has no CPU path)")
        if p.dtype not in dtypes:
            raise TypeError(f"{name}: expected {' or '.join(str(d) for d in dtypes)}, got {p.dtype}")
        if p.dim() != 3:
            raise ValueError(f"{name}: 3 dimensions ({'T, h0, w0' if name == 'y' else 'T, ceil(h0 / sub_y), ceil(w0 / sub_x)'}), got {tuple(p.shape)}")
    if u.dtype != y.dtype or v.dtype != y.dtype:
        raise TypeError(f"y, u, v: one dtype, got {y.dtype}, {u.dtype}, {v.dtype}")
    if siting not in YUV_SITINGS:
        raise ValueError(f"siting={siting!r}: one of {YUV_SITINGS}")
    try:
        sx, sy = (int(s) for s in subsampling)
    except (TypeError, ValueError):
        raise ValueError(f"subsampling={subsampling!r}: (sub_x, sub_y), each 1 or 2") from None
    if sx not in (1, 2) or sy not in (1, 2):
        raise ValueError(f"subsampling={subsampling!r}: (sub_x, sub_y), each 1 or 2")
    depth, shift = int(depth), int(shift)
    bits = 8 * y.element_size()
    if not 8 <= depth <= 16 or shift < 0 or depth + shift > bits:
        raise ValueError(f"depth={depth}, shift={shift}: depth 8..16 and depth + shift within the {bits} bits of {y.dtype}")
    coef = yuv_coefficients_depth(matrix, range, depth)
    T, h0, w0 = y.shape
    want = (T, (h0 + sy - 1) // sy, (w0 + sx - 1) // sx)
    if tuple(u.shape) != want or tuple(v.shape) != want:
        raise ValueError(f"u, v: chroma planes of shape {want} for luma {tuple(y.shape)} subsampled {(sx, sy)}, got {tuple(u.shape)} and "
                         f"{tuple(v.shape)}")
    if u.device != y.device or v.device != y.device:
        raise ValueError(f"y, u, v: one device, got {y.device}, {u.device}, {v.device}")
    if w0 > 1 and y.stride(2) != 1:
        raise ValueError(f"y: luma columns must be adjacent (last stride 1), got strides {y.stride()}")
    if any(n > 1 and su != sv for n, su, sv in zip(want, u.stride(), v.stride())):    # (an axis of one sample: its stride is never used)
        raise ValueError(f"u, v: the same strides (the kernel takes one set for both planes), got {u.stride()} and {v.stride()}")
    return (y.element_size(), depth, shift, sx, sy), (y.stride(0), y.stride(1), u.stride(0), u.stride(1), u.stride(2), *coef, YUV_SITINGS.index(siting))


def _yuv420_plane_args(y, u, v, matrix, range, siting):
    """-> what fgvc_frames_yuv420_* take after (T, h0, w0): no format, and the tail without c_off."""
    _, tail = _yuv_plane_args(y, u, v, 8, 0, (2, 2), matrix, range, siting, dtypes=(torch.uint8,))
    return (), tail[:7] + tail[8:]


def _planes_to_lab(entry: str, y, u, v, args, size, pad, out):
    fmt, tail = args
    T, h0, w0 = y.shape
    h, w, pad, out = _lab_out(T, h0, w0, size, pad, out, y.device)
    if T > 0:
        _lib.call(entry, _ptr(y), _ptr(u), _ptr(v), *fmt, T, h0, w0, *tail, h, w, *pad, _ptr(out), _stream(y))
    return out


def _planes_to_rgb8(entry: str, y, u, v, args, out):
    fmt, tail = args
    T, h0, w0 = y.shape
    out = _out(out, (T, h0, w0, 3), torch.uint8, y.device)
    if T > 0:
        _lib.call(entry, _ptr(y), _ptr(u), _ptr(v), *fmt, T, h0, w0, *tail, _ptr(out), _stream(y))
    return out


def yuv_frames_to_lab(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, size: Optional[Tuple[int, int]] = None,
                      pad: Tuple[int, int, int, int] = (0, 0, 0, 0), matrix: str = "bt601", range: str = "limited", siting: str = "left",
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """8-bit YUV 4:2:0 planes y (T, h0, w0), u, v (T, (h0 + 1) // 2, (w0 + 1) // 2) uint8 -> (T, 3, hp, wp) f32: per frame exactly
    datasets.preprocess_yuv420_frames (chroma bilinear at the luma pixel by `siting`; R'G'B' by `matrix` and `range`, unclamped; then
    frames_to_lab's steps) at (top, left) of a border of exact zeros -- one launch of fgvc_frames_yuv420_to_lab_f32.  The planes are read
    through their strides (yuv420_planes' views of packed NV12 / I420 frames, crops, time slices): nothing is copied; the luma columns
    must be adjacent and u, v share their strides.  NV21 / YV12: pass the planes swapped.  `size`, `pad`, `out`: as frames_to_lab's."""
    return _planes_to_lab("fgvc_frames_yuv420_to_lab_f32", y, u, v, _yuv420_plane_args(y, u, v, matrix, range, siting), size, pad, out)


def yuv_frames_to_rgb8(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, matrix: str = "bt601", range: str = "limited",
                       siting: str = "left", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same planes -> (T, h0, w0, 3) uint8 RGB: rint (half to even) of the unclamped R'G'B' clamped to [0, 255], exactly
    datasets.yuv420_to_rgb8 -- one launch of fgvc_frames_yuv420_to_rgb8.  What render_frames draws on.  `out`: a contiguous uint8 tensor
    of that shape on the planes' device."""
    return _planes_to_rgb8("fgvc_frames_yuv420_to_rgb8", y, u, v, _yuv420_plane_args(y, u, v, matrix, range, siting), out)


def yuv_planes_to_lab(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, depth: int = 8, shift: int = 0,
                      subsampling: Tuple[int, int] = (2, 2), size: Optional[Tuple[int, int]] = None,
                      pad: Tuple[int, int, int, int] = (0, 0, 0, 0), matrix: str = "bt601", range: str = "limited", siting: str = "left",
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Y'CbCr planes y (T, h0, w0), u, v (T, ceil(h0 / sub_y), ceil(w0 / sub_x)) -- uint8 or uint16, one dtype; a sample is
    (word >> shift) & (2^depth - 1); subsampling = (sub_x, sub_y), each 1 or 2 -- -> (T, 3, hp, wp) f32: per frame exactly
    datasets.preprocess_yuv_frames at (top, left) of a border of exact zeros, one launch of fgvc_frames_yuvp_to_lab_f32.  The planes are read
    through their strides (yuv_planes' views of packed frames, crops, time slices): nothing is copied; the luma columns must be adjacent
    and u, v share their strides.  `siting` places the chroma of a horizontally subsampled format only.  Swapped chroma (NV21-style): pass the
    planes swapped.  `size`, `pad`, `out`: as frames_to_lab's."""
    args = _yuv_plane_args(y, u, v, depth, shift, subsampling, matrix, range, siting)
    return _planes_to_lab("fgvc_frames_yuvp_to_lab_f32", y, u, v, args, size, pad, out)


def yuv_planes_to_rgb8(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, depth: int = 8, shift: int = 0,
                       subsampling: Tuple[int, int] = (2, 2), matrix: str = "bt601", range: str = "limited", siting: str = "left",
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The same planes -> (T, h0, w0, 3) uint8 RGB: rint (half to even) of the unclamped R'G'B' clamped to [0, 255], exactly
    datasets.yuv_to_rgb8 -- one launch of fgvc_frames_yuvp_to_rgb8.  `out`: a contiguous uint8 tensor of that shape on the planes' device."""
    args = _yuv_plane_args(y, u, v, depth, shift, subsampling, matrix, range, siting)
    return _planes_to_rgb8("fgvc_frames_yuvp_to_rgb8", y, u, v, args, out)


# ---- the output stage for 8-bit YUV 4:2:0 video: RGB bytes -> NV12 / I420 ------------------------------------------

YUV_OUT_TILE = (8, 512)  # luma rows, columns one workgroup of fgvc_frames_rgb8_to_yuv420 owns (= fgvc_yuv_out_tile_rows/_cols(); the tests go one past them)


def rgb_to_yuv_coefficients(matrix: str = "bt601", range: str = "limited") -> Tuple[float, float, float, float, float, float, float]:
    """(kr, kg, kb, y_off, sy, cu, cv) of Y = y_off + sy lum, U = 128 + cu (B - lum), V = 128 + cv (R - lum) with lum = (kr R + kg G) + kb B:
    the inverse of yuv_coefficients' matrix, computed in float64 from the same tables -- kg = 1 - kr - kb, sy = 1 / cy,
    cu = 1 / (2 (1 - kb) sc), cv = 1 / (2 (1 - kr) sc) -- as Python floats.  The kernel takes them rounded to f32 once."""
    if matrix not in YUV_MATRICES:
        raise ValueError(f"matrix={matrix!r}: one of {tuple(YUV_MATRICES)}")
    if range not in YUV_RANGES:
        raise ValueError(f"range={range!r}: one of {tuple(YUV_RANGES)}")
    kr, kb = YUV_MATRICES[matrix]
    y_off, cy, sc = YUV_RANGES[range]
    return (kr, 1.0 - kr - kb, kb, y_off, 1.0 / cy, 1.0 / (2.0 * (1.0 - kb) * sc), 1.0 / (2.0 * (1.0 - kr) * sc))


def rgb_frames_to_yuv420(frames_u8: torch.Tensor, fmt: str = "i420", layout: str = "thwc", matrix: str = "bt601", range: str = "limited",
                         siting: str = "left", out: Optional[torch.Tensor] = None, planes=None):
    """uint8 RGB frames (T, h0, w0, 3) ('thwc') or (T, 3, h0, w0) ('tchw') -> 8-bit Y'CbCr 4:2:0, exactly datasets.rgb8_to_yuv420 (Y' at
    every pixel; the R, G, B bytes filtered to the chroma position of `siting`, edge clamped, then Cb, Cr; rint half to even of the clamped
    value) -- one launch of fgvc_frames_rgb8_to_yuv420 on the current stream.  The frames are read through their own strides: a view (a
    crop, a permuted tensor, a time slice) is not copied.
    Without `planes`: returns the packed (T, 3 h0 / 2, w0) frames of `fmt` ('i420' | 'nv12', what yuv420_planes takes apart and
    datasets.write_y4m writes), into `out` when given (a contiguous uint8 tensor of that shape on the frames' device); h0 and w0 must be even.
    With planes=(y, u, v): writes into those uint8 views -- y (T, h0, w0) with adjacent columns, u, v (T, (h0 + 1) // 2, (w0 + 1) // 2) with
    the same strides; odd sizes, row strides wider than the rows, yuv420_planes' views of a packed buffer -- and returns them; `fmt` and
    `out` do not apply.  NV21 / YV12: pass u and v swapped.  The outputs must not overlap the frames."""
    if layout not in INPUT_LAYOUTS:
        raise ValueError(f"layout={layout!r}: one of {INPUT_LAYOUTS}")
    if siting not in YUV_SITINGS:
        raise ValueError(f"siting={siting!r}: one of {YUV_SITINGS}")
    coef = rgb_to_yuv_coefficients(matrix, range)
    if not frames_u8.is_cuda:
        raise _lib.FgvcHipError("frames_u8 must be on the GPU (fgvc_amd has no CPU path)")
    if frames_u8.dtype != torch.uint8:
        raise TypeError(f"frames_u8: expected torch.uint8, got {frames_u8.dtype}")
    if frames_u8.dim() != 4:
        raise ValueError(f"frames_u8: 4 dimensions ({'T, h0, w0, 3' if layout == 'thwc' else 'T, 3, h0, w0'}), got {tuple(frames_u8.shape)}")
    f = frames_u8 if layout == "thwc" else frames_u8.permute(0, 2, 3, 1)              # (T, h0, w0, 3) view either way
    T, h0, w0, ch = f.shape
    if ch != 3:
        raise ValueError(f"frames_u8: 3 channels (RGB) in layout {layout!r}, got {ch} (shape {tuple(frames_u8.shape)})")
    if h0 == 0 or w0 == 0:
        raise ValueError(f"frames_u8: empty frames ({h0} x {w0})")
    dev = f.device
    if planes is None:
        if fmt not in YUV_FORMATS:
            raise ValueError(f"fmt={fmt!r}: one of {YUV_FORMATS}")
        if h0 % 2 or w0 % 2:
            raise ValueError(f"frames_u8: {h0} x {w0} frames have no packed {fmt} form (an odd side); pass planes=(y, u, v) instead")
        shape = (T, h0 // 2 * 3, w0)
        if out is None:
            out = torch.empty(shape, device=dev, dtype=torch.uint8)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != dev or not out.is_contiguous():
            raise ValueError(f"out: a contiguous uint8 tensor of shape {shape} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        y, u, v = yuv420_planes(out, fmt)
        result = out
    else:
        if out is not None:
            raise ValueError("out: goes with the packed form; with planes=(y, u, v) the planes are the output")
        if len(planes) != 3:
            raise ValueError(f"planes: (y, u, v), got {len(planes)} tensors")
        y, u, v = planes
        want = (T, (h0 + 1) // 2, (w0 + 1) // 2)
        for name, p, shp in (("y", y, (T, h0, w0)), ("u", u, want), ("v", v, want)):
            if not p.is_cuda or p.device != dev:
                raise ValueError(f"planes: {name} on {dev} with the frames, got {p.device}")
            if p.dtype != torch.uint8:
                raise TypeError(f"planes: {name}: expected torch.uint8, got {p.dtype}")
            if tuple(p.shape) != shp:
                raise ValueError(f"planes: {name} of shape {shp} for frames {tuple(frames_u8.shape)} in layout {layout!r}, got {tuple(p.shape)}")
        if w0 > 1 and y.stride(2) != 1:
            raise ValueError(f"planes: luma columns must be adjacent (last stride 1), got strides {y.stride()}")
        if any(n > 1 and su != sv for n, su, sv in zip(want, u.stride(), v.stride())):    # (an axis of one sample: its stride is never used)
            raise ValueError(f"planes: u, v: the same strides (the kernel takes one set for both planes), got {u.stride()} and {v.stride()}")
        result = (y, u, v)
    if T == 0:
        return result

    def stride(p, d, n, least):
        """an axis of one sample has no stride to speak of: the least the kernel's overlap check accepts"""
        return p.stride(d) if n > 1 else max(p.stride(d), least)
    cw, chh = (w0 + 1) // 2, (h0 + 1) // 2
    csx = stride(u, 2, cw, 1)
    csy = stride(u, 1, chh, (cw - 1) * csx + 1)
    ysy = stride(y, 1, h0, w0)
    st, sy, sx, sc = f.stride()                                                       # (uint8: elements are bytes)
    _lib.call("fgvc_frames_rgb8_to_yuv420", _ptr(f), T, h0, w0, st, sy, sx, sc, _ptr(y), y.stride(0), ysy, _ptr(u), _ptr(v), u.stride(0), csy, csx,
              *coef, YUV_SITINGS.index(siting), _stream(f))
    return result


# ---- DAVIS J&F on the device: the integer counts metrics.db_eval_iou / f_measure divide ------------------------

JF_TILE = 32            # rows one workgroup of fgvc_jf_counts_u8 owns (= fgvc_jf_tile_rows(); the tests put mask edges on its multiples)
JF_MAX_RADIUS = 64


def jf_counts(gt: torch.Tensor, pred: torch.Tensor, n_objects: int, radius: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gt, pred (T, h, w) uint8 object ids (0 = background) -> (T, n_objects, 6) int64: per frame and object o = 1 .. n_objects, with
    G = (gt == o) and S = (pred == o): |G & S|, |G | S|, |b(S)|, |b(G)|, |b(S) & dil(b(G))|, |b(G) & dil(b(S))| -- b = metrics._seg2bmap,
    dil = the dilation by metrics._disk(radius) -- one launch of fgvc_jf_counts_u8 on the current stream; metrics.jf_from_counts turns
    them into J and F.  A non-contiguous view is made contiguous (a copy).  `out`: a contiguous (T, n_objects, 6) int64 tensor on gt's
    device; every element is written, the caller clears nothing."""
    for name, m in (("gt", gt), ("pred", pred)):
        if not m.is_cuda:
            raise _lib.FgvcHipError(f"{name} must be on the GPU (fgvc_amd has no CPU path)")
        if m.dtype != torch.uint8:
            raise TypeError(f"{name}: expected torch.uint8 object ids, got {m.dtype}")
        if m.dim() != 3:
            raise ValueError(f"{name}: 3 dimensions (T, h, w), got {tuple(m.shape)}")
    if gt.shape != pred.shape or gt.device != pred.device:
        raise ValueError(f"gt {tuple(gt.shape)} on {gt.device} and pred {tuple(pred.shape)} on {pred.device}: one shape, one device")
    n_objects, radius = int(n_objects), int(radius)
    if not 0 <= n_objects <= 255:
        raise ValueError(f"n_objects={n_objects}: 0 .. 255 (the ids are bytes)")
    if not 1 <= radius <= JF_MAX_RADIUS:
        raise ValueError(f"radius={radius}: 1 .. {JF_MAX_RADIUS}")
    T, h, w = gt.shape
    shape = (T, n_objects, 6)
    if out is None:
        out = torch.empty(shape, device=gt.device, dtype=torch.int64)
    elif tuple(out.shape) != shape or out.dtype != torch.int64 or out.device != gt.device or not out.is_contiguous():
        raise ValueError(f"out: a contiguous int64 tensor of shape {shape} on {gt.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    if T == 0 or n_objects == 0:
        return out
    gt, pred = gt.contiguous(), pred.contiguous()
    _lib.call("fgvc_jf_counts_u8", _ptr(gt), _ptr(pred), T, h, w, n_objects, radius, _ptr(out), _stream(gt))
    return out


# ---- objects as boxes: area, box, coordinate sums and border count per frame and id -----------------------------

OBJECT_WORDS = ("area", "x0", "y0", "x1", "y1", "sum_x", "sum_y", "border")


def object_stats(ids: torch.Tensor, n_ids: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ids (T, h, w) uint8 on the GPU -> (T, n_ids, 8) int64: per frame and id o = 0 .. n_ids - 1 (the background has its row), over the
    pixels with that id: area, x0 = min x, y0 = min y, x1 = max x + 1, y1 = max y + 1, sum of x, sum of y, and the number of them on the
    frame's outermost rows and columns -- metrics.object_stats_host word for word, in one launch of fgvc_seg_object_stats_u8 on the current
    stream.  An absent id: eight zeros; ids of n_ids or more are counted nowhere.  1 <= n_ids <= 256.  The map is read through its frame
    and row strides (a time slice or a window is not copied; pixels must be packed, else a contiguous copy is made).  `out`: a contiguous
    (T, n_ids, 8) int64 tensor on ids' device; every element is written, the caller clears nothing."""
    if not ids.is_cuda:
        raise _lib.FgvcHipError("ids must be on the GPU (fgvc_amd has no CPU path)")
    if ids.dtype != torch.uint8:
        raise TypeError(f"ids: expected torch.uint8 object ids, got {ids.dtype}")
    if ids.dim() != 3:
        raise ValueError(f"ids: 3 dimensions (T, h, w), got {tuple(ids.shape)}")
    n_ids = int(n_ids)
    if not 1 <= n_ids <= 256:
        raise ValueError(f"n_ids={n_ids}: 1 .. 256 (the ids are bytes)")
    T, h, w = ids.shape
    shape = (T, n_ids, 8)
    if out is None:
        out = torch.empty(shape, device=ids.device, dtype=torch.int64)
    elif tuple(out.shape) != shape or out.dtype != torch.int64 or out.device != ids.device or not out.is_contiguous():
        raise ValueError(f"out: a contiguous int64 tensor of shape {shape} on {ids.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    if T == 0:
        return out
    if h == 0 or w == 0:
        return out.zero_()
    if not (ids.stride(2) == 1 and ids.stride(1) >= w and ids.stride(0) >= 0):
        ids = ids.contiguous()
    _lib.call("fgvc_seg_object_stats_u8", _ptr(ids), ids.stride(0), ids.stride(1), T, h, w, n_ids, _ptr(out), _stream(ids))
    return out


# ---- connected components of id maps: labels, despeckle, keep largest, fill holes ------------------------------

CCL_TILE = (16, 64)     # rows, columns one workgroup of the labelling kernels owns (= fgvc_seg_ccl_tile_rows/_cols(); the tests put components on its seams)
CLEAN_WORDS = ("components", "kept", "dropped_pixels", "filled_pixels")


def _ccl_ids(ids: torch.Tensor) -> torch.Tensor:
    if not ids.is_cuda:
        raise _lib.FgvcHipError("ids must be on the GPU (fgvc_amd has no CPU path)")
    if ids.dtype != torch.uint8:
        raise TypeError(f"ids: expected torch.uint8 object ids, got {ids.dtype}")
    if ids.dim() != 3:
        raise ValueError(f"ids: 3 dimensions (T, h, w), got {tuple(ids.shape)}")
    T, h, w = ids.shape
    if h * w >= 1 << 31:
        raise ValueError(f"ids: a frame of {h} x {w} has 2^31 pixels or more")
    return ids


def _strided_rows(m: torch.Tensor) -> bool:
    return m.stride(2) == 1 and m.stride(1) >= m.shape[2] and m.stride(0) >= 0


def seg_components(ids: torch.Tensor, connectivity: int = 8, background: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ids (T, h, w) uint8 on the GPU -> (T, h, w) int32: each pixel's label is the smallest index y * w + x of its connected component
    -- pixels of one id that are 4- or 8-neighbours (`connectivity`; id 0 always 4) -- and -1 on id 0 unless background=True:
    metrics.components_host word for word, in three launches of fgvc_seg_components_i32 on the current stream.  The map is read through
    its frame and row strides (pixels must be packed, else a contiguous copy is made).  `out`: a contiguous (T, h, w) int32 tensor on ids'
    device; every element is written."""
    ids = _ccl_ids(ids)
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity={connectivity}: 4 or 8")
    T, h, w = ids.shape
    if out is None:
        out = torch.empty((T, h, w), device=ids.device, dtype=torch.int32)
    elif tuple(out.shape) != (T, h, w) or out.dtype != torch.int32 or out.device != ids.device or not out.is_contiguous():
        raise ValueError(f"out: a contiguous int32 tensor of shape {(T, h, w)} on {ids.device}, got {out.dtype} {tuple(out.shape)} on {out.device}")
    if T == 0 or h == 0 or w == 0:
        return out
    if not _strided_rows(ids):
        ids = ids.contiguous()
    _lib.call("fgvc_seg_components_i32", _ptr(ids), ids.stride(0), ids.stride(1), T, h, w, int(connectivity), int(bool(background)), _ptr(out),
              _stream(ids))
    return out


def seg_clean_workspace_bytes(T: int, h: int, w: int, n_ids: int) -> int:
    """The bytes of device memory ops.seg_clean needs as `workspace` for a (T, h, w) map (fgvc_seg_clean_workspace_bytes)."""
    return int(_lib.load().fgvc_seg_clean_workspace_bytes(int(T), int(h), int(w), int(n_ids)))


def seg_clean(ids: torch.Tensor, n_ids: int, connectivity: int = 8, min_area: int = 0, keep: str = "all", fill_holes: bool = False,
              max_hole_area: Optional[int] = None, frames: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
              stats: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """ids (T, h, w) uint8 on the GPU -> (out (T, h, w) uint8, stats (T, n_ids, 4) int64): out = fill(drop(ids)) per frame,
    metrics.clean_masks_host word for word (fgvc_seg_clean_u8: four launches, five with keep='largest', four more with fill_holes, on the
    current stream).  Drop: a component of an id 1 .. n_ids - 1 becomes 0 when it has fewer than min_area pixels, with keep='largest' also
    when it is not the largest of its id on the frame (equal areas: the smaller root).  Fill: a 4-connected background component inside
    the frame whose neighbours carry one id o < n_ids, of at most max_hole_area pixels (None: any), becomes o.  frames: (T,) bools on
    the device; a frame whose entry is false is copied and its stats are zero.  stats[t, o] = CLEAN_WORDS.  ids is read through its frame
    and row strides (pixels must be packed, else a contiguous copy is made); `out` may be ids itself, or a (T, h, w) uint8 tensor with packed
    pixels on ids' device that does not overlap it; `stats`: contiguous (T, n_ids, 4) int64; `workspace`: a contiguous uint8 tensor of at least
    seg_clean_workspace_bytes(T, h, w, n_ids) bytes, whose contents do not matter (allocated when None).  Every element of out and stats
    is written."""
    ids = _ccl_ids(ids)
    n_ids = int(n_ids)
    if not 1 <= n_ids <= 256:
        raise ValueError(f"n_ids={n_ids}: 1 .. 256 (the ids are bytes)")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity={connectivity}: 4 or 8")
    if keep not in ("all", "largest"):
        raise ValueError(f"keep={keep!r}: 'all' or 'largest'")
    min_area = int(min_area)
    if not 0 <= min_area < 1 << 31:
        raise ValueError(f"min_area={min_area}: 0 .. 2^31 - 1")
    if max_hole_area is not None and int(max_hole_area) < 0:
        raise ValueError(f"max_hole_area={max_hole_area}: at least 0, or None")
    T, h, w = ids.shape
    dev = ids.device
    if frames is not None and (tuple(frames.shape) != (T,) or frames.dtype != torch.bool or frames.device != dev):
        raise ValueError(f"frames: a bool tensor of shape ({T},) on {dev}, got {frames.dtype} {tuple(frames.shape)} on {frames.device}")
    in_place = out is ids
    if out is not None and not in_place and (tuple(out.shape) != (T, h, w) or out.dtype != torch.uint8 or out.device != dev
                                             or not (T == 0 or h == 0 or w == 0 or _strided_rows(out))):
        raise ValueError(f"out: ids itself or a uint8 tensor of shape {(T, h, w)} with packed pixels on {dev}, got {out.dtype} "
                         f"{tuple(out.shape)} on {out.device}")
    shape = (T, n_ids, 4)
    if stats is None:
        stats = torch.empty(shape, device=dev, dtype=torch.int64)
    elif tuple(stats.shape) != shape or stats.dtype != torch.int64 or stats.device != dev or not stats.is_contiguous():
        raise ValueError(f"stats: a contiguous int64 tensor of shape {shape} on {dev}, got {stats.dtype} {tuple(stats.shape)} on {stats.device}")
    if out is None:
        out = torch.empty((T, h, w), device=dev, dtype=torch.uint8)
    if T == 0:
        return out, stats
    if h == 0 or w == 0:
        return out, stats.zero_()
    if not _strided_rows(ids):
        if in_place:
            raise ValueError("out: in place needs ids with packed pixels, rows that do not overlap and a non-negative frame stride")
        ids = ids.contiguous()
    if in_place:
        out = ids
    if (T > 1 and out.stride(0) < (h - 1) * out.stride(1) + w):
        raise ValueError("out: its frames must not overlap")
    need = seg_clean_workspace_bytes(T, h, w, n_ids)
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"workspace: a contiguous uint8 tensor of at least {need} bytes on {dev} (seg_clean_workspace_bytes), got "
                         f"{workspace.dtype} of {workspace.numel()} elements on {workspace.device}")
    if frames is not None:
        frames = frames.contiguous()
    _lib.call("fgvc_seg_clean_u8", _ptr(ids), ids.stride(0), ids.stride(1), T, h, w, n_ids, int(connectivity), min_area,
              int(keep == "largest"), int(bool(fill_holes)), -1 if max_hole_area is None else int(max_hole_area),
              _ptr(frames) if frames is not None else None, _ptr(out), out.stride(0), out.stride(1), _ptr(stats), _ptr(workspace),
              workspace.numel(), _stream(ids))
    return out, stats


# ---- object crops: windows that follow each object, resampled on the device -----------------------------------------

def _objects_tensor(objects, device) -> torch.Tensor:
    return torch.tensor(list(objects), dtype=torch.int32, device=device)


def object_windows(stats: torch.Tensor, size, pad: float = 0.125, min_side: int = 8, smooth: int = 0, mask_size=None, frame_size=None,
                   objects=None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """stats (T, N, 8) int64 on the GPU, as object_stats gives them -> windows (T, M, 8) int64 for the M ids of `objects` (a sequence of
    Python ints on the host; default 1 .. N - 1): per frame and object the crop window of size's aspect around the object's box, grown by
    `pad` and at least `min_side`, averaged over the `smooth` frames on each side on which the object is present; words 0 .. 3 in mask
    pixels (mask_size = (h, w)), words 4 .. 7 in the pixels of frame_size = (H, W) (None: mask_size); eight zeros where the object is
    absent -- metrics.object_windows_host word for word, in one launch of fgvc_seg_object_windows_i64 on the current stream.  Nothing is read
    back.  Refused by name before the launch: a size outside 1 .. 1024, pad outside 0 .. 4, a side above 32768, an id outside 0 .. N - 1.
    `out`: a contiguous (T, M, 8) int64 tensor on stats' device; every element is written."""
    from . import metrics
    if not isinstance(stats, torch.Tensor) or not stats.is_cuda:
        raise _lib.FgvcHipError("stats must be on the GPU (fgvc_amd has no CPU path; metrics.object_windows_host is the host contract)")
    if stats.dtype != torch.int64 or stats.dim() != 3 or stats.shape[2] != 8:
        raise ValueError(f"stats: (T, N, 8) int64, got {stats.dtype} {tuple(stats.shape)}")
    T, N = stats.shape[:2]
    objs, S_h, S_w, pad_q, min_side, smooth, h, w, H, W = metrics.window_args(N, size, pad, min_side, smooth, mask_size, frame_size, objects)
    M = len(objs)
    out = _out(out, (T, M, 8), torch.int64, stats.device)
    if T == 0 or M == 0:
        return out
    stats = stats.contiguous()
    o = _objects_tensor(objs, stats.device)
    _lib.call("fgvc_seg_object_windows_i64", _ptr(stats), T, N, _ptr(o), M, S_h, S_w, pad_q, min_side, smooth, h, w, H, W, _ptr(out),
              _stream(stats))
    return out


def _crop_size(size) -> Tuple[int, int]:
    from . import viz
    try:
        S_h, S_w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f"size={size!r}: (S_h, S_w)") from None
    if not (1 <= S_h <= viz.CROP_MAX_SIZE and 1 <= S_w <= viz.CROP_MAX_SIZE):
        raise ValueError(f"size={tuple(size)}: S_h and S_w in 1 .. {viz.CROP_MAX_SIZE}")
    return S_h, S_w


def _crop_taps(max_taps, frame_size, size) -> int:
    from . import viz
    taps = viz.crop_default_taps(frame_size, size) if max_taps is None else int(max_taps)
    if not 4 <= taps <= viz.CROP_MAX_TAPS:
        raise ValueError(f"max_taps={taps}: 4 .. {viz.CROP_MAX_TAPS} taps per axis")
    return taps


def object_crops_workspace_bytes(T: int, M: int, size, frame_size=None, max_taps: Optional[int] = None) -> int:
    """The bytes of device memory ops.object_crops needs as `workspace` for T x M crops of `size` (fgvc_frames_object_crops_workspace_bytes):
    the coefficient table, 4 (S_h + S_w)(2 + max_taps) bytes a crop.  max_taps None: viz.crop_default_taps(frame_size, size), what
    object_crops takes by default for frames of frame_size = (H, W).  Known on the host without reading a window back."""
    S_h, S_w = _crop_size(size)
    if max_taps is None and frame_size is None:
        raise ValueError("frame_size: (H, W) of the frames, or max_taps")
    taps = _crop_taps(max_taps, frame_size, (S_h, S_w))
    if int(T) < 1 or int(M) < 1:
        return 0
    return int(_lib.load().fgvc_frames_object_crops_workspace_bytes(int(T), int(M), S_h, S_w, taps))


def object_crops(frames_u8: torch.Tensor, windows: torch.Tensor, size, layout: str = "thwc", fill=None, ids: Optional[torch.Tensor] = None,
                 objects=None, out: Optional[torch.Tensor] = None, mask_out: Optional[torch.Tensor] = None,
                 workspace: Optional[torch.Tensor] = None, max_taps: Optional[int] = None):
    """uint8 RGB frames (T, H, W, 3) ('thwc') or (T, 3, H, W) ('tchw') on the GPU and windows (T, M, 8) int64 as object_windows gives them
    -- or (T, M, 4) integer windows (x0, y0, x1, y1) of the caller's own -- -> crops (T, M, S_h, S_w, 3) uint8: every window resampled onto
    size = (S_h, S_w) with the triangle filter widened by the scale (anti-aliased; Pillow's BILINEAR resize with box=), fixed-point
    coefficients, horizontal pass then vertical with a uint8 intermediate, everything outside the frame `fill` ((3,) uint8 values on the
    host, default zeros) -- viz.crop_windows_host byte for byte, in two launches of fgvc_frames_object_crops_u8 on the current stream.
    With ids (T, h, w) uint8 and objects (M ids, Python ints) also masks (T, M, S_h, S_w) uint8 (255 where the nearest pixel of the
    mask-space window carries the object's id), returned as a pair.  The frames are read through their strides (a slice, a window of a
    larger tensor, a permuted view is not copied); ids through its frame and row strides.  A window that is empty, has a coordinate of
    2^30 or more in magnitude or needs more than max_taps taps on an axis (viz.crop_window_ok; max_taps None:
    viz.crop_default_taps, enough for windows up to twice the frame's side; at most 256) gives a crop of `fill` and a mask of zeros.
    `out`, `mask_out`: contiguous uint8 tensors of those shapes; `workspace`: a contiguous uint8 tensor of at least
    object_crops_workspace_bytes(T, M, size, (H, W), max_taps) bytes whose contents do not matter (allocated when None).  Nothing is read
    back."""
    if layout not in INPUT_LAYOUTS:
        raise ValueError(f"layout={layout!r}: one of {INPUT_LAYOUTS}")
    if not frames_u8.is_cuda:
        raise _lib.FgvcHipError("frames_u8 must be on the GPU (fgvc_amd has no CPU path; viz.crop_windows_host is the host contract)")
    if frames_u8.dtype != torch.uint8:
        raise TypeError(f"frames_u8: expected torch.uint8, got {frames_u8.dtype}")
    if frames_u8.dim() != 4:
        raise ValueError(f"frames_u8: 4 dimensions ({'T, H, W, 3' if layout == 'thwc' else 'T, 3, H, W'}), got {tuple(frames_u8.shape)}")
    f = frames_u8 if layout == "thwc" else frames_u8.permute(0, 2, 3, 1)
    T, H, W, ch = f.shape
    dev = f.device
    if ch != 3:
        raise ValueError(f"frames_u8: 3 channels (RGB) in layout {layout!r}, got {ch} (shape {tuple(frames_u8.shape)})")
    if T and not (1 <= H <= 32768 and 1 <= W <= 32768):
        raise ValueError(f"frames_u8: H, W = {H}, {W} (1 .. 32768)")
    S_h, S_w = _crop_size(size)
    if not isinstance(windows, torch.Tensor) or windows.device != dev:
        raise ValueError(f"windows: a tensor on {dev} with the frames")
    if windows.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise TypeError(f"windows: expected an integer type, got {windows.dtype}")
    if windows.dim() != 3 or windows.shape[0] != T or windows.shape[2] not in (4, 8):
        raise ValueError(f"windows: ({T}, M, 8) or ({T}, M, 4) to go with the frames, got {tuple(windows.shape)}")
    M, words = windows.shape[1], windows.shape[2]
    win = windows.to(torch.int64).contiguous()
    if fill is None:
        fill = (0, 0, 0)
    fill = [int(v) for v in (fill.tolist() if hasattr(fill, "tolist") else fill)]
    if len(fill) != 3 or not all(0 <= v <= 255 for v in fill):
        raise ValueError(f"fill={fill}: three bytes (R, G, B)")
    if (ids is None) != (objects is None):
        raise ValueError("ids and objects: both or neither")
    if mask_out is not None and ids is None:
        raise ValueError("mask_out: without ids there are no masks")
    h = w = 0
    obj = None
    if ids is not None:
        if not isinstance(ids, torch.Tensor) or ids.device != dev or ids.dtype != torch.uint8:
            raise ValueError(f"ids: a uint8 tensor on {dev} with the frames")
        if ids.dim() != 3 or ids.shape[0] != T:
            raise ValueError(f"ids: ({T}, h, w) to go with the frames, got {tuple(ids.shape)}")
        h, w = ids.shape[1:]
        if T and not (1 <= h <= 32768 and 1 <= w <= 32768):
            raise ValueError(f"ids: h, w = {h}, {w} (1 .. 32768)")
        objs = [int(o) for o in objects]
        if len(objs) != M:
            raise ValueError(f"objects: {M} ids to go with the windows, got {len(objs)}")
        for o in objs:
            if not 0 <= o <= 255:
                raise ValueError(f"objects: id {o} outside 0 .. 255 (the ids are bytes)")
        if not _strided_rows(ids):
            ids = ids.contiguous()
        obj = _objects_tensor(objs, dev)
    taps = _crop_taps(max_taps, (max(H, 1), max(W, 1)), (S_h, S_w))
    out = _out(out, (T, M, S_h, S_w, 3), torch.uint8, dev)
    masks = None
    if ids is not None:
        try:
            masks = _out(mask_out, (T, M, S_h, S_w), torch.uint8, dev)
        except ValueError as e:
            raise ValueError("mask_" + str(e)) from None
    if T == 0 or M == 0:
        return out if masks is None else (out, masks)
    need = int(_lib.load().fgvc_frames_object_crops_workspace_bytes(T, M, S_h, S_w, taps))
    if workspace is None:
        workspace = torch.empty(need, device=dev, dtype=torch.uint8)
    elif workspace.dtype != torch.uint8 or workspace.device != dev or not workspace.is_contiguous() or workspace.numel() < need:
        raise ValueError(f"workspace: a contiguous uint8 tensor of at least {need} bytes on {dev} (object_crops_workspace_bytes), got "
                         f"{workspace.dtype} of {workspace.numel()} elements on {workspace.device}")
    st, sy, sx, sc = f.stride()
    _lib.call("fgvc_frames_object_crops_u8", _ptr(f), T, H, W, st, sy, sx, sc, _ptr(win), words, M, S_h, S_w, *fill,
              None if ids is None else _ptr(ids), 0 if ids is None else ids.stride(0), 0 if ids is None else ids.stride(1), h, w,
              None if obj is None else _ptr(obj), taps, _ptr(out), None if masks is None else _ptr(masks), _ptr(workspace),
              workspace.numel(), _stream(f))
    return out if masks is None else (out, masks)


# ---- render: mask overlay and point icons onto uint8 video -------------------------------------------------------

RENDER_TILE = (8, 256)  # rows, columns one workgroup of fgvc_render_frames_u8 owns (= fgvc_render_tile_rows/_cols(); the tests put points on its corners)
RENDER_MAX_RADIUS = 31
_render_tables: dict = {}


def _render_table(key, device, make):
    """Small constant tables of the renderer on the device (the icon per radius, the default palette), uploaded once per device."""
    k = (key, str(device))
    if k not in _render_tables:
        import numpy as np
        _render_tables[k] = torch.from_numpy(np.array(make())).to(device)             # (a writable copy: the tables are read-only)
    return _render_tables[k]


def render_frames(frames_u8: torch.Tensor, ids: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None, alpha: int = 128,
                  contour: bool = True, tracks: Optional[torch.Tensor] = None, visibles: Optional[torch.Tensor] = None,
                  colors: Optional[torch.Tensor] = None, radius: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """frames_u8 (T, H, W, 3) uint8 -> the same with the objects of ids (T, H, W) uint8 blended in (palette (256, 3) uint8, None: the DAVIS
    palette; alpha 0 .. 256; contour) and then the points of tracks (P, T, 2) as (x, y) painted on (visibles (P, T) bool or uint8, None: all;
    colors (P, 3) uint8, None: viz.track_colors(P); radius 1 .. 31, None: the reference's round(min(H, W) * 0.015)) -- viz.render's host
    backend bit for bit, in one launch of fgvc_render_frames_u8 on the current stream.  Everything is a tensor on the frames' device.
    Frames, ids and `out` are read and written through their own frame and row strides (a time slice or a cropped window is not copied;
    pixels must be packed); tracks of another float type are converted to float64 first (exact).  `out`: a (T, H, W, 3) uint8 tensor to write
    into, `frames_u8` itself included; neither ids nor tracks: a copy."""
    head, out, _, hold = _render_head(frames_u8, ids, palette, alpha, contour, tracks, visibles, colors, radius, out)
    if head is not None:
        _lib.call("fgvc_render_frames_u8", *head, _stream(out))
    return out


def _render_head(frames_u8, ids, palette, alpha, contour, tracks, visibles, colors, radius, out, dots=True):
    """What render_frames, render_trails and render_pose share: the checks on the frames, `out`, ids and tracks (dots=False: no radius, no
    icon).  Returns (head, out, colors, hold): the 25 leading arguments of the three entries (None when no pixel exists: nothing to
    launch), the tensor to return, the points' colours as checked (None without tracks), and every tensor `head` points into -- the
    caller keeps `hold` until its call has returned."""
    from . import viz
    if not frames_u8.is_cuda:
        raise _lib.FgvcHipError("frames_u8 must be on the GPU (fgvc_amd has no CPU path)")
    if frames_u8.dtype != torch.uint8:
        raise TypeError(f"frames_u8: expected torch.uint8, got {frames_u8.dtype}")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"frames_u8: (T, H, W, 3), got {tuple(frames_u8.shape)}")
    dev = frames_u8.device
    T, H, W, _ = frames_u8.shape

    def packed(x, px):
        """the view itself when its pixels are packed (px bytes each), its rows apart and its strides non-negative, else a contiguous copy"""
        inner = x.stride(2) == px and (px == 1 or x.stride(3) == 1)
        return x if x.numel() == 0 or (inner and x.stride(0) >= 0 and x.stride(1) >= W * px) else x.contiguous()
    f = packed(frames_u8, 3)
    if out is None:
        out = torch.empty((T, H, W, 3), device=dev, dtype=torch.uint8)
    else:
        if tuple(out.shape) != (T, H, W, 3) or out.dtype != torch.uint8 or out.device != dev:
            raise ValueError(f"out: a uint8 tensor of shape {(T, H, W, 3)} on {dev}, got {out.dtype} {tuple(out.shape)} on {out.device}")
        if packed(out, 3) is not out:
            raise ValueError(f"out: packed pixels and non-negative strides, got strides {out.stride()}")
    hold = [f]
    args_ids = (None, 0, 0, None, 128, 0)
    if ids is not None:
        if not ids.is_cuda or ids.device != dev:
            raise ValueError(f"ids: on {dev} with the frames, got {ids.device}")
        if ids.dtype != torch.uint8:
            raise TypeError(f"ids: expected torch.uint8 object ids, got {ids.dtype}")
        if tuple(ids.shape) != (T, H, W):
            raise ValueError(f"ids: {(T, H, W)} to go with the frames, got {tuple(ids.shape)}")
        if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
            raise ValueError(f"alpha={alpha!r}: an integer in 0 .. 256")
        if palette is None:
            palette = _render_table("palette", dev, viz.davis_palette)
        if palette.dtype != torch.uint8:
            raise TypeError(f"palette: expected torch.uint8, got {palette.dtype}")
        if tuple(palette.shape) != (256, 3) or palette.device != dev:
            raise ValueError(f"palette: (256, 3) on {dev}, got {tuple(palette.shape)} on {palette.device}")
        m, palette = packed(ids, 1), palette.contiguous()
        args_ids = (_ptr(m), m.stride(0), m.stride(1), _ptr(palette), int(alpha), int(bool(contour)))
        hold += [m, palette]
    args_pts, col = (None, 0, 0, None, 0, 0, None, 0, 0, None), None
    if tracks is not None:
        if tracks.device != dev:
            raise ValueError(f"tracks: on {dev} with the frames, got {tracks.device}")
        if tracks.dim() != 3 or tracks.shape[1] != T or tracks.shape[2] != 2:
            raise ValueError(f"tracks: (P, {T}, 2) to go with the frames, got {tuple(tracks.shape)}")
        if tracks.dtype == torch.bool or tracks.dtype.is_complex:
            raise TypeError(f"tracks: a real number type, got {tracks.dtype}")
        P = tracks.shape[0]
        r = viz.check_radius(radius, H, W) if dots else 0
        tr = tracks.to(torch.float64)
        if tr.stride(2) != 1 or tr.data_ptr() % 8:
            tr = tr.contiguous()
        vis = None
        if visibles is not None:
            if visibles.dtype not in (torch.bool, torch.uint8):
                raise TypeError(f"visibles: expected torch.bool (or uint8), got {visibles.dtype}")
            if tuple(visibles.shape) != (P, T) or visibles.device != dev:
                raise ValueError(f"visibles: {(P, T)} on {dev} to go with the tracks, got {tuple(visibles.shape)} on {visibles.device}")
            vis = visibles.view(torch.uint8) if visibles.dtype == torch.bool else visibles
        if colors is None:
            colors = torch.from_numpy(viz.track_colors(P)).to(dev)
        if colors.dtype != torch.uint8:
            raise TypeError(f"colors: expected torch.uint8, got {colors.dtype}")
        if tuple(colors.shape) != (P, 3) or colors.device != dev:
            raise ValueError(f"colors: {(P, 3)} on {dev} to go with the tracks, got {tuple(colors.shape)} on {colors.device}")
        col = colors.contiguous()
        icon = _render_table(("icon", r), dev, lambda: viz.icon_table(r)) if dots else None
        args_vis = (None, 0, 0) if vis is None else (_ptr(vis), vis.stride(0), vis.stride(1))
        args_pts = (_ptr(tr), tr.stride(0), tr.stride(1), *args_vis, _ptr(col), int(P), int(r), None if icon is None else _ptr(icon))
        hold += [tr, vis, col, icon]
    if T == 0 or H == 0 or W == 0:
        return None, out, col, hold
    head = (_ptr(f), f.stride(0), f.stride(1), _ptr(out), out.stride(0), out.stride(1), T, H, W, *args_ids, *args_pts)
    return head, out, col, hold


def render_trails(frames_u8: torch.Tensor, tracks: torch.Tensor, visibles: Optional[torch.Tensor] = None, colors: Optional[torch.Tensor] = None,
                  trail: int = 8, linewidth: float = 2.0, fade: Optional[torch.Tensor] = None, time_colors: Optional[torch.Tensor] = None,
                  ids: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None, alpha: int = 128, contour: bool = True,
                  radius: Optional[int] = None, dots: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """render_frames with motion trails: the overlay, then every point's last `trail` (1 .. 64) steps as line segments
    `linewidth` (1 .. 16) pixels wide, then (dots=True) the dots -- viz.render(trail=...)'s host backend bit for bit, in one launch of
    fgvc_render_trails_u8 on the current stream.  fade: (trail,) float64 in [0, 1] on the frames' device, the opacity by age (None:
    viz.trail_fade(trail)); time_colors: (T - 1, 3) uint8, the colour of step s (viz.spring_colors(T) is the reference's), None: the point's
    own `colors`.  Every other argument is render_frames'; with dots=False `radius` is not used."""
    from . import viz
    if tracks is None:
        raise ValueError("tracks: (P, T, 2), got None (trails need tracks)")
    dev = frames_u8.device
    L, lw, _ = viz._check_trails(trail, linewidth, None, "track")
    if fade is None:
        fade = _render_table(("fade", L), dev, lambda: viz.trail_fade(L))
    else:
        if not isinstance(fade, torch.Tensor) or fade.device != dev:
            raise ValueError(f"fade: a tensor on {dev} with the frames")
        if fade.dtype.is_complex or fade.dtype == torch.bool or tuple(fade.shape) != (L,):
            raise ValueError(f"fade: ({L},) real numbers to go with trail={L}, got {fade.dtype} {tuple(fade.shape)}")
        fade = fade.to(torch.float64).contiguous()
        if not bool(((fade >= 0) & (fade <= 1)).all()):
            raise ValueError("fade: values in [0, 1]")
    if time_colors is not None:
        T = frames_u8.shape[0] if frames_u8.dim() == 4 else 0
        if time_colors.dtype != torch.uint8:
            raise TypeError(f"time_colors: expected torch.uint8, got {time_colors.dtype}")
        if tuple(time_colors.shape) != (max(T - 1, 0), 3) or time_colors.device != dev:
            raise ValueError(f"time_colors: {(max(T - 1, 0), 3)} on {dev}, got {tuple(time_colors.shape)} on {time_colors.device}")
        time_colors = time_colors.contiguous()
    head, out, _, hold = _render_head(frames_u8, ids, palette, alpha, contour, tracks, visibles, colors, radius, out, bool(dots))
    if head is not None:
        ro2, g, _ = viz.trail_consts(lw)
        tcol = None if time_colors is None or frames_u8.shape[0] <= 1 else _ptr(time_colors)
        _lib.call("fgvc_render_trails_u8", *head, L, lw, ro2, g, _ptr(fade), tcol, _stream(out))
    return out


def render_pose(frames_u8: torch.Tensor, tracks: Optional[torch.Tensor] = None, visibles: Optional[torch.Tensor] = None,
                colors: Optional[torch.Tensor] = None, skeleton: Optional[torch.Tensor] = None, limb_colors: Optional[torch.Tensor] = None,
                limb_width: float = 2.0, limb_alpha: float = 1.0, heat: Optional[torch.Tensor] = None,
                heat_colors: Optional[torch.Tensor] = None, heat_gain: float = 1.0, heat_alpha: float = 0.5,
                ids: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None, alpha: int = 128, contour: bool = True,
                radius: Optional[int] = None, dots: bool = True, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """render_frames with a pose: the overlay, then the heat maps `heat` (T, K, H, W) float32 | float64 blended in
    with heat_colors (K, 3) uint8 (None: viz.track_colors(K)), then the limbs of skeleton (E, 2) integer joint indices (numpy, a list or a
    tensor; checked on the host, so a device tensor is read back: pass a host table where that matters) `limb_width`
    (1 .. 16) pixels wide in limb_colors (E, 3) uint8 (None: the colour of each edge's second joint), then (dots=True) the dots --
    viz.render(skeleton=..., heat=...)'s host backend bit for bit, in one launch of fgvc_render_pose_u8 on the current stream.  The maps
    are read through their frame, channel and row strides (a time slice, a channel-strided view or a window is not copied; a row's values
    must be contiguous).  Every other argument is render_frames'; with dots=False `radius` is not used.  Neither skeleton nor heat: the
    bytes of render_frames."""
    from . import viz
    if skeleton is not None and tracks is None:
        raise ValueError("skeleton: needs tracks (P, T, 2), got None")
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"frames_u8: (T, H, W, 3), got {tuple(frames_u8.shape)}")
    dev = frames_u8.device
    T, H, W, _ = frames_u8.shape
    P = tracks.shape[0] if tracks is not None and tracks.dim() == 3 else 0
    maps = (None, 0, 0, 0, 0, 0, None, 1.0, 0.0)                                              # the entry's arguments from `heat` on
    if heat is not None:
        gain, h_alpha = viz._check_heat_consts(heat_gain, heat_alpha)
        if not isinstance(heat, torch.Tensor) or heat.device != dev:
            raise ValueError(f"heat: a tensor on {dev} with the frames")
        if heat.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"heat: expected float32 or float64, got {heat.dtype}")
        if heat.dim() != 4 or (heat.shape[0], heat.shape[2], heat.shape[3]) != (T, H, W):
            raise ValueError(f"heat: ({T}, K, {H}, {W}) to go with the frames, got {tuple(heat.shape)}")
        K = heat.shape[1]
        if not 1 <= K <= viz.MAX_HEAT_MAPS:
            raise ValueError(f"heat: K={K} maps (1 .. {viz.MAX_HEAT_MAPS})")
        if heat.numel() and (heat.stride(3) != 1 or heat.stride(2) < W or min(heat.stride(0), heat.stride(1)) < 0):
            heat = heat.contiguous()
        if heat_colors is None:
            heat_colors = torch.from_numpy(viz.track_colors(K)).to(dev)
        if heat_colors.dtype != torch.uint8:
            raise TypeError(f"heat_colors: expected torch.uint8, got {heat_colors.dtype}")
        if tuple(heat_colors.shape) != (K, 3) or heat_colors.device != dev:
            raise ValueError(f"heat_colors: {(K, 3)} on {dev} to go with the maps, got {tuple(heat_colors.shape)} on {heat_colors.device}")
        heat_colors = heat_colors.contiguous()
        maps = (_ptr(heat), int(heat.dtype == torch.float64), K, heat.stride(0), heat.stride(1), heat.stride(2), _ptr(heat_colors), gain, h_alpha)
    E = 0
    if skeleton is not None:
        lw, l_alpha = viz._check_limb_consts(limb_width, limb_alpha)
        # the table is checked on the host (the kernel skips, never reads, an edge outside 0 .. P - 1) and kept on the device per distinct
        # table: a skeleton given as numpy or a list costs no transfer after its first call; a device tensor is read back every call
        host = skeleton.detach().cpu().numpy() if isinstance(skeleton, torch.Tensor) else skeleton
        edges = viz._check_skeleton(host, P)
        E = edges.shape[0]
        sk = _render_table(("skeleton", edges.tobytes()), dev, lambda: edges) if E else None
        if limb_colors is not None:
            if limb_colors.dtype != torch.uint8:
                raise TypeError(f"limb_colors: expected torch.uint8, got {limb_colors.dtype}")
            if tuple(limb_colors.shape) != (E, 3) or limb_colors.device != dev:
                raise ValueError(f"limb_colors: {(E, 3)} on {dev} to go with the skeleton, got {tuple(limb_colors.shape)} on {limb_colors.device}")
            limb_colors = limb_colors.contiguous()
        ro2, g, _ = viz.trail_consts(lw)
    head, out, col, hold = _render_head(frames_u8, ids, palette, alpha, contour, tracks, visibles, colors, radius, out, bool(dots))
    if head is None:
        return out
    limbs = (None, 0, None, 2.0, 1.0, 1.0, 1.0)
    if E:
        if limb_colors is None:
            limb_colors = col[sk[:, 1].long()].contiguous()                               # the colour of every edge's second joint
        limbs = (_ptr(sk), E, _ptr(limb_colors), lw, ro2, g, l_alpha)
    _lib.call("fgvc_render_pose_u8", *head, *limbs, *maps, _stream(out))
    return out


def render_boxes(frames_u8: torch.Tensor, boxes: torch.Tensor, box_visibles: Optional[torch.Tensor] = None,
                 box_colors: Optional[torch.Tensor] = None, box_width: int = 2, box_alpha: int = 255, box_labels: Optional[torch.Tensor] = None,
                 label_scale: int = 1, ids: Optional[torch.Tensor] = None, palette: Optional[torch.Tensor] = None, alpha: int = 128,
                 contour: bool = True, tracks: Optional[torch.Tensor] = None, visibles: Optional[torch.Tensor] = None,
                 colors: Optional[torch.Tensor] = None, radius: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """render_frames with boxes: the overlay, then box i of boxes (T, N, 4) integer (x0, y0, x1, y1), half-open, as a
    ring `box_width` (1 .. 16) pixels wide outside the box in box_colors[i] ((N, 3) uint8; None: palette[i]) at opacity box_alpha
    (0 .. 256), with a tag of the decimal digits of box_labels[i] ((N,) integers 0 .. 999; None: no tags) at label_scale (1 .. 4), then the
    dots -- viz.render(boxes=...)'s host backend bit for bit, in one launch of fgvc_render_boxes_u8 on the current stream.  box_visibles
    (T, N) bool or uint8, None: all; an empty box draws nothing.  N <= 255; a coordinate of 2**20 or more in magnitude is refused (one
    host read of a flag).  Every tensor is on the frames' device; every other argument is render_frames'."""
    from . import viz
    if frames_u8.dim() != 4 or frames_u8.shape[3] != 3:
        raise ValueError(f"frames_u8: (T, H, W, 3), got {tuple(frames_u8.shape)}")
    dev = frames_u8.device
    T = frames_u8.shape[0]
    if not isinstance(boxes, torch.Tensor) or boxes.device != dev:
        raise ValueError(f"boxes: a tensor on {dev} with the frames")
    if boxes.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise TypeError(f"boxes: expected an integer type, got {boxes.dtype}")
    if boxes.dim() != 3 or boxes.shape[0] != T or boxes.shape[2] != 4:
        raise ValueError(f"boxes: ({T}, N, 4) to go with the frames, got {tuple(boxes.shape)}")
    N = boxes.shape[1]
    if N > viz.MAX_BOXES:
        raise ValueError(f"boxes: N={N} boxes a frame (0 .. {viz.MAX_BOXES})")
    if boxes.numel() and bool((boxes.long().abs() >= viz.BOX_LIMIT).any()):
        raise ValueError("boxes: coordinates below 2**20 in magnitude")
    b = boxes.to(torch.int32).contiguous()
    bw = viz._int_in(box_width, viz.BOX_WIDTHS[0], viz.BOX_WIDTHS[1], "box_width")
    b_alpha = viz._int_in(box_alpha, 0, 256, "box_alpha")
    scale = viz._int_in(label_scale, viz.LABEL_SCALES[0], viz.LABEL_SCALES[1], "label_scale")
    vis = None
    if box_visibles is not None:
        if box_visibles.dtype not in (torch.bool, torch.uint8):
            raise TypeError(f"box_visibles: expected torch.bool (or uint8), got {box_visibles.dtype}")
        if tuple(box_visibles.shape) != (T, N) or box_visibles.device != dev:
            raise ValueError(f"box_visibles: {(T, N)} on {dev} to go with the boxes, got {tuple(box_visibles.shape)} on {box_visibles.device}")
        vis = (box_visibles.view(torch.uint8) if box_visibles.dtype == torch.bool else box_visibles).contiguous()
    if box_colors is None:
        pal = _render_table("palette", dev, viz.davis_palette) if palette is None else palette
        if pal.dtype != torch.uint8 or tuple(pal.shape) != (256, 3) or pal.device != dev:
            raise ValueError(f"palette: (256, 3) uint8 on {dev} (box_colors=None takes palette[i])")
        box_colors = pal[:N]
    if box_colors.dtype != torch.uint8:
        raise TypeError(f"box_colors: expected torch.uint8, got {box_colors.dtype}")
    if tuple(box_colors.shape) != (N, 3) or box_colors.device != dev:
        raise ValueError(f"box_colors: {(N, 3)} on {dev} to go with the boxes, got {tuple(box_colors.shape)} on {box_colors.device}")
    col = box_colors.contiguous()
    labels = digits = None
    if box_labels is not None:
        if not isinstance(box_labels, torch.Tensor) or box_labels.device != dev or box_labels.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"box_labels: an int32 or int64 tensor on {dev} with the frames")
        if tuple(box_labels.shape) != (N,):
            raise ValueError(f"box_labels: {N} integers in 0 .. {viz.MAX_LABEL}, got {tuple(box_labels.shape)}")
        if N and bool(((box_labels < 0) | (box_labels > viz.MAX_LABEL)).any()):
            raise ValueError(f"box_labels: integers in 0 .. {viz.MAX_LABEL}")
        labels = box_labels.to(torch.int32).contiguous()
        digits = _render_table("digits5x7", dev, lambda: viz.DIGITS_5X7)
    head, out, _, hold = _render_head(frames_u8, ids, palette, alpha, contour, tracks, visibles, colors, radius, out)
    if head is not None:
        _lib.call("fgvc_render_boxes_u8", *head, _ptr(b) if N else None, b.stride(0), None if vis is None else _ptr(vis), 0 if vis is None else vis.stride(0),
                  _ptr(col) if N else None,
                  N, bw, b_alpha, None if labels is None else _ptr(labels), scale, None if digits is None else _ptr(digits), _stream(out))
    return out
