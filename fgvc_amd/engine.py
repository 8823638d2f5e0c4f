"""Label-propagation engine: the schedule the reference's driver runs frame by frame
(vanilla_tracker.py:305-412), restated as three device phases.

  phase 1  correlation + top-k for EVERY (query frame, key frame) pair of the clip in one launch
           (indices/scores depend on features only, so all frames go in parallel);
  phase 2  per output frame: merge its key slots' lists, temperature, softmax   (one launch);
  phase 3  the only sequential part: label propagation frame by frame (tiny gathers), then the
           fused upsample + soft-argmax read-out.

`plan_*` are pure host functions (tested on CPU); `run_*` enqueue HIP work and never synchronise.

De-duplication: the reference re-encodes and re-correlates the whole tail of
the clip once per distinct query time t0 (vanilla_tracker.py:249-295).  A (query frame, key frame)
pair's top-k does not depend on t0, and top-k of a union of slots == top-k of the union of the
slots' top-k lists, so pairs are computed ONCE and every group merges the pairs it needs;
frame t0 in slot 0 and again as a preceding frame (:353-362) costs one pair, not two.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import ops
from .ops import MaskSpec


@dataclass
class TrackerConfig:
    """test_cfg_<task> keys the path reads (configs/eval/res18_d1_eval.py:12-58, vanilla_tracker.py:246,330-392).

    The reference reads `with_first` twice with DIFFERENT defaults: `.get('with_first', False)` decides whether points are
    regrouped by query time (:246) and `.get('with_first', True)` whether the group's first frame is key slot 0 (:353).
    They are two fields here (`regroup`, `with_first`) so that a config without the key behaves as the reference does:
    one group from frame 0, first frame in slot 0."""
    precede_frames: int = 5
    topk: int = 10
    temperature: float = 0.07
    neighbor_range: Optional[int] = 30
    mask_mode: str = "circle"
    with_first: bool = True            # key slot 0 = first frame of the group (:353)
    regroup: bool = False              # one pass per distinct query time (:246)
    with_first_neighbor: bool = True
    with_norm: bool = True
    mode: str = "softmax"
    sim_mode: str = "dot_product"      # or 'l2-distance' (local_attention.py:324-327), normalised features only
    test_mode: str = "v1"              # anything else = masked_attention_efficient_v2 (:379-392)
    sigma: float = 6.0
    pair_precision: str = "auto"   # ops.pair_topk_auto: "auto" | "f32" | "split" (not a reference key)
    pair_split_fmt: str = "f16"    # operand format of the split pair kernel: "f16" = split_f16x2 rows -> fgvc_pair_topk_f16x3 (three f16 products, 1e-7-grade),
                                   # "f16f6" = split_f16f6p rows -> fgvc_pair_topk_f16f6 (f16 + FP6 cross terms: half the matrix work, ~6e-5 logit);
                                   # VanillaTracker picks "f16f6" when its encoder computes in f16f8 / f16f6 and the mask allows it (engine_config)
    pair_refine: bool = True       # with "f16f6": the bank carries the exact f32 channels behind every row (split_f16f6x: 2 KiB rows) and the
                                   # merge re-scores near-ties from them (fgvc_merge_refine_topk_f32): the lists are the exact top-k in the exact
                                   # order wherever the approximate scores are within `pair_refine_eps` of the exact products (round 5: the
                                   # reference's own lists, profiles/r05_precision_ledger.json).  False: round 4's plain merge of approximate scores
    pair_refine_eps: float = ops.REFINE_EPS
    hard_prop: bool = False        # mask path: a frame's bank row is one_hot(argmax) of its logits (vanilla_tracker.py:81, :763-769)
    norm_mask: bool = True         # mask path: per-channel min-max normalisation before the argmax (vanilla_tracker.py:82, :787-797)

    @staticmethod
    def from_test_cfg(cfg) -> "TrackerConfig":
        """Every key the reference's driver reads is either honoured or refused loudly -- never dropped."""
        g = cfg.get
        neighbor_range, mask_mode = g("neighbor_range", None), g("mask_mode", "circle")
        with_first_neighbor = g("with_first_neighbor", True)
        test_mode = g("test_mode", "v1")
        if test_mode != "v1":
            # masked_attention_efficient_v2: always the disc `dist < neighbor_range // 2` (local_attention.py:463-467), on every
            # key slot (non_mask_len is accepted and ignored there, :467-470); `mask_mode` is not read on this branch
            if neighbor_range is None:
                raise ValueError("test_mode != 'v1' needs neighbor_range (vanilla_tracker.py:384 computes neighbor_range // 2)")
            mask_mode, with_first_neighbor = "circle", True
        # (_v2 accepts `sim_mode` and never reads it, local_attention.py:453-455)
        sim_mode = g("sim_mode", "dot_product") if test_mode == "v1" else "dot_product"
        with_norm = g("with_norm", True)
        if sim_mode not in ("dot_product", "l2-distance"):
            raise NotImplementedError(f"fgvc_amd: sim_mode={sim_mode!r} (the reference knows 'dot_product' and 'l2-distance')")
        if sim_mode == "l2-distance" and not with_norm:
            raise NotImplementedError("fgvc_amd: sim_mode='l2-distance' is on the accelerated path for normalised features only")
        return TrackerConfig(
            precede_frames=g("precede_frames", 5), topk=g("topk", 10), temperature=g("temperature", 0.07),
            neighbor_range=neighbor_range, mask_mode=mask_mode,
            with_first=bool(g("with_first", True)), regroup=bool(g("with_first", False)),
            with_first_neighbor=with_first_neighbor, with_norm=with_norm, sim_mode=sim_mode, test_mode=test_mode,
            pair_precision=g("pair_precision", "auto"), pair_split_fmt=g("pair_split_fmt", "f16"),   # from here on: extension keys
            pair_refine=bool(g("pair_refine", True)), pair_refine_eps=float(g("pair_refine_eps", ops.REFINE_EPS)),
            hard_prop=bool(g("hard_prop", False)), norm_mask=bool(g("norm_mask", True)))

    @property
    def bank_fmt(self) -> str:
        """The format get_feats_hwc(split=True) / run_pairs() build the bank in: split_f16f6x() rows where the f16 + FP6 pair kernel runs
        with the refining merge behind it, else what `pair_split_fmt` names."""
        return "f16f6x" if (self.pair_split_fmt == "f16f6" and self.pair_refine) else self.pair_split_fmt

    @property
    def mask(self) -> MaskSpec:
        return MaskSpec.from_neighbor_range(self.neighbor_range, self.mask_mode)

    def softmax_temperature(self, channels: int) -> float:
        """Divisor of the raw dot products of L2-normalised rows before the softmax over the k survivors.
        'l2-distance' (local_attention.py:324-327): affinity = (2 k.q - |k|^2) / sqrt(C) with |k| = 1, no temperature: the
        same ranking as the dot product, and softmax((2 d - 1) / sqrt(C)) = softmax(d / (sqrt(C) / 2))."""
        if self.sim_mode == "l2-distance":
            if self.mode != "softmax":
                raise NotImplementedError("fgvc_amd: sim_mode='l2-distance' with mode='cosine'")
            return math.sqrt(channels) / 2.0
        return float(self.temperature)


def key_slots(frame: int, start: int, precede_frames: int, with_first: bool) -> List[int]:
    """Clip-absolute key frames of query frame `frame` in the group that starts at `start`
    (vanilla_tracker.py:346-362 with frame numbers shifted by `start`)."""
    ks = list(range(max(start, frame - precede_frames), frame))
    return ([start] + ks) if with_first else ks


@dataclass
class Plan:
    """Host-side schedule for one clip."""
    n_frames: int
    starts: List[int]                                   # distinct query times, ascending
    pairs: List[Tuple[int, int, bool]]                  # unique (query frame, key frame, masked)
    out_rows: Dict[Tuple[int, int], int]                # (start, frame) -> row of slot tables
    slot_pair: List[List[int]]                          # row -> pair id per key slot (-1 pad)
    slot_frame: List[List[int]]                         # row -> clip frame per key slot (0 pad)
    t_max: int = 0
    _dev: Dict[str, tuple] = field(default_factory=dict, repr=False)

    def tables(self, dev):
        """Device copies of the schedule (pairs int32 (n,4), slot_pair / slot_frame int32 (rows,t_max)).
        A plan depends only on (n_frames, starts, cfg), so the tables are uploaded once and reused."""
        key = str(dev)
        if key not in self._dev:
            rows = len(self.slot_pair)
            self._dev[key] = (
                ops.make_pairs(self.pairs, dev),
                torch.tensor(self.slot_pair, dtype=torch.int32, device=dev).reshape(rows, self.t_max),
                torch.tensor(self.slot_frame, dtype=torch.int32, device=dev).reshape(rows, self.t_max))
        return self._dev[key]


def plan_clip(n_frames: int, starts: Sequence[int], cfg: TrackerConfig,
              frame_range: Optional[Tuple[int, int]] = None) -> Plan:
    """Build the pair list and slot tables.  `frame_range` = [lo, hi) restricts the QUERY frames
    (clip sharding across GPUs: each rank plans only its own frames)."""
    starts = sorted(set(int(s) for s in starts))
    lo, hi = frame_range if frame_range is not None else (0, n_frames)
    non_mask_len = 0 if cfg.with_first_neighbor else 1
    pair_id: Dict[Tuple[int, int, bool], int] = {}
    rows: Dict[Tuple[int, int], int] = {}
    slot_pair, slot_frame = [], []
    t_max = cfg.precede_frames + (1 if cfg.with_first else 0)
    t_max = max(t_max, 1)
    for s in starts:
        for f in range(max(s + 1, lo), min(n_frames, hi)):
            ks = key_slots(f, s, cfg.precede_frames, cfg.with_first)
            sp, sf = [], []
            for t, kf in enumerate(ks):
                masked = not (t < non_mask_len) and not cfg.mask.is_none
                key = (f, kf, masked)
                if key not in pair_id:
                    pair_id[key] = len(pair_id)
                sp.append(pair_id[key])
                sf.append(kf)
            pad = t_max - len(ks)
            rows[(s, f)] = len(slot_pair)
            slot_pair.append(sp + [-1] * pad)
            slot_frame.append(sf + [0] * pad)
    pairs = [k for k, _ in sorted(pair_id.items(), key=lambda kv: kv[1])]
    return Plan(n_frames, starts, pairs, rows, slot_pair, slot_frame, t_max)


@dataclass
class DeviceTopk:
    """phase 1+2 results on the device."""
    plan: Plan
    idx: torch.Tensor        # (rows, HW, k) int32   slot*HW + pixel
    logit: torch.Tensor      # (rows, HW, k)
    weight: torch.Tensor     # (rows, HW, k)
    slot_frame: torch.Tensor  # (rows, t_max) int32
    row_map: Optional[Dict[int, int]] = None    # plan row -> row of idx / weight / slot_frame when only some rows were merged
    refine_stats: Optional[torch.Tensor] = None # the refining merge's int32 counters (3,) on the device: queries re-scored, of them from scratch, candidates

    def row(self, plan_row: int) -> int:
        return plan_row if self.row_map is None else self.row_map[plan_row]


@dataclass
class PairLists:
    """phase 1 results on the device: per (query frame, key frame) pair the top-k list of every query pixel."""
    plan: Plan
    idx: torch.Tensor        # (pairs, HW, k) int32   pixel index in the key frame
    score: torch.Tensor      # (pairs, HW, k)
    HW: int
    channels: int = 256      # un-padded feature channels (only 'l2-distance' reads it)
    exact: Optional[torch.Tensor] = None    # the scores are fgvc_pair_topk_f16f6's approximations; the bank whose exact rows re-score them
    geom: Optional[Tuple[int, int]] = None  # (Hf, Wf) (the refining merge needs the grid for the mask predicate)


def run_affinity(feats_hwc: torch.Tensor, Hf: int, Wf: int, plan: Plan, cfg: TrackerConfig,
                 pair_chunk: int = 16384, events=None, phases=None, channels: Optional[int] = None) -> DeviceTopk:
    """Phases 1 and 2 (= merge_pairs(run_pairs(...)))."""
    return merge_pairs(run_pairs(feats_hwc, Hf, Wf, plan, cfg, pair_chunk, events, channels=channels, phases=phases), cfg)


def merge_pairs(pl: PairLists, cfg: TrackerConfig, rows: Optional[Sequence[int]] = None) -> DeviceTopk:
    """Phase 2: per query frame, merge the lists of its key slots and softmax the k survivors.
    `rows` = plan rows to merge (default all).  track_points merges one query-time group at a time: with strided TAP-Vid queries
    a clip has one group per distinct query time and merging every (group, frame) row at once costs rows * HW * k * 12 bytes
    (T = 250 at 128 x 128: ~6k rows, 12 GB)."""
    plan = pl.plan
    _, slot_pair, slot_frame = plan.tables(pl.idx.device)
    row_map = None
    if rows is not None:
        rows = list(rows)
        sel = torch.tensor(rows, dtype=torch.int64, device=pl.idx.device)
        slot_pair, slot_frame = slot_pair[sel].contiguous(), slot_frame[sel].contiguous()
        row_map = {r: i for i, r in enumerate(rows)}
    if slot_pair.shape[0] == 0:
        e = torch.empty((0, pl.HW, cfg.topk), device=pl.idx.device)
        return DeviceTopk(plan, e.int(), e, e, slot_frame, row_map)
    if pl.exact is not None:
        pairs_dev = plan.tables(pl.idx.device)[0]
        Hf, Wf = pl.geom
        idx, logit, weight, stats = ops.merge_refine_topk(pl.idx, pl.score, slot_pair, pairs_dev, pl.exact, pl.exact, Hf, Wf, Hf, Wf,
                                                          cfg.mask, cfg.topk, cfg.softmax_temperature(pl.channels), cfg.mode,
                                                          eps=cfg.pair_refine_eps)
        tk = DeviceTopk(plan, idx, logit, weight, slot_frame, row_map)
        tk.refine_stats = stats
        return tk
    idx, logit, weight = ops.merge_topk(pl.idx, pl.score, slot_pair, pl.HW, cfg.topk, cfg.softmax_temperature(pl.channels),
                                        cfg.mode, validate=False)
    return DeviceTopk(plan, idx, logit, weight, slot_frame, row_map)


def run_pairs(feats_hwc: torch.Tensor, Hf: int, Wf: int, plan: Plan, cfg: TrackerConfig,
              pair_chunk: int = 16384, events=None, channels: Optional[int] = None, phases=None) -> PairLists:
    """Phase 1.  feats_hwc (T, HW, C) normalised channels-last features of the whole clip, f32 -- or their
    split form (T, HW, 2, C) int16 in the format cfg.pair_split_fmt names, where the split pair kernel applies
    (VanillaTracker.get_feats_hwc(split=True)).
    `events` = (start, end) torch.cuda.Events recorded around the pair top-k launch(es); `channels` = the encoder's channel
    count where it differs from the (zero-padded) row length.
    `phases` = (first, between): the pairs whose plan indices are in `first` are launched, then `between()` is called, then the
    rest -- clip sharding launches the pairs that touch no halo frame while the halo messages are in flight and lets
    `between` make the stream wait for them (the frames of the later pairs need not be valid in `feats_hwc` before that)."""
    dev = feats_hwc.device
    HW = Hf * Wf
    k = cfg.topk
    n = len(plan.pairs)
    pairs_dev, slot_pair, slot_frame = plan.tables(dev)
    rows = len(plan.slot_pair)
    exact = None
    pre_split = feats_hwc.dtype == torch.int16            # (T, HW, 2 | 4, C): the bank already in a pair kernel's operand format
    if n == 0:                                            # a one-frame clip, or every query point on the last frame: nothing to correlate
        e = torch.empty((0, HW, k), device=dev)
        return PairLists(plan, e.int(), e, HW, feats_hwc.shape[-1] if channels is None else channels)
    all_masked = all(m for (_, _, m) in plan.pairs)
    use_split = cfg.pair_precision == "split" or (
        cfg.pair_precision == "auto" and ops.split_path_ok(feats_hwc.shape[-1], Hf, Wf, k, cfg.with_norm, None, cfg.mask, all_masked))
    if pre_split and not use_split:
        raise ValueError("run_affinity: split features given, but the split pair kernel does not apply to this configuration")
    if cfg.sim_mode == "l2-distance" and channels is None:
        # the softmax divisor of this mode is sqrt(C) / 2 with the encoder's OWN channel count (local_attention.py:327 uses
        # att_channels); the row length may be that count rounded up with zero channels (normalize_to_hwc(pad=True)), so it must be given
        raise ValueError("run_pairs: sim_mode='l2-distance' needs channels= (the encoder's un-padded channel count)")
    if use_split:      # 16-bit matrix pipe on the two-part split of the (normalised) features, f32-grade scores
        if cfg.pair_split_fmt not in ("f16", "f16f6"):
            raise ValueError(f"pair_split_fmt={cfg.pair_split_fmt!r}: 'f16' (split_f16x2 rows) or 'f16f6' (split_f16f6p / split_f16f6x rows)")
        # a pre-split bank says itself whether its rows are split_f16f6x()'s; between split_f16x2() and split_f16f6p() rows (one shape) the
        # configuration's word is all there is -- VanillaTracker.get_feats_hwc builds the bank from the same configuration
        fmt = ops.bank_format(feats_hwc, cfg.pair_split_fmt) if pre_split else cfg.bank_fmt
        if pre_split and fmt == "f16f6x" and cfg.pair_split_fmt != "f16f6":
            raise ValueError("run_pairs: the bank holds split_f16f6x() rows, but the configuration asks for pair_split_fmt='f16' "
                             "(build the bank and run the pairs from ONE configuration: VanillaTracker.engine_config())")
        if fmt != "f16" and not ops.pair_f16f6_ok(feats_hwc.shape[-1], Hf, Wf, k, cfg.with_norm, None, cfg.mask, all_masked):
            if pre_split:
                raise ValueError("run_pairs: the bank is in the f16f6 format, but fgvc_pair_topk_f16f6 does not apply to this mask / pair list "
                                 "(every pair masked, at most 64 key blocks in reach): encode with pair_split_fmt='f16'")
            fmt = "f16"
        split = feats_hwc if pre_split else {"f16": ops.split_f16x2, "f16f6": ops.split_f16f6p, "f16f6x": ops.split_f16f6x}[fmt](feats_hwc)
        if fmt == "f16f6x":
            exact = split                                 # the refining merge reads the rows' second KiB
        pair_fn = lambda prs: ops.pair_topk_split(split, split, prs, Hf, Wf, Hf, Wf, cfg.mask, k, validate=False, all_masked=all_masked,
                                                  fmt=fmt)
    else:
        pair_fn = lambda prs: ops.pair_topk(feats_hwc, feats_hwc, prs, Hf, Wf, Hf, Wf, cfg.mask, k, validate=False)
    if events is not None:
        events[0].record()
    if phases is not None:
        first, between = phases
        fs = set(int(i) for i in first)
        key = ("phases", str(dev), tuple(sorted(fs)))
        if key not in plan._dev:
            sel = [[i for i in range(n) if i in fs], [i for i in range(n) if i not in fs]]
            plan._dev[key] = [(torch.tensor(ix, dtype=torch.int64, device=dev), ops.make_pairs([plan.pairs[i] for i in ix], dev))
                              for ix in sel]
        pidx = torch.empty((n, HW, k), device=dev, dtype=torch.int32)
        pscore = torch.empty((n, HW, k), device=dev, dtype=torch.float32)
        for ph, (ix, prs) in enumerate(plan._dev[key]):
            if ph == 1:
                between()
            for c0 in range(0, prs.shape[0], pair_chunk):
                c1 = min(prs.shape[0], c0 + pair_chunk)
                i, s_ = pair_fn(prs if (c0 == 0 and c1 == prs.shape[0]) else ops.make_pairs([plan.pairs[j] for j in ix[c0:c1].tolist()], dev))
                pidx.index_copy_(0, ix[c0:c1], i)
                pscore.index_copy_(0, ix[c0:c1], s_)
    elif n <= pair_chunk:
        pidx, pscore = pair_fn(pairs_dev)
    else:
        pidx = torch.empty((n, HW, k), device=dev, dtype=torch.int32)
        pscore = torch.empty((n, HW, k), device=dev, dtype=torch.float32)
        for c0 in range(0, n, pair_chunk):
            c1 = min(n, c0 + pair_chunk)
            i, s = pair_fn(pairs_dev[c0:c1])
            pidx[c0:c1], pscore[c0:c1] = i, s
    if events is not None:
        events[1].record()
    return PairLists(plan, pidx, pscore, HW, feats_hwc.shape[-1] if channels is None else channels, exact=exact, geom=(Hf, Wf))


def run_propagation(topk: DeviceTopk, start: int, points_xy: torch.Tensor, Hf: int, Wf: int, h: int, w: int,
                    cfg: TrackerConfig, frames: Optional[Tuple[int, int]] = None,
                    labels: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Phase 3 for the group that starts at `start`.  points_xy (P,2) on the device.
    Returns (labels bank (T, HW, P) with frames < start untouched/zero, coords (T-start, P, 2) f64)."""
    plan = topk.plan
    T = plan.n_frames
    dev = points_xy.device
    P = points_xy.shape[0]
    stride = h // Hf                                            # vanilla_tracker.py:197
    if labels is None:
        labels = torch.zeros((T, Hf * Wf, P), device=dev, dtype=torch.float32)
    lo, hi = frames if frames is not None else (start + 1, T)
    if lo <= start + 1:
        ops.gaussian_labels(points_xy, Hf, Wf, stride, cfg.sigma, out=labels[start])
    for f in range(max(lo, start + 1), hi):
        row = topk.row(plan.out_rows[(start, f)])
        ops.propagate_topk(labels, topk.slot_frame[row], topk.idx[row], topk.weight[row], Hf, Wf, Hf, Wf,
                           out=labels[f])
    coords = ops.softargmax_top5(labels[start:], Hf, Wf, h, w, gauss_points=points_xy, sigma=cfg.sigma)
    return labels, coords


def run_propagation_async(topk, start: int, points_xy: torch.Tensor, Hf: int, Wf: int, h: int, w: int,
                          cfg: TrackerConfig, stream: "torch.cuda.Stream"):
    """run_propagation on a side stream: the sweep and the read-out are a chain of small launches that leave most of the GPU
    idle (0.27 ms per 480p clip); on their own stream the NEXT clip's encoder runs under them.  `topk`: a DeviceTopk, or the
    PairLists of run_pairs() -- then the merge runs on the side stream as well.  The caller's stream does not wait: returns
    (labels, coords, event) -- wait for the event (or synchronise) before reading them.  The inputs are kept from the caching
    allocator until the side stream is done with them (record_stream)."""
    cur = torch.cuda.current_stream(points_xy.device)
    stream.wait_stream(cur)
    with torch.cuda.stream(stream):
        if isinstance(topk, PairLists):
            for t in (topk.idx, topk.score, topk.exact):
                if t is not None:
                    t.record_stream(stream)
            topk = merge_pairs(topk, cfg)
        for t in (topk.idx, topk.logit, topk.weight, topk.slot_frame, points_xy):
            t.record_stream(stream)
        labels, coords = run_propagation(topk, start, points_xy, Hf, Wf, h, w, cfg)
        done = torch.cuda.Event()
        done.record(stream)
    return labels, coords, done


def track_points(feats_hwc: torch.Tensor, Hf: int, Wf: int, h: int, w: int, query_points: torch.Tensor,
                 cfg: TrackerConfig, channels: Optional[int] = None, stats_out: Optional[list] = None):
    """The whole post-encoder path for one clip.  query_points (P,3) = (t, x, y) (any device).
    Returns traj_pred (T, P', 2) f64 on the device with points re-ordered by query time (the
    reference's regrouping, vanilla_tracker.py:257-299) and `order` (P',) original indices.
    `channels`: the encoder's channel count where the rows are zero-padded beyond it (read by sim_mode='l2-distance' only).
    `stats_out`: a list that receives the refining merge's counters (DeviceTopk.refine_stats) of every group."""
    T = feats_hwc.shape[0]
    dev = feats_hwc.device
    qp = query_points.detach().to("cpu")
    times = qp[:, 0].to(torch.int64)
    starts = sorted(set(times.tolist())) if cfg.regroup else [0]
    plan = plan_clip(T, starts, cfg)
    pl = run_pairs(feats_hwc, Hf, Wf, plan, cfg, channels=channels)
    traj = torch.zeros((T, qp.shape[0], 2), device=dev, dtype=torch.float64)
    order = []
    K = 0
    for s in starts:
        sel = (times == s).nonzero().flatten() if cfg.regroup else torch.arange(qp.shape[0])
        pts = qp[sel, 1:].to(dev, torch.float32)
        topk = merge_pairs(pl, cfg, [plan.out_rows[(s, f)] for f in range(s + 1, T)])     # this group's rows only
        if stats_out is not None and topk.refine_stats is not None:
            stats_out.append(topk.refine_stats)                                          # (the refining merge's device counters, per group)
        _, coords = run_propagation(topk, s, pts, Hf, Wf, h, w, cfg)
        traj[s:, K:K + sel.numel()] = coords
        order.extend(sel.tolist())
        K += sel.numel()
    return traj, torch.tensor(order, dtype=torch.int64)


def pad_divide_by(h: int, w: int, d: int) -> Tuple[Tuple[int, int], Tuple[int, int, int, int]]:
    """common/utils.py:397-410 on sizes: ((hp, wp), (left, right, top, bottom)) -- zeros, floor(extra / 2) before, the rest after."""
    hp, wp = -(-h // d) * d, -(-w // d) * d
    lh, lw = (hp - h) // 2, (wp - w) // 2
    return (hp, wp), (lw, wp - w - lw, lh, hp - h - lh)


def _record(events: Optional[dict], key: str) -> None:
    """The label-map functions' `events`: torch.cuda.Events keyed 'labels', 'affinity', 'propagation', 'readout', 'end', each recorded
    immediately before its phase ('end' after the last one).  None: nothing is recorded."""
    if events is not None:
        events[key].record()


MAPS_BUDGET = 512 << 20           # bytes of full-resolution maps held on the device at once by softmaps_to_host


def plan_map_chunks(n_frames: int, K: int, out_shape: Tuple[int, int], itemsize: int, budget: int = MAPS_BUDGET) -> List[Tuple[int, int]]:
    """Frame ranges [(f_begin, f_end), ...] covering 0 .. n_frames, each of at most `budget` bytes of (K, h0, w0) maps."""
    frame_bytes = int(K) * int(out_shape[0]) * int(out_shape[1]) * int(itemsize)
    per = int(budget) // frame_bytes
    if per < 1:
        raise ValueError(f"maps_budget={int(budget)} bytes holds less than one frame's {K} x {out_shape[0]} x {out_shape[1]} maps "
                         f"({frame_bytes} bytes needed)")
    return [(f, min(f + per, n_frames)) for f in range(0, n_frames, per)]


def softmaps_to_host(bank: torch.Tensor, heat: torch.Tensor, Hf: int, Wf: int, map_pad: Tuple[int, int, int, int],
                     out_shape: Tuple[int, int], budget: int = MAPS_BUDGET, events: Optional[dict] = None):
    """The (T, K, h0, w0) stack of a propagated bank (propagate_soft_bank) as a numpy array, in heat's dtype.
    The read-out runs over plan_map_chunks' frame ranges into ONE reused device buffer of at most `budget` bytes; each chunk is copied
    into the host array before the buffer is written again (the copy is synchronous: no overlap with the next chunk's read-out).
    `events`: 'readout' is recorded before the first chunk and 'end' after the last copy."""
    T, K = bank.shape[0], heat.shape[0]
    chunks = plan_map_chunks(T, K, out_shape, heat.element_size(), budget)
    host = torch.empty((T, K, *out_shape), dtype=heat.dtype)
    buf = torch.empty((chunks[0][1] - chunks[0][0], K, *out_shape), device=bank.device, dtype=heat.dtype)
    _record(events, "readout")
    for f0, f1 in chunks:
        ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape, frames=(f0, f1), out=buf[:f1 - f0])
        host[f0:f1].copy_(buf[:f1 - f0])
    _record(events, "end")
    return host.numpy()


# ---- HRVanillaTracker's label maps: the local-window affinity (vanilla_tracker.py:663-830, local_attention.py:883-1006) ----------------
#
# masked_attention_efficient_correlation scores every query pixel against the (2R+1)^2 window of each key slot (mmcv.ops.Correlation,
# zero padded: a tap outside the frame scores 0 and carries label 0) and keeps the top k of K*(2R+1)^2 candidates.  Planned like the dense
# path: the clip's unique (query frame, key frame) pairs run through the pair kernel under the square window, chunk by chunk, each chunk's
# rows are merged in one launch (fgvc_local_merge_plan_f32 adds the zero taps per slot), then the frames are swept one by one.

LOCAL_PAIR_BUDGET = 512 << 20     # bytes of pair lists (idx + score) held at once: 8.2 MB per pair at 480 x 854 (240 x 427 features, k = 10)


@dataclass
class LocalConfig:
    """test_cfg keys of HRVanillaTracker.forward_test_backward_save_mem.  `temperature`, `topk` and `precede_frames` are read as
    attributes there (:728, :754-755), with no defaults; R = neighbor_range // 2 (constructor, default 24); `with_norm` (:758, default True;
    NOT the points path's `withnorm`); `with_first` (:742, default True).  hard_prop / norm_mask as the VanillaTracker mask path reads them.
    pair_precision / pair_budget are not reference keys: "auto" | "f32" | "split" as TrackerConfig's, and the pair-list byte budget."""
    temperature: float
    topk: int
    precede_frames: int
    radius: int = 12
    with_first: bool = True
    with_norm: bool = True
    hard_prop: bool = False
    norm_mask: bool = True
    pair_precision: str = "auto"
    pair_budget: int = LOCAL_PAIR_BUDGET

    @property
    def mask(self) -> MaskSpec:
        return MaskSpec(ry=self.radius, rx=self.radius)

    @property
    def window(self) -> int:
        return 2 * self.radius + 1


@dataclass
class LocalPlan:
    """Host-side schedule of one clip on the local window.  Row r = output frame r + 1."""
    n_frames: int
    pairs: List[Tuple[int, int]]                 # unique (query frame, key frame), grouped by row
    slot_pair: List[List[int]]                   # row -> pair per key slot position (-1 pad)
    slot_frame: List[List[int]]                  # row -> clip frame per key slot position (0 pad)
    t_max: int
    chunks: List[Tuple[int, int, int, int]]      # (row0, row1, pair0, pair1): rows and the pairs they own, one pair launch + one merge each
    pair_bytes: int                              # bytes of one pair's lists
    _dev: Dict[str, tuple] = field(default_factory=dict, repr=False)

    def tables(self, dev):
        """Per chunk (pairs int32 (n,4), slot_pair int32 (rows, t_max) relative to the chunk's first pair), and slot_frame (rows, t_max)."""
        key = str(dev)
        if key not in self._dev:
            per = []
            for r0, r1, p0, p1 in self.chunks:
                rel = [[p - p0 if p >= 0 else -1 for p in row] for row in self.slot_pair[r0:r1]]
                per.append((ops.make_pairs([(f, s, True) for f, s in self.pairs[p0:p1]], dev),
                            torch.tensor(rel, dtype=torch.int32, device=dev).reshape(r1 - r0, self.t_max)))
            sf = torch.tensor(self.slot_frame, dtype=torch.int32, device=dev).reshape(len(self.slot_frame), self.t_max)
            self._dev[key] = (per, sf)
        return self._dev[key]


def plan_local_clip(n_frames: int, cfg: LocalConfig, HW: int) -> LocalPlan:
    """Key slots of frame f (vanilla_tracker.py:728-745): frame 0 when with_first, then key_start .. f-1 with key_start =
    max(0, f - precede_frames) -- duplicates kept (frame 1: [0, 0]), one pair for both.  Rows are chunked so that a chunk's pair lists
    (HW * topk * 8 bytes per pair) stay within cfg.pair_budget."""
    pre = int(cfg.precede_frames)
    t_max = max(1, pre + (1 if cfg.with_first else 0))
    pair_bytes = HW * int(cfg.topk) * 8
    pairs: List[Tuple[int, int]] = []
    slot_pair, slot_frame, row_pairs = [], [], []
    for f in range(1, n_frames):
        ks = key_slots(f, 0, pre, cfg.with_first)
        own: Dict[int, int] = {}
        for kf in ks:
            if kf not in own:
                own[kf] = len(pairs)
                pairs.append((f, kf))
        row_pairs.append(len(own))
        slot_pair.append([own[kf] for kf in ks] + [-1] * (t_max - len(ks)))
        slot_frame.append(list(ks) + [0] * (t_max - len(ks)))
    chunks, r0, p0, n = [], 0, 0, 0
    for r, m in enumerate(row_pairs):
        if m * pair_bytes > cfg.pair_budget:
            raise ValueError(f"pair_budget={cfg.pair_budget} bytes holds less than one frame's {m} pair lists ({m * pair_bytes} bytes)")
        if (n + m) * pair_bytes > cfg.pair_budget:
            chunks.append((r0, r, p0, p0 + n))
            r0, p0, n = r, p0 + n, 0
        n += m
    if row_pairs:
        chunks.append((r0, len(row_pairs), p0, p0 + n))
    return LocalPlan(n_frames, pairs, slot_pair, slot_frame, t_max, chunks, pair_bytes)


def local_route(feats_hwc: torch.Tensor, Hf: int, Wf: int, cfg: LocalConfig) -> str:
    """'f16x3' (fgvc_pair_topk_f16x3 on split_f16x2 rows) where ops.split_path_ok holds, else 'f32'; an int16 bank IS split_f16x2 rows."""
    if cfg.pair_precision not in ("auto", "f32", "split"):
        raise ValueError(f"pair_precision={cfg.pair_precision!r}")
    ok = ops.split_path_ok(feats_hwc.shape[-1], Hf, Wf, cfg.topk, cfg.with_norm, None, cfg.mask, True)
    if feats_hwc.dtype == torch.int16 or cfg.pair_precision == "split":
        if not ok:
            raise ValueError("the f16x3 local window needs normalised 256-channel rows, topk <= 10 and a window within the kernel's block list")
        return "f16x3"
    return "f16x3" if (ok and cfg.pair_precision == "auto") else "f32"


def run_local_affinity(feats_hwc: torch.Tensor, Hf: int, Wf: int, plan: LocalPlan, cfg: LocalConfig,
                       stats: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Every row's top-k over its slots' windows: idx (rows, HW, k) int32 = slot position * L^2 + tap, logit, weight.
    feats_hwc (T, HW, C) f32 rows (L2-normalised iff cfg.with_norm), or their split_f16x2 form (T, HW, 2, 256) int16; a f32 bank on the
    f16x3 route is split ONCE here.  `stats`: receives 'route', 'chunks' and 'workspace_bytes' (the largest chunk's pair lists)."""
    dev, HW, k, R = feats_hwc.device, Hf * Wf, int(cfg.topk), int(cfg.radius)
    rows = len(plan.slot_pair)
    idx = torch.empty((rows, HW, k), device=dev, dtype=torch.int32)
    logit = torch.empty((rows, HW, k), device=dev, dtype=torch.float32)
    weight = torch.empty_like(logit)
    route = local_route(feats_hwc, Hf, Wf, cfg)
    if route == "f16x3":
        bank = feats_hwc if feats_hwc.dtype == torch.int16 else ops.split_f16x2(feats_hwc)
        pair_fn = lambda prs: ops.pair_topk_split(bank, bank, prs, Hf, Wf, Hf, Wf, cfg.mask, k, validate=False, all_masked=True, fmt="f16")
    else:
        pair_fn = lambda prs: ops.pair_topk(feats_hwc, feats_hwc, prs, Hf, Wf, Hf, Wf, cfg.mask, k, validate=False)
    per, _ = plan.tables(dev)
    for (r0, r1, p0, p1), (prs, sp) in zip(plan.chunks, per):
        pidx, pscore = pair_fn(prs)
        ops.local_merge_plan(pidx, pscore, sp, Hf, Wf, R, k, float(cfg.temperature), out=(idx[r0:r1], logit[r0:r1], weight[r0:r1]))
        del pidx, pscore
    if stats is not None:
        stats.update(route=route, chunks=len(plan.chunks),
                     workspace_bytes=max((p1 - p0) * plan.pair_bytes for _, _, p0, p1 in plan.chunks) if plan.chunks else 0)
    return idx, logit, weight


# ---- label maps: one sweep, two affinities (vanilla_tracker.py:663-830) -------------------------------------------------------------------
#
# Masks, heat maps and soft maps are one algorithm: seed frame 0's labels, compute the affinity, sweep frames 1 .. T-1, read out.  The
# configuration's type picks the affinity: a TrackerConfig VanillaTracker's dense (disc-masked) one (:366-378), a LocalConfig
# HRVanillaTracker's local window.  Keywords every entry point takes:
#   channels, stats_out   dense only: the encoder's un-padded channel count (run_pairs), and a list that receives the refining merge's
#                         counters (DeviceTopk.refine_stats).  The local window reads neither and appends nothing;
#   affinity_stats        local only: run_local_affinity's `stats` dict.  The dense affinity leaves it alone;
#   events                _record's.

@dataclass
class LabelSweep:
    """What the sweep reads: output frame f takes row f - 1 of each tensor."""
    slot_frame: torch.Tensor   # (T-1, t_max) int32  clip frame per key slot
    idx: torch.Tensor          # (T-1, HW, k) int32  slot*HW + pixel (dense), slot * L^2 + tap (local window)
    weight: torch.Tensor       # (T-1, HW, k)
    window_L: int              # 0 = dense candidates, else the window's side L = cfg.window


def label_affinity(feats_hwc: torch.Tensor, Hf: int, Wf: int, T: int, cfg, channels: Optional[int] = None,
                   stats_out: Optional[list] = None, affinity_stats: Optional[dict] = None) -> LabelSweep:
    """The affinity of a clip whose labels all start at frame 0, on the route `cfg`'s type names."""
    if isinstance(cfg, LocalConfig):
        plan = plan_local_clip(T, cfg, Hf * Wf)
        idx, _, weight = run_local_affinity(feats_hwc, Hf, Wf, plan, cfg, affinity_stats)
        return LabelSweep(plan.tables(feats_hwc.device)[1], idx, weight, cfg.window)
    plan = plan_clip(T, [0], cfg)
    tk = run_affinity(feats_hwc, Hf, Wf, plan, cfg, channels=channels)
    if stats_out is not None and tk.refine_stats is not None:
        stats_out.append(tk.refine_stats)
    assert [tk.row(plan.out_rows[(0, f)]) for f in range(1, T)] == list(range(T - 1))     # one group from frame 0: row f - 1 is frame f
    return LabelSweep(tk.slot_frame, tk.idx, tk.weight, 0)


def _sweep_labels(bank: torch.Tensor, soft: torch.Tensor, sw: LabelSweep, Hf: int, Wf: int, hard_prop: bool = False) -> None:
    """Frames 1.. in order: soft[f] = top-k weights x the label bank of the row's slot frames; under hard_prop bank[f] = one_hot(argmax) of
    it (vanilla_tracker.py:81, :763-769), else `soft` is `bank`."""
    for f in range(1, bank.shape[0]):
        ops.propagate_topk(bank, sw.slot_frame[f - 1], sw.idx[f - 1], sw.weight[f - 1], Hf, Wf, Hf, Wf, window_L=sw.window_L, out=soft[f])
        if hard_prop:
            ops.seg_hard_onehot(soft[f], out=bank[f])


# ---- the edge-aware read-out (test_cfg.readout, an extension key) ---------------------------------------------------
#
# The plain read-out interpolates the label grid and never looks at the frames.  type='guided' weighs the cells around an output pixel by
# how close they are AND by how close their mean colour is to the pixel's own (joint bilateral upsampling), so that a label edge snaps to
# the image edge beside it.  guided_readout_host states the rule in float64; ops.seg_readout_guided runs it in one kernel.

READOUT_TYPES = ("bilinear", "guided")
READOUT_RADII = (1, 2, 3)


@dataclass
class ReadoutConfig:
    """test_cfg.readout = dict(type='guided', radius=2, sigma_space=1.0, sigma_range=0.1), parsed.  The default sigmas are untuned."""
    type: str = "guided"
    radius: int = 2
    sigma_space: float = 1.0
    sigma_range: float = 0.1


def check_guided_args(Hf: int, Wf: int, pad_shape: Tuple[int, int], radius, sigma_space, sigma_range, name: str = "readout") -> None:
    """The refusals the host rule and the parser share, each by name (ValueError)."""
    if isinstance(radius, bool) or not isinstance(radius, int) or radius not in READOUT_RADII:
        raise ValueError(f"{name}: radius={radius!r} (an integer, one of {READOUT_RADII})")
    for key, v in (("sigma_space", sigma_space), ("sigma_range", sigma_range)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
            raise ValueError(f"{name}: {key}={v!r} (a positive finite number)")
    if pad_shape is not None:
        hp, wp = pad_shape
        if Hf <= 0 or Wf <= 0 or hp % Hf or wp % Wf:
            raise ValueError(f"{name}: the feature grid {Hf} x {Wf} does not divide the padded frame {hp} x {wp}")


def parse_readout(spec) -> Optional[ReadoutConfig]:
    """None or dict(type='bilinear') -> None (today's read-out, byte for byte).  dict(type='guided', ...) -> ReadoutConfig; an unknown
    type, key or value raises ValueError by name, a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError(f"test_cfg.readout: a dict such as dict(type='guided', radius=2), got {type(spec).__name__}")
    spec = dict(spec)
    kind = spec.pop("type", None)
    if kind not in READOUT_TYPES:
        raise ValueError(f"test_cfg.readout: type={kind!r} (one of {READOUT_TYPES})")
    allowed = ("radius", "sigma_space", "sigma_range") if kind == "guided" else ()
    unknown = sorted(k for k in spec if k not in allowed)
    if unknown:
        raise ValueError(f"test_cfg.readout: unknown key(s) {unknown} for type={kind!r} (type" + "".join(f", {k}" for k in allowed) + ")")
    if kind == "bilinear":
        return None
    rc = ReadoutConfig("guided", spec.get("radius", 2), spec.get("sigma_space", 1.0), spec.get("sigma_range", 0.1))
    check_guided_args(1, 1, None, rc.radius, rc.sigma_space, rc.sigma_range, "test_cfg.readout")
    return ReadoutConfig("guided", int(rc.radius), float(rc.sigma_space), float(rc.sigma_range))


@dataclass
class GuidedReadout:
    """What guided_readout_host returns, all on the host."""
    ids: torch.Tensor        # (n, h0, w0) uint8   argmax over C, the first maximum wins
    conf: torch.Tensor       # (n, h0, w0) uint8   rint(255 * clamp(best - second, 0, 1)), 255 where C == 1
    margin: torch.Tensor     # (n, h0, w0) float64 best - second (inf where C == 1)
    values: torch.Tensor     # (n, h0, w0, C) float64 the filtered channel values
    e_min: torch.Tensor      # (n, h0, w0) float64 the smallest exponent among each pixel's taps


def guided_readout_host(labels: torch.Tensor, guide: torch.Tensor, Hf: int, Wf: int, pad_shape: Tuple[int, int],
                        pad: Tuple[int, int, int, int], out_shape: Tuple[int, int], norm: bool = True, radius: int = 2,
                        sigma_space: float = 1.0, sigma_range: float = 0.1, shift: float = 0.0) -> GuidedReadout:
    """The edge-aware read-out in float64 torch on the CPU: the contract ops.seg_readout_guided is held to.

    labels (n, Hf*Wf, C): what seg_readout takes.  guide (n, 3, hp, wp): the padded Lab-normalised frames the encoder read; its values are
    ASSUMED FINITE (as the labels are), nothing is promised otherwise.  (hp, wp) = pad_shape must be whole multiples of (Hf, Wf);
    pad = (left, right, top, bottom); out_shape = (h0, w0).  Per frame:
      cell colours   Gc[i, j] = the mean of the guide over the cell's (hp / Hf) x (wp / Wf) pixel block;
      normalisation  (norm) per channel (L - min) / (max - min + 1e-12) where max > 0, else L: seg_readout's rule, but with the extremes
                     taken over the FEATURE GRID, not over the interpolated full-resolution map (the filter below is a convex combination,
                     so the affine map may be applied to the cell values first; the two read-outs therefore normalise slightly differently);
      position       py = clamp((y + 0.5) hu / h0 - 0.5, 0, hu - 1) + top with hu the unpadded height, px alike; I = the guide sampled
                     bilinearly at (py, px); fy = (py + 0.5) Hf / hp - 0.5, fx alike; centre cell (floor(fy + 0.5), floor(fx + 0.5));
      taps           the (2 radius + 1)^2 cells around the centre cell that lie inside the grid:
                     e = ((i - fy)^2 + (j - fx)^2) / (2 sigma_space^2) + |I - Gc[i, j]|^2 / (2 sigma_range^2) (+ shift),
                     w = exp(-(e - e_min)), e_min the smallest e of the pixel: the ratio is unchanged and the denominator is >= 1;
      value          sum(w L) / sum(w) per channel; id = argmax, the first maximum wins; conf as seg_readout_conf defines it.
    `shift` is added to every exponent; it cancels (a test's handle on exactly that)."""
    (hp, wp), (lw, uw, lh, uh), (h0, w0) = (int(v) for v in pad_shape), (int(v) for v in pad), (int(v) for v in out_shape)
    check_guided_args(Hf, Wf, (hp, wp), radius, sigma_space, sigma_range, "guided_readout_host")
    labels, guide = labels.detach().cpu().double(), guide.detach().cpu().double()
    n, HW, C = labels.shape
    if HW != Hf * Wf or tuple(guide.shape) != (n, 3, hp, wp):
        raise ValueError(f"guided_readout_host: labels {tuple(labels.shape)} / guide {tuple(guide.shape)} against ({n}, {Hf * Wf}, C) / "
                         f"({n}, 3, {hp}, {wp})")
    hu, wu = hp - lh - uh, wp - lw - uw
    if hu <= 0 or wu <= 0 or min(lh, uh, lw, uw) < 0:
        raise ValueError("guided_readout_host: the unpadded window must lie inside the padded frame")
    sy, sx = hp // Hf, wp // Wf
    Gc = guide.reshape(n, 3, Hf, sy, Wf, sx).mean((3, 5))                                  # (n, 3, Hf, Wf)
    L = labels.reshape(n, Hf, Wf, C)
    if norm:
        mn, mx = L.amin((1, 2), keepdim=True), L.amax((1, 2), keepdim=True)
        L = torch.where(mx > 0, (L - mn) / (mx - mn + 1e-12), L)

    def axis(n_out, n_un, off, n_pad, n_cells):
        o = torch.arange(n_out, dtype=torch.float64)
        p = ((o + 0.5) * n_un / n_out - 0.5).clamp(0, n_un - 1) + off
        f = (p + 0.5) * n_cells / n_pad - 0.5
        p0 = torch.floor(p).long().clamp(max=n_pad - 1)
        return p0, (p0 + 1).clamp(max=n_pad - 1), p - p0, f, torch.floor(f + 0.5).long()

    y0, y1, ly, fy, cy = axis(h0, hu, lh, hp, Hf)
    x0, x1, lx, fx, cx = axis(w0, wu, lw, wp, Wf)
    ly, lx = ly[None, :, None], lx[None, None, :]
    ids = torch.empty((n, h0, w0), dtype=torch.uint8)
    conf = torch.empty((n, h0, w0), dtype=torch.uint8)
    margin = torch.empty((n, h0, w0), dtype=torch.float64)
    values = torch.empty((n, h0, w0, C), dtype=torch.float64)
    e_min = torch.empty((n, h0, w0), dtype=torch.float64)
    for f in range(n):
        g = guide[f]
        I = ((1 - ly) * ((1 - lx) * g[:, y0][:, :, x0] + lx * g[:, y0][:, :, x1])
             + ly * ((1 - lx) * g[:, y1][:, :, x0] + lx * g[:, y1][:, :, x1]))             # (3, h0, w0)
        E, taps = [], []
        for a in range(-radius, radius + 1):
            i = cy + a
            for b in range(-radius, radius + 1):
                j = cx + b
                inside = ((i >= 0) & (i < Hf))[:, None] & ((j >= 0) & (j < Wf))[None, :]
                ic, jc = i.clamp(0, Hf - 1), j.clamp(0, Wf - 1)
                e = (((i - fy) ** 2)[:, None] + ((j - fx) ** 2)[None, :]) / (2 * sigma_space ** 2) \
                    + ((I - Gc[f][:, ic][:, :, jc]) ** 2).sum(0) / (2 * sigma_range ** 2) + shift
                E.append(torch.where(inside, e, torch.full_like(e, float("inf"))))
                taps.append((ic, jc))
        E = torch.stack(E)
        e_min[f] = E.amin(0)
        W = torch.exp(-(E - e_min[f]))
        num = torch.zeros((h0, w0, C), dtype=torch.float64)
        for k, (ic, jc) in enumerate(taps):
            num += W[k][..., None] * L[f][ic][:, jc]
        values[f] = num / W.sum(0)[..., None]
        ids[f] = values[f].argmax(-1).to(torch.uint8)
        if C == 1:
            margin[f] = float("inf")
            conf[f] = 255
        else:
            top = values[f].topk(2, dim=-1).values
            margin[f] = top[..., 0] - top[..., 1]
            conf[f] = torch.round(255 * margin[f].clamp(0, 1)).to(torch.uint8)
    return GuidedReadout(ids, conf, margin, values, e_min)


def _guided_call(soft: torch.Tensor, guide: torch.Tensor, cells: Optional[torch.Tensor], Hf: int, Wf: int, pad_shape, pad, out_shape,
                 norm_mask: bool, readout: ReadoutConfig, conf: bool = False, out=None):
    if guide is None:
        raise ValueError("the guided read-out needs the padded frames (guide=)")
    return ops.seg_readout_guided(soft, guide, Hf, Wf, pad_shape, pad, out_shape, norm_mask, readout.radius, readout.sigma_space,
                                  readout.sigma_range, conf=conf, out=out, cells=cells)


def _mask_readout(soft: torch.Tensor, Hf: int, Wf: int, seg_map: torch.Tensor, pad: Tuple[int, int, int, int],
                  out_shape: Tuple[int, int], norm_mask: bool, guide: Optional[torch.Tensor] = None,
                  readout: Optional[ReadoutConfig] = None) -> torch.Tensor:
    """(T, h0, w0) uint8: the argmax of the soft logits for frames 1.. (:772-802); frame 0 is the unpadded input map, nearest-resized to
    the output size (:708-711).  readout (a ReadoutConfig): frames 1.. go through the edge-aware read-out with guide (T, 3, hp, wp), the
    clip's padded frames; frame 0 is unchanged."""
    T = soft.shape[0]
    hp, wp = seg_map.shape
    lw, uw, lh, uh = pad
    masks = torch.empty((T, *out_shape), device=soft.device, dtype=torch.uint8)
    if T > 1 and readout is not None:
        _guided_call(soft[1:], None if guide is None else guide[1:], None, Hf, Wf, (hp, wp), pad, out_shape, norm_mask, readout,
                     out=masks[1:])
    elif T > 1:
        ops.seg_readout(soft[1:], Hf, Wf, (hp, wp), pad, out_shape, norm_mask, out=masks[1:])
    ref = seg_map[lh:hp - uh, lw:wp - uw].float()[None, None]
    masks[0] = torch.nn.functional.interpolate(ref, size=tuple(out_shape), mode="nearest")[0, 0].to(torch.uint8)
    return masks


def propagate_masks(feats_hwc: torch.Tensor, Hf: int, Wf: int, seg_map: torch.Tensor, pad: Tuple[int, int, int, int],
                    out_shape: Tuple[int, int], cfg, channels: Optional[int] = None, stats_out: Optional[list] = None,
                    events: Optional[dict] = None, affinity_stats: Optional[dict] = None, guide: Optional[torch.Tensor] = None,
                    readout: Optional[ReadoutConfig] = None, objects_out: Optional[list] = None, clean: Optional["CleanConfig"] = None,
                    clean_out: Optional[list] = None) -> torch.Tensor:
    """Semi-supervised VOS for one clip.  feats_hwc: the clip's bank as run_affinity (TrackerConfig) or run_local_affinity (LocalConfig)
    takes it, encoded from the PADDED frames; seg_map (hp, wp) uint8 the padded first-frame index map; pad = (left, right, top, bottom) as
    pad_divide_by gives it; out_shape = (h0, w0).  On the local window the feature grid is whatever the encoder made of the padded
    frame: (Hf, Wf) need not divide (hp, wp).
    Returns (T, h0, w0) uint8 on the device.  One host synchronisation: reading C = 1 + the largest id of the map at feature
    resolution (F.one_hot infers it the same way, so an id that vanishes there never appears in the output).
    readout (parse_readout's ReadoutConfig) with guide (T, 3, hp, wp) f32, the padded frames: the edge-aware read-out; None: the plain one.
    objects_out (a list): receives ops.object_stats of the returned masks with n_ids = C, the (T, C, 8) int64 device tensor (test_cfg.objects).
    clean (parse_clean's CleanConfig, test_cfg.clean): frames 1.. -- the read-out's -- are cleaned in place by ops.seg_clean with n_ids = C
    before the object statistics; frame 0, the given map, is left alone.  clean_out (a list) receives the (T, C, 4) int64 statistics."""
    T, dev = feats_hwc.shape[0], feats_hwc.device
    _record(events, "labels")
    C = int(ops.seg_max_label(seg_map, Hf, Wf).item()) + 1
    bank = torch.zeros((T, Hf * Wf, C), device=dev, dtype=torch.float32)
    ops.seg_onehot_labels(seg_map, Hf, Wf, C, out=bank[0])
    _record(events, "affinity")
    sw = label_affinity(feats_hwc, Hf, Wf, T, cfg, channels, stats_out, affinity_stats)
    _record(events, "propagation")
    soft = torch.empty_like(bank) if cfg.hard_prop else bank       # the read-out always sees the soft logits (:772-786)
    _sweep_labels(bank, soft, sw, Hf, Wf, cfg.hard_prop)
    _record(events, "readout")
    masks = _mask_readout(soft, Hf, Wf, seg_map, pad, out_shape, cfg.norm_mask, guide, readout)
    if clean is not None:
        _clean_masks(masks, C, clean, np.arange(T) >= 1, clean_out)
    if objects_out is not None:
        objects_out.append(ops.object_stats(masks, C))
    _record(events, "end")
    return masks


# ---- index maps annotated at any frame (test_cfg.refs, an extension key) -------------------------------------------
#
# The rule, stated once in sweep_refs_host (float64, on given top-k lists) and run on the device by propagate_masks_refs.  s0 = the earliest
# annotated frame.  The forward pass is the ordinary sweep of the sub-clip s0 .. T-1 (plan_clip(T, [s0], cfg) with its frames renumbered from
# 0: key slots [s0] + the preceding frames); an annotated frame t > s0 is injected after its propagation.  direction='both' labels frames
# s0-1 .. 0 by the same sweep of the time-reversed sub-clip s0, s0-1, .., 0 (a reversed copy of those frames' features, the ordinary forward
# plan of length s0 + 1).  The lists depend on the features only: a LabelSweep per (s0, 'fw' | 'bw') is what a LabelSession keeps.

REFS_DIRECTIONS = ("forward", "both")
REFS_OVERRIDES = ("new", "all")
REFS_FUSES = (None, "linear")


@dataclass
class RefsConfig:
    """test_cfg.refs = dict(direction='forward' | 'both', override='new' | 'all', confidence=False, fuse=None | 'linear'), parsed."""
    direction: str = "forward"
    override: str = "new"
    confidence: bool = False
    fuse: Optional[str] = None         # 'linear': forward and backward sweeps blended between annotated frames (section 25)


def parse_refs(spec) -> Optional[RefsConfig]:
    """None -> None (the option is off: ref_seg_map is one tensor for frame 0).  A mapping -> RefsConfig; an unknown key or value raises
    ValueError, a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError(f"test_cfg.refs: a dict such as dict(direction='forward', override='new'), got {type(spec).__name__}")
    spec = dict(spec)
    direction, override, confidence = spec.pop("direction", "forward"), spec.pop("override", "new"), spec.pop("confidence", False)
    fuse = spec.pop("fuse", None)
    if spec:
        raise ValueError(f"test_cfg.refs: unknown key(s) {sorted(spec)} (direction, override, confidence, fuse)")
    if direction not in REFS_DIRECTIONS:
        raise ValueError(f"test_cfg.refs: direction={direction!r} (one of {REFS_DIRECTIONS})")
    if override not in REFS_OVERRIDES:
        raise ValueError(f"test_cfg.refs: override={override!r} (one of {REFS_OVERRIDES})")
    if not isinstance(confidence, bool):
        raise ValueError(f"test_cfg.refs: confidence={confidence!r} (True or False)")
    if fuse not in REFS_FUSES:
        raise ValueError(f"test_cfg.refs: fuse={fuse!r} (one of {REFS_FUSES})")
    if fuse is not None and (direction != "both" or override != "all"):
        # a later map under 'new' is partial (YouTube-VOS's are): its background proves nothing, so no backward pass can start from it
        raise ValueError(f"test_cfg.refs: fuse={fuse!r} needs direction='both' and override='all', got direction={direction!r}, "
                         f"override={override!r}")
    return RefsConfig(direction, override, confidence, fuse)


def check_ref_maps(refs, n_frames: int, shape: Tuple[int, int]) -> Dict[int, torch.Tensor]:
    """The mapping form of ref_seg_map, checked: {frame index: integer map (h, w) or (1, h, w)} -> {int frame: (h, w) uint8 tensor} in
    ascending frame order (each on the device it came from).  A tensor means {0: tensor}.  TypeError for anything else; ValueError for an
    empty mapping, a frame index outside the clip, a map of another size than `shape`, a negative id; NotImplementedError for an id above 255
    (today's ref_seg_map rules)."""
    if torch.is_tensor(refs):
        refs = {0: refs}
    if not hasattr(refs, "keys"):
        raise TypeError(f"ref_seg_map: with test_cfg.refs a mapping {{frame index: index map}} or one tensor, got {type(refs).__name__}")
    if len(refs) == 0:
        raise ValueError("ref_seg_map: the mapping is empty (at least one annotated frame)")
    out = {}
    for key in sorted(refs.keys(), key=int):
        t, m = int(key), refs[key]
        if t != key or not 0 <= t < n_frames:
            raise ValueError(f"ref_seg_map: frame index {key!r} outside the clip's {n_frames} frames")
        if not torch.is_tensor(m):
            m = torch.as_tensor(m)
        if m.dim() == 3 and m.shape[0] == 1:
            m = m[0]
        if m.dim() != 2 or tuple(m.shape) != tuple(shape):
            raise ValueError(f"ref_seg_map[{t}]: a map of size {tuple(shape)} (the frames'), got {tuple(m.shape)}")
        if m.is_floating_point() or m.dtype == torch.bool:
            raise TypeError(f"ref_seg_map[{t}]: integer ids, got {m.dtype}")
        if m.dtype != torch.uint8:
            lo, hi = int(m.min()), int(m.max())
            if hi > 255:
                raise NotImplementedError(f"fgvc_amd: the mask path takes at most 255 object ids (largest id {hi} at frame {t}); split the "
                                          "objects over several calls")
            if lo < 0:
                raise ValueError(f"ref_seg_map[{t}]: negative id {lo}")
            m = m.to(torch.uint8)
        out[t] = m
    return out


def sweep_refs_host(small: Dict[int, torch.Tensor], n_frames: int, fw=None, bw=None, direction: str = "forward", override: str = "new",
                    hard_prop: bool = False) -> torch.Tensor:
    """The contract of test_cfg.refs in float64 torch, on given top-k lists.  small = {frame: (HW,) integer ids}, each annotated map
    already sampled to the feature grid; fw / bw: the lists of the forward sub-clip s0 .. T-1 and of the reversed sub-clip s0, s0-1, .., 0,
    each with `slot_frame` (n-1, t_max), `idx` (n-1, HW, k) = slot * HW + pixel and `weight` (n-1, HW, k) in the SUB-CLIP's own frame
    numbering (row j - 1 belongs to sub-clip frame j, a LabelSweep's layout; None where the sub-clip has one frame or is not swept).
    Returns the soft rows (T, HW, C) float64, C = 1 + the largest id of any map: what the read-out sees.  Frame s0 holds one_hot(M_s0);
    frames before s0 under 'forward' hold the background's one-hot."""
    if direction not in REFS_DIRECTIONS or override not in REFS_OVERRIDES:
        raise ValueError(f"sweep_refs_host: direction={direction!r}, override={override!r}")
    frames = sorted(small)
    s0, T = frames[0], int(n_frames)
    small = {t: small[t].reshape(-1).long() for t in frames}
    HW = small[s0].numel()
    C = 1 + max(int(m.max()) for m in small.values())

    def one_hot(m):
        return torch.nn.functional.one_hot(m, C).double()

    def sweep(lists, first, n, inject):
        bank = torch.zeros(n, HW, C, dtype=torch.float64)
        soft = torch.zeros_like(bank)
        bank[0] = soft[0] = first
        seen = set(small[s0].unique().tolist())
        for j in range(1, n):
            sf, idx, w = lists.slot_frame[j - 1].cpu().long(), lists.idx[j - 1].cpu().long(), lists.weight[j - 1].cpu().double()
            slot, pix = idx // HW, idx % HW
            soft[j] = (w[..., None] * bank[sf[slot], pix]).sum(1)
            hard = one_hot(soft[j].argmax(-1)) if hard_prop else None
            t = s0 + j
            if inject and t in small:
                ids = set(small[t].unique().tolist())
                chosen = ids if override == "all" else ids - seen
                seen |= ids
                sel = torch.isin(small[t], torch.tensor(sorted(chosen), dtype=torch.long))
                soft[j][sel] = one_hot(small[t])[sel]
                if hard_prop:
                    hard[sel] = one_hot(small[t])[sel]
            bank[j] = hard if hard_prop else soft[j]
        return soft

    out = torch.zeros(T, HW, C, dtype=torch.float64)
    out[:s0, :, 0] = 1.0
    out[s0:] = sweep(fw, one_hot(small[s0]), T - s0, True)
    if direction == "both" and s0 > 0:
        out[:s0] = sweep(bw, one_hot(small[s0]), s0 + 1, False)[1:].flip(0)
    return out


def next_frame_to_annotate(frame_score, annotated) -> Optional[int]:
    """The un-annotated frame with the lowest score, the lowest index among equals; None when every frame is annotated."""
    scores = [float(v) for v in (frame_score.tolist() if hasattr(frame_score, "tolist") else frame_score)]
    done = set(int(t) for t in annotated)
    best = None
    for f, s in enumerate(scores):
        if f not in done and (best is None or s < scores[best]):
            best = f
    return best


# ---- forward and backward sweeps fused between annotated frames (refs fuse='linear') --------------------------------
#
# With annotated frames s_0 < .. < s_m the forward pass starts at s_0 and the backward pass at s_m, both with every later (earlier) map
# injected whole (override='all').  Between two annotated frames the two passes' soft rows are blended linearly in time; the number of
# cells on which they name different objects is the frame's disagreement.

def fuse_refs_host(small: Dict[int, torch.Tensor], n_frames: int, fw=None, bw=None, hard_prop: bool = False):
    """The contract of test_cfg.refs fuse='linear' in float64 torch, on given top-k lists.  small as sweep_refs_host takes it; fw: the lists
    of the forward sub-clip s_0 .. T-1, bw: the lists of the reversed sub-clip s_m, s_m - 1, .., 0 (the LabelSweep refs_sweeps keeps under
    (s_m, 'bw')).  F = sweep_refs_host(forward, 'all') from s_0; B = the same rule on the reversed sub-clip with the maps mirrored, flipped
    back; under hard_prop each pass keeps its own hard bank and the soft rows are what is fused.
    Returns (rows (T, HW, C) float64, disagree (T,) int64):
      rows[t] = F[t] at an annotated frame (its one-hot map) and for t > s_m;  B[t] for t < s_0;
                w F[t] + (1 - w) B[t], w = (s_{i+1} - t) / (s_{i+1} - s_i), for s_i < t < s_{i+1};
      disagree[t] = the number of cells with argmax F[t] != argmax B[t] (the first maximum wins) for s_i < t < s_{i+1}, else 0.
    One annotated frame: sweep_refs_host(direction='both') itself and zeros."""
    frames = sorted(small)
    s0, sm, T = frames[0], frames[-1], int(n_frames)
    disagree = torch.zeros(T, dtype=torch.int64)
    if len(frames) == 1:
        return sweep_refs_host(small, T, fw=fw, bw=bw, direction="both", override="all", hard_prop=hard_prop), disagree
    F = sweep_refs_host(small, T, fw=fw, direction="forward", override="all", hard_prop=hard_prop)
    mirrored = {sm - t: small[t] for t in frames}
    B = sweep_refs_host(mirrored, sm + 1, fw=bw, direction="forward", override="all", hard_prop=hard_prop).flip(0)      # B[t], t = 0 .. s_m
    rows = F.clone()
    rows[:s0] = B[:s0]
    for a, b in zip(frames[:-1], frames[1:]):
        for t in range(a + 1, b):
            w = (b - t) / (b - a)
            rows[t] = w * F[t] + (1.0 - w) * B[t]
            disagree[t] = int((F[t].argmax(-1) != B[t].argmax(-1)).sum())
    return rows, disagree


def next_frame_to_annotate_by(disagree, annotated) -> Optional[int]:
    """The un-annotated frame with the largest disagreement count, the lowest index among equals; None when every frame is annotated."""
    counts = [int(v) for v in (disagree.tolist() if hasattr(disagree, "tolist") else disagree)]
    done = set(int(t) for t in annotated)
    best = None
    for f, n in enumerate(counts):
        if f not in done and (best is None or n > counts[best]):
            best = f
    return best


def refs_sweeps(feats_hwc: torch.Tensor, Hf: int, Wf: int, s0: int, both: bool, cfg: TrackerConfig, channels: Optional[int] = None,
                stats_out: Optional[list] = None, sweeps: Optional[dict] = None, counters: Optional[dict] = None,
                bw_from: Optional[int] = None):
    """(fw, bw): the LabelSweeps of the forward sub-clip s0 .. T-1 and (both, s0 > 0) of the reversed sub-clip s0 .. 0; None where the
    sub-clip has one frame.  `sweeps`: a cache keyed (s0, 'fw' | 'bw') that is read and filled; `counters['affinity_runs']` goes up by one
    when this call had to compute a part.  bw_from (the fused branch: the last annotated frame s_m): the reversed sub-clip starts there
    instead, cached under (s_m, 'bw'); no (s_m, 'fw') is computed."""
    if isinstance(cfg, LocalConfig):
        raise NotImplementedError("test_cfg.refs: the local-window affinity (plan_local_clip has no start frame)")
    T = feats_hwc.shape[0]
    sweeps = {} if sweeps is None else sweeps
    sb = s0 if bw_from is None else int(bw_from)
    ran = False
    if (s0, "fw") not in sweeps:
        sweeps[(s0, "fw")] = label_affinity(feats_hwc[s0:], Hf, Wf, T - s0, cfg, channels, stats_out) if T - s0 > 1 else None
        ran = ran or T - s0 > 1
    if both and sb > 0 and (sb, "bw") not in sweeps:
        rev = feats_hwc[:sb + 1].flip(0).contiguous()
        sweeps[(sb, "bw")] = label_affinity(rev, Hf, Wf, sb + 1, cfg, channels, stats_out)
        ran = True
    if ran and counters is not None:
        counters["affinity_runs"] = counters.get("affinity_runs", 0) + 1
    return sweeps[(s0, "fw")], (sweeps[(sb, "bw")] if both and sb > 0 else None)


def _sweep_refs(bank: torch.Tensor, soft: torch.Tensor, sw: Optional[LabelSweep], Hf: int, Wf: int, hard_prop: bool, inject: dict) -> None:
    """_sweep_labels with injections: inject = {sub-clip frame j: (padded map, id set (8,) int32 on the device)}, applied to soft[j] (and
    bank[j] under hard_prop) after frame j's propagation."""
    C = bank.shape[2]
    for f in range(1, bank.shape[0]):
        ops.propagate_topk(bank, sw.slot_frame[f - 1], sw.idx[f - 1], sw.weight[f - 1], Hf, Wf, Hf, Wf, window_L=sw.window_L, out=soft[f])
        if hard_prop:
            ops.seg_hard_onehot(soft[f], out=bank[f])
        if f in inject:
            seg, ids = inject[f]
            ops.seg_inject_labels(seg, Hf, Wf, C, ids, soft[f])
            if hard_prop:
                ops.seg_inject_labels(seg, Hf, Wf, C, ids, bank[f])


def propagate_masks_refs(feats_hwc: torch.Tensor, Hf: int, Wf: int, seg_maps: Dict[int, torch.Tensor], pad: Tuple[int, int, int, int],
                         out_shape: Tuple[int, int], cfg, rc: RefsConfig, channels: Optional[int] = None, stats_out: Optional[list] = None,
                         confidence: bool = False, sweeps: Optional[dict] = None, counters: Optional[dict] = None,
                         guide: Optional[torch.Tensor] = None, readout: Optional[ReadoutConfig] = None, cells: Optional[torch.Tensor] = None,
                         disagree_out: Optional[list] = None, objects_out: Optional[list] = None, clean: Optional["CleanConfig"] = None,
                         clean_out: Optional[list] = None):
    """propagate_masks with index maps at any frames: seg_maps = {frame: padded (hp, wp) uint8 map on the device}; rc names the direction and
    the override rule (sweep_refs_host is the contract).  Returns (T, h0, w0) uint8 on the device; frame s0 (the earliest annotated one) is
    its given map, unpadded and nearest-resized, every other frame the read-out of its rows, frames before s0 under 'forward' zero.
    confidence: (masks, conf (T, h0, w0) uint8, stats (T, C, 2) int64) as ops.seg_readout_conf gives them; frame s0 has conf 255, frames
    that are not labelled at all conf 0.  One host read: the presence sets of all maps (C = 1 + the largest id present in any).
    sweeps / counters: refs_sweeps' cache and counter; counters['sweeps'] counts these calls.
    readout / guide as propagate_masks takes them; cells: ops.guide_cells of the whole guide where the caller keeps it (a LabelSession).
    rc.fuse='linear' with more than one annotated frame (fuse_refs_host is the contract): the forward sweep from the first and the backward
    sweep from the last annotated frame, blended between the maps by ops.seg_fuse_rows, then the same read-outs; disagree_out (a list)
    receives the (T,) int64 device tensor of per-frame disagreement counts.  With one annotated frame the call is direction='both'.
    objects_out (a list): receives ops.object_stats of the returned masks with n_ids = C, the (T, C, 8) int64 device tensor.
    clean / clean_out as propagate_masks takes them: every frame a read-out launch wrote is cleaned -- frames s0 + 1 .. T - 1, later annotated
    frames among them (their maps were injected into the rows, the read-out made the pixels), and frames 0 .. s0 - 1 where the backward
    pass labels them; frame s0, the given map, and frames that stay zero under 'forward' are left alone.  conf and stats stay the raw
    read-out's."""
    if readout is not None and guide is None:
        raise ValueError("the guided read-out needs the padded frames (guide=)")
    if isinstance(cfg, LocalConfig):
        raise NotImplementedError("test_cfg.refs: the local-window affinity (plan_local_clip has no start frame)")
    T, dev = feats_hwc.shape[0], feats_hwc.device
    frames = sorted(seg_maps)
    s0 = frames[0]
    sets_dev = torch.empty((len(frames), 8), device=dev, dtype=torch.int32)
    for i, t in enumerate(frames):
        ops.seg_label_set(seg_maps[t], Hf, Wf, out=sets_dev[i])
    present = [set(ops.label_set_ids(row)) for row in sets_dev.cpu()]                     # the call's one host read
    C = 1 + max(max(p) for p in present)
    inject, seen = {}, set(present[0])
    for t, ids in zip(frames[1:], present[1:]):
        chosen = ids if rc.override == "all" else ids - seen
        seen |= ids
        if chosen:
            inject[t - s0] = (seg_maps[t], ops.label_set_words(sorted(chosen)).to(dev))
    both = rc.direction == "both"
    sm = frames[-1]
    fused = rc.fuse is not None and sm > s0                             # one annotated frame: nothing to fuse, the call is direction='both'
    fw, bw = refs_sweeps(feats_hwc, Hf, Wf, s0, both, cfg, channels, stats_out, sweeps, counters, bw_from=sm if fused else None)
    if counters is not None:
        counters["sweeps"] = counters.get("sweeps", 0) + 1
    hp, wp = seg_maps[s0].shape
    lw, uw, lh, uh = pad
    masks = torch.zeros((T, *out_shape), device=dev, dtype=torch.uint8)
    conf = torch.zeros_like(masks) if confidence else None
    stats = torch.zeros((T, C, 2), device=dev, dtype=torch.int64) if confidence else None

    def sweep(n, first, sw, inj):
        """the soft rows (n, HW, C) of one sub-clip of n frames that starts from one_hot(M_first)"""
        bank = torch.zeros((n, Hf * Wf, C), device=dev, dtype=torch.float32)
        ops.seg_onehot_labels(seg_maps[first], Hf, Wf, C, out=bank[0])
        soft = torch.empty_like(bank) if cfg.hard_prop else bank
        _sweep_refs(bank, soft, sw, Hf, Wf, cfg.hard_prop, inj)
        return soft

    def read(rows, dst):
        """the read-out of the row blocks `rows` goes to the clip frames `dst` (a slice or an index)"""
        if readout is not None:
            out = _guided_call(rows, guide[dst], None if cells is None else cells[dst], Hf, Wf, (hp, wp), pad, out_shape, cfg.norm_mask,
                               readout, conf=confidence)
            if confidence:
                masks[dst], conf[dst], stats[dst] = out
            else:
                masks[dst] = out
        elif confidence:
            m, c, st = ops.seg_readout_conf(rows, Hf, Wf, (hp, wp), pad, out_shape, cfg.norm_mask)
            masks[dst], conf[dst], stats[dst] = m, c, st
        elif isinstance(dst, slice):
            ops.seg_readout(rows, Hf, Wf, (hp, wp), pad, out_shape, cfg.norm_mask, out=masks[dst])
        else:
            masks[dst] = ops.seg_readout(rows, Hf, Wf, (hp, wp), pad, out_shape, cfg.norm_mask)

    def run(n, sw, inj, dst):
        """one sub-clip of n frames from one_hot(M_s0); the read-out of its frames 1.. goes to the clip frames `dst`"""
        soft = sweep(n, s0, sw, inj)
        if n >= 2:
            read(soft[1:], dst)

    if fused:
        # forward from s_0 and backward from s_m, every other map injected whole; the frames between two maps are blended in ONE launch,
        # written over the forward pass's rows, so that the read-outs below see the clip's rows where the unfused call has them
        soft_f = sweep(T - s0, s0, fw, inject)
        soft_b = sweep(sm + 1, sm, bw, {sm - t: (seg_maps[t], ops.label_set_words(sorted(ids)).to(dev))
                                        for t, ids in zip(frames[:-1], present[:-1])})
        between = [(t, (b - t) / (b - a)) for a, b in zip(frames[:-1], frames[1:]) for t in range(a + 1, b)]
        disagree = torch.zeros((T,), device=dev, dtype=torch.int64)
        if between:
            _, counts = ops.seg_fuse_rows(soft_f, soft_b, [t - s0 for t, _ in between], [sm - t for t, _ in between], [w for _, w in between])
            disagree[torch.tensor([t for t, _ in between], device=dev)] = counts
        if disagree_out is not None:
            disagree_out.append(disagree)
        read(soft_f[1:], slice(s0 + 1, T))
        if s0 > 0:
            read(soft_b[sm - s0 + 1:], torch.arange(s0 - 1, -1, -1, device=dev))      # sub-clip frame j of the backward pass is clip frame s_m - j
    else:
        run(T - s0, fw, inject, slice(s0 + 1, T))
        if both and s0 > 0:
            run(s0 + 1, bw, {}, torch.arange(s0 - 1, -1, -1, device=dev))
    ref = seg_maps[s0][lh:hp - uh, lw:wp - uw].float()[None, None]
    masks[s0] = torch.nn.functional.interpolate(ref, size=tuple(out_shape), mode="nearest")[0, 0].to(torch.uint8)
    if clean is not None:
        produced = np.arange(T) > s0
        if s0 > 0 and (fused or both):
            produced |= np.arange(T) < s0
        _clean_masks(masks, C, clean, produced, clean_out)
    if objects_out is not None:
        objects_out.append(ops.object_stats(masks, C))
    if not confidence:
        return masks
    conf[s0] = 255
    given = [s0] if both else list(range(s0 + 1))                     # frames whose statistics no read-out wrote: counts by id, conf as above
    for f in given:
        cnt = torch.bincount(masks[f].flatten().long(), minlength=C)[:C]
        stats[f, :, 0] = cnt
        stats[f, :, 1] = cnt * (255 if f == s0 else 0)
    return masks, conf, stats


def frame_scores(stats: torch.Tensor, out_shape: Tuple[int, int]) -> torch.Tensor:
    """stats (T, C, 2) int64 -> (T,) float64 on the host: the mean conf byte of every frame / 255, from the integer sums."""
    return stats[..., 1].sum(1).cpu().double() / (255.0 * int(out_shape[0]) * int(out_shape[1]))


def propagate_soft_bank(feats_hwc: torch.Tensor, Hf: int, Wf: int, heat: torch.Tensor, map_pad: Tuple[int, int, int, int], cfg,
                        channels: Optional[int] = None, stats_out: Optional[list] = None, events: Optional[dict] = None,
                        affinity_stats: Optional[dict] = None) -> Tuple[torch.Tensor, LabelSweep]:
    """The part propagate_heatmaps and propagate_softmaps share: first-frame labels, affinity and the sweep.  heat (K, hm, wm) f32 | f64 on
    the device, the map BEFORE its own padding map_pad = (left, right, top, bottom) (pad_divide_by of the map's size, :672).  Returns the
    label bank (T, HfWf, K) f32 both read-outs start from, and the LabelSweep it was swept with.  K is the map's first dimension: no
    host read; no min-max normalisation (:785 applies to index maps only).  Records the events 'labels', 'affinity', 'propagation'.
    hard_prop is refused on either route: the reference's F.one_hot without num_classes fails on soft labels (:762-768)."""
    if cfg.hard_prop:
        raise NotImplementedError("propagate_soft_bank: hard_prop with soft labels")
    T, dev = feats_hwc.shape[0], feats_hwc.device
    _record(events, "labels")
    bank = torch.zeros((T, Hf * Wf, heat.shape[0]), device=dev, dtype=torch.float32)
    ops.seg_soft_labels(heat, map_pad, Hf, Wf, out=bank[0])
    _record(events, "affinity")
    sw = label_affinity(feats_hwc, Hf, Wf, T, cfg, channels, stats_out, affinity_stats)
    _record(events, "propagation")
    _sweep_labels(bank, bank, sw, Hf, Wf)
    return bank, sw


@dataclass
class PoseConfig:
    """test_cfg.pose = dict(confidence=True, keep_field=False), parsed."""
    confidence: bool = True
    keep_field: bool = False


def parse_pose(spec) -> Optional[PoseConfig]:
    """None -> None (the option is off: the coords=True call leaves last_pose None).  A mapping -> PoseConfig; an unknown key or value
    raises ValueError, a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError(f"test_cfg.pose: a dict such as dict(confidence=True, keep_field=False), got {type(spec).__name__}")
    spec = dict(spec)
    confidence, keep_field = spec.pop("confidence", True), spec.pop("keep_field", False)
    if spec:
        raise ValueError(f"test_cfg.pose: unknown key(s) {sorted(spec)} (confidence, keep_field)")
    if not isinstance(confidence, bool):
        raise ValueError(f"test_cfg.pose: confidence={confidence!r} (True or False)")
    if not isinstance(keep_field, bool):
        raise ValueError(f"test_cfg.pose: keep_field={keep_field!r} (True or False)")
    return PoseConfig(confidence, keep_field)


@dataclass
class PoseField:
    """What the coordinate read-out of one clip scanned, kept on the device (test_cfg.pose.keep_field=True): the label bank (T, HfWf, K) f32,
    the first-frame map (K, hm, wm) and the geometry.  maps() makes the full-resolution maps of a frame range from them, without a second
    model call: T K h0 w0 values never have to exist at once."""
    bank: torch.Tensor
    heat: torch.Tensor
    Hf: int
    Wf: int
    map_pad: Tuple[int, int, int, int]
    out_shape: Tuple[int, int]

    @property
    def num_frames(self) -> int:
        return int(self.bank.shape[0])

    @property
    def num_joints(self) -> int:
        return int(self.heat.shape[0])

    def maps(self, f_begin: int = 0, f_end: Optional[int] = None, out_dtype: Optional[torch.dtype] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Frames [f_begin, f_end) of the maps, (f_end - f_begin, K, h0, w0) on the device: ops.softmap_readout, what the return_maps=True
        call gives for those frames, bit for bit."""
        f_end = self.num_frames if f_end is None else int(f_end)
        return ops.softmap_readout(self.bank, self.heat, self.Hf, self.Wf, self.map_pad, self.out_shape, frames=(int(f_begin), f_end),
                                   out_dtype=out_dtype, out=out)


def propagate_heatmaps(feats_hwc: torch.Tensor, Hf: int, Wf: int, heat: torch.Tensor, map_pad: Tuple[int, int, int, int],
                       out_shape: Tuple[int, int], cfg, channels: Optional[int] = None, stats_out: Optional[list] = None,
                       events: Optional[dict] = None, affinity_stats: Optional[dict] = None, peak: bool = False,
                       field_out: Optional[list] = None):
    """Soft first-frame labels read out as joint coordinates for one clip (test_cfg.coords=True): propagate_soft_bank's arguments and
    out_shape = (h0, w0).  Returns (2, K, T) float64 on the device = img2coord of the stacked maps (:814-818); frame 0 is the padded map,
    not unpadded (:712-716).  peak=True: (coords, peak (K, T) float64), every map's largest value (ops.heatmap_coords).  field_out: a list
    that receives the clip's PoseField."""
    bank, _ = propagate_soft_bank(feats_hwc, Hf, Wf, heat, map_pad, cfg, channels, stats_out, events, affinity_stats)
    _record(events, "readout")
    coords = ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape, peak=peak)
    _record(events, "end")
    if field_out is not None:
        field_out.append(PoseField(bank, heat, Hf, Wf, tuple(map_pad), tuple(out_shape)))
    return coords


def propagate_softmaps(feats_hwc: torch.Tensor, Hf: int, Wf: int, heat: torch.Tensor, map_pad: Tuple[int, int, int, int],
                       out_shape: Tuple[int, int], cfg, channels: Optional[int] = None, stats_out: Optional[list] = None,
                       events: Optional[dict] = None, frames: Optional[Tuple[int, int]] = None,
                       affinity_stats: Optional[dict] = None) -> torch.Tensor:
    """propagate_heatmaps with the maps themselves as the result (the reference's return value without `coords`, :770-784, :800-803):
    (T, K, h0, w0) on the device, or the rows `frames` = (f_begin, f_end) of it, float64 iff `heat` is float64 (np.stack of a float64
    frame 0 with float32 later frames).  Same bank, same field as the coordinate read-out: ops.softmap_readout writes what
    ops.heatmap_coords scans.  The whole stack is T K h0 w0 values: for a host-bound result see softmaps_to_host."""
    bank, _ = propagate_soft_bank(feats_hwc, Hf, Wf, heat, map_pad, cfg, channels, stats_out, events, affinity_stats)
    _record(events, "readout")
    maps = ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape, frames=frames)
    _record(events, "end")
    return maps

# ---- predicted visibility: the forward-backward cycle check -------------------------------------------------------
#
# HRVanillaTracker.forward_test_forward (vanilla_tracker.py:591-645) with precede_frames = 1 pushes points through the chain of
# frame-to-frame coordinate fields.  Run on the reversed sub-clip [f, f-1, ..., s] from the PREDICTED position x_f it walks the prediction
# back to the query frame; how far it lands from the query point is the forward-backward tracking error.  The field of query frame g and
# key frame g - 1 does not depend on s, f or the point: the T - 1 fields are computed once per clip and every (group, frame, point) chases
# through them.

@dataclass
class OcclusionConfig:
    """test_cfg.occlusion = dict(type='cycle', cycle_thresh=1.0, radius=None), parsed.  `cycle_thresh` is in FEATURE CELLS (the fields live
    on the feature grid: an error below its pitch cannot be told from their own quantisation); `radius` = the local window of the fields."""
    cycle_thresh: float = 1.0
    radius: int = 12


def parse_occlusion(spec, default_radius: int) -> Optional[OcclusionConfig]:
    """None -> None (the option is off: the trackers return zeros, as the reference does).  A mapping with type='cycle' -> OcclusionConfig;
    any other `type` (or none), an unknown key or a value out of range raises ValueError, a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError(f"test_cfg.occlusion: a dict such as dict(type='cycle', cycle_thresh=1.0, radius=None), got {type(spec).__name__}")
    spec = dict(spec)
    typ = spec.pop("type", None)
    if typ != "cycle":
        raise ValueError(f"test_cfg.occlusion: type={typ!r} (only 'cycle', the forward-backward cycle check)")
    thresh, radius = spec.pop("cycle_thresh", 1.0), spec.pop("radius", None)
    if spec:
        raise ValueError(f"test_cfg.occlusion: unknown key(s) {sorted(spec)} (type, cycle_thresh, radius)")
    thresh = float(thresh)
    if not (math.isfinite(thresh) and thresh >= 0):
        raise ValueError(f"test_cfg.occlusion: cycle_thresh={thresh} (a finite number of feature cells >= 0)")
    radius = int(default_radius) if radius is None else int(radius)
    if radius < 0:
        raise ValueError(f"test_cfg.occlusion: radius={radius}")
    return OcclusionConfig(thresh, radius)


@dataclass
class InputConfig:
    """test_cfg.input, parsed (an extension key, DESIGN.md sections 14 and 19): the trackers then take uint8 frames wherever they take float
    ones.  dict(type='rgb8', size=(h, w) | None, layout='thwc' | 'tchw'): RGB bytes, converted with ops.frames_to_lab.
    dict(type='nv12' | 'i420', size=, matrix='bt601' | 'bt709', range='limited' | 'full', siting='left' | 'center'): packed 8-bit YUV 4:2:0
    frames (T, 3 h0 / 2, w0), converted with ops.yuv_frames_to_lab.  dict(type=<an ops.YUV_PIXEL_FORMATS name>, size=, matrix=, range=,
    siting=): packed frames of that format in its dtype (uint16 for 10 to 16 bits), (T, 3 h0 / 2 | 2 h0 | 3 h0, w0), converted with
    ops.yuv_planes_to_lab; `matrix` has no default there and `siting` is refused with a 4:4:4 type.  `size`: the network size the frames are resized to (None: their own);
    `layout`: where an RGB frame tensor keeps its channels."""
    size: Optional[Tuple[int, int]] = None
    layout: str = "thwc"
    type: str = "rgb8"
    matrix: str = "bt601"
    range: str = "limited"
    siting: str = "left"

    @property
    def yuv(self) -> bool:
        return self.type != "rgb8"


INPUT_TYPES = ("rgb8",) + ops.YUV_FORMATS + tuple(ops.YUV_PIXEL_FORMATS)


def input_dtype(typ: str) -> torch.dtype:
    """The dtype of the raw frames a test_cfg.input type names: uint8, or uint16 for the 10- to 16-bit formats."""
    return ops.YUV_PIXEL_FORMATS[typ][5] if typ in ops.YUV_PIXEL_FORMATS else torch.uint8


def parse_input(spec) -> Optional[InputConfig]:
    """None -> None (the option is off: float frames only).  A mapping with type='rgb8' | 'nv12' | 'i420' | an ops.YUV_PIXEL_FORMATS
    name -> InputConfig; any other `type` (or none), a key its type does not have (`layout` with a YUV type; `matrix`, `range`, `siting` with
    'rgb8'; `siting` with a 4:4:4 type), an ops.YUV_PIXEL_FORMATS type without its `matrix`, an unknown value, or a size
    that is not two positive integers raises ValueError, a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError(f"test_cfg.input: a dict such as dict(type='rgb8', size=(256, 256), layout='thwc'), got {type(spec).__name__}")
    spec = dict(spec)
    typ = spec.pop("type", None)
    if typ not in INPUT_TYPES:
        raise ValueError(f"test_cfg.input: type={typ!r} (one of {INPUT_TYPES}: uint8 RGB frames, packed 8-bit YUV 4:2:0 frames, packed "
                         "4:2:0 / 4:2:2 / 4:4:4 frames at 8 to 16 bits)")
    size = spec.pop("size", None)
    if typ == "rgb8":
        layout = spec.pop("layout", "thwc")
        if spec:
            raise ValueError(f"test_cfg.input: unknown key(s) {sorted(spec)} (type, size, layout)")
        if layout not in ops.INPUT_LAYOUTS:
            raise ValueError(f"test_cfg.input: layout={layout!r} (one of {ops.INPUT_LAYOUTS})")
        ic = InputConfig(None, layout)
    else:
        if "siting" in spec and typ in ops.YUV_PIXEL_FORMATS and ops.YUV_PIXEL_FORMATS[typ][1] == 1:
            raise ValueError(f"test_cfg.input: siting= has no meaning for type={typ!r} (4:4:4: every pixel has its own chroma sample); remove it")
        # 'nv12' / 'i420' default to bt601 as they always did; the newer types have no default matrix -- 10-bit, 4:2:2 and 4:4:4 material is
        # HD, UHD or camera footage, for which a silent bt601 is wrong more often than right -- so the type alone (dict(type='p010')) stays
        # the ValueError it was before these types existed
        matrix = spec.pop("matrix", None if typ in ops.YUV_PIXEL_FORMATS else "bt601")
        rng, siting = spec.pop("range", "limited"), spec.pop("siting", "left")
        if "layout" in spec:
            raise ValueError(f"test_cfg.input: layout= belongs to type='rgb8'; {typ!r} frames are packed {ops._packed_shape(typ)}")
        if spec:
            raise ValueError(f"test_cfg.input: unknown key(s) {sorted(spec)} (type, size, matrix, range, siting)")
        if matrix is None:
            raise ValueError(f"test_cfg.input: type={typ!r} needs matrix= (one of {tuple(ops.YUV_MATRICES)}): the stream's own, there is no "
                             "default for this type")
        if matrix not in ops.YUV_MATRICES:
            raise ValueError(f"test_cfg.input: matrix={matrix!r} (one of {tuple(ops.YUV_MATRICES)})")
        if rng not in ops.YUV_RANGES:
            raise ValueError(f"test_cfg.input: range={rng!r} (one of {tuple(ops.YUV_RANGES)})")
        if siting not in ops.YUV_SITINGS:
            raise ValueError(f"test_cfg.input: siting={siting!r} (one of {ops.YUV_SITINGS})")
        ic = InputConfig(None, "thwc", typ, matrix, rng, siting)
    if size is not None:
        size = tuple(int(v) for v in size)
        if len(size) != 2 or min(size) < 1:
            raise ValueError(f"test_cfg.input: size={size} (two positive integers (h, w), or None for the frames' own size)")
    ic.size = size
    return ic


MASK_FORMS = ("numpy", "device")


def parse_masks(value) -> str:
    """test_cfg.masks (an extension key): how the index-map call returns its masks.  None | 'numpy' -> 'numpy' (the (T, h0, w0) float64
    host array, as the reference returns), 'device' -> 'device' (the uint8 CUDA tensor propagate_masks made, for metrics' backend='hip');
    anything else raises ValueError."""
    if value is None:
        return "numpy"
    if value not in MASK_FORMS:
        raise ValueError(f"test_cfg.masks={value!r}: one of {MASK_FORMS}")
    return value


OBJECTS_KEYS = ("stats",)


def parse_objects(spec) -> bool:
    """test_cfg.objects (an extension key): None -> False; dict(stats=True | False) -> whether the index-map call
    leaves an ObjectTracks of the masks it returns in model.last_objects.  An unknown sub-key, a non-mapping or a non-bool value raises
    ValueError naming it."""
    if spec is None:
        return False
    if not hasattr(spec, "keys"):
        raise ValueError(f"test_cfg.objects={spec!r}: a dict with the keys {OBJECTS_KEYS}")
    unknown = sorted(set(spec.keys()) - set(OBJECTS_KEYS))
    if unknown:
        raise ValueError(f"test_cfg.objects: unknown key(s) {unknown}; the keys are {OBJECTS_KEYS}")
    stats = spec.get("stats", True)
    if not isinstance(stats, bool):
        raise ValueError(f"test_cfg.objects.stats={stats!r}: True or False")
    return stats


CLEAN_KEYS = ("min_area", "keep", "connectivity", "fill_holes", "max_hole_area")
CLEAN_KEEPS = ("all", "largest")


@dataclass(frozen=True)
class CleanConfig:
    """test_cfg.clean, parsed: the arguments of ops.seg_clean / metrics.clean_masks_host."""
    min_area: int = 0
    keep: str = "all"
    connectivity: int = 8
    fill_holes: bool = False
    max_hole_area: Optional[int] = None

    @property
    def active(self) -> bool:
        """whether the rule can change a pixel at all (a component has at least one pixel)"""
        return self.min_area > 1 or self.keep == "largest" or self.fill_holes

    def kwargs(self) -> dict:
        return dict(min_area=self.min_area, keep=self.keep, connectivity=self.connectivity, fill_holes=self.fill_holes,
                    max_hole_area=self.max_hole_area)


def parse_clean(spec) -> Optional[CleanConfig]:
    """test_cfg.clean (an extension key): None -> None; dict(min_area=0, keep='all' | 'largest', connectivity=8 | 4,
    fill_holes=False, max_hole_area=None) -> a CleanConfig: the index-map call cleans the frames its read-out made (ops.seg_clean) before
    the object statistics, the scoring and the host copy.  An unknown sub-key, a non-mapping or a bad value raises ValueError naming it.
    A spec that changes nothing (min_area <= 1, keep='all', no fill) is accepted; the call then launches nothing for it."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise ValueError(f"test_cfg.clean={spec!r}: a dict with the keys {CLEAN_KEYS}")
    unknown = sorted(set(spec.keys()) - set(CLEAN_KEYS))
    if unknown:
        raise ValueError(f"test_cfg.clean: unknown key(s) {unknown}; the keys are {CLEAN_KEYS}")

    def integer(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
    min_area = spec.get("min_area", 0)
    if not integer(min_area) or not 0 <= min_area < 1 << 31:
        raise ValueError(f"test_cfg.clean.min_area={min_area!r}: an integer 0 .. 2^31 - 1")
    keep = spec.get("keep", "all")
    if keep not in CLEAN_KEEPS:
        raise ValueError(f"test_cfg.clean.keep={keep!r}: one of {CLEAN_KEEPS}")
    connectivity = spec.get("connectivity", 8)
    if not integer(connectivity) or connectivity not in (4, 8):
        raise ValueError(f"test_cfg.clean.connectivity={connectivity!r}: 4 or 8")
    fill_holes = spec.get("fill_holes", False)
    if not isinstance(fill_holes, bool):
        raise ValueError(f"test_cfg.clean.fill_holes={fill_holes!r}: True or False")
    max_hole_area = spec.get("max_hole_area", None)
    if max_hole_area is not None and (not integer(max_hole_area) or max_hole_area < 0):
        raise ValueError(f"test_cfg.clean.max_hole_area={max_hole_area!r}: None or an integer >= 0")
    return CleanConfig(int(min_area), keep, int(connectivity), fill_holes, None if max_hole_area is None else int(max_hole_area))


def _clean_masks(masks: torch.Tensor, C: int, clean: CleanConfig, produced: np.ndarray, clean_out: Optional[list]) -> None:
    """ops.seg_clean in place on the frames of masks (T, h, w) uint8 whose `produced` entry is true, n_ids = C; the (T, C, 4) int64 statistics
    go to clean_out.  A spec that changes nothing, or no produced frame: nothing is launched and clean_out receives None."""
    stats = None
    if clean.active and produced.any() and masks.numel():
        flags = None if produced.all() else torch.from_numpy(produced).to(masks.device)
        _, stats = ops.seg_clean(masks, C, frames=flags, out=masks, **clean.kwargs())
    if clean_out is not None:
        clean_out.append(stats)


@dataclass
class ObjectTracks:
    """The objects of a (T, h, w) id map as boxes: a view over stats (T, N, 8) int64 as ops.object_stats / metrics.object_stats_host give
    them (a tensor on any device or an array; kept as given in `stats`, every property is a numpy array on the host).  Row o is id o, the
    background (row 0) included.  The host copy is made once, at the first property read: `stats` is not to be written afterwards."""
    stats: object
    _host_copy: Optional[np.ndarray] = field(default=None, init=False, repr=False, compare=False)

    def _host(self) -> np.ndarray:
        if self._host_copy is None:
            s = self.stats
            a = s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else np.asarray(s)
            if a.ndim != 3 or a.shape[2] != 8 or a.dtype != np.int64:
                raise ValueError(f"stats: (T, N, 8) int64, got {a.dtype} {a.shape}")
            a = a.view()
            a.setflags(write=False)
            self._host_copy = a
        return self._host_copy

    @property
    def area(self) -> np.ndarray:
        """(T, N) int64 pixel counts"""
        return self._host()[..., 0]

    @property
    def present(self) -> np.ndarray:
        """(T, N) bool: the id has a pixel on the frame"""
        return self._host()[..., 0] > 0

    @property
    def boxes(self) -> np.ndarray:
        """(T, N, 4) int64 (x0, y0, x1, y1), half-open; an absent object's is (0, 0, 0, 0), which is empty"""
        return self._host()[..., 1:5]

    @property
    def centroids(self) -> np.ndarray:
        """(T, N, 2) float64 (mean x, mean y) of the pixels' integer coordinates = sum / area; NaN where absent"""
        a = self._host()
        area = a[..., 0:1].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(area > 0, a[..., 5:7].astype(np.float64) / area, np.nan)

    @property
    def border(self) -> np.ndarray:
        """(T, N) int64: the object's pixels on the frame's outermost rows and columns"""
        return self._host()[..., 7]

    def centroid_tracks(self):
        """(tracks (N, T, 2) float64, visibles (N, T) bool) as viz.paint_point_track / viz.paint_trails / viz.render take them.  The
        painters draw a track coordinate c at c + 0.5 in pixel indices (viz._paint_host: x = track + 0.5, and a dot at track 5.0 is shared
        equally by pixels 5 and 6; the trails' segments run through track + 0.5 with pixel p at the point p): in the painters' convention
        the centre of pixel p is the coordinate p - 0.5.  `centroids` are means of pixel indices, so the tracks are centroids - 0.5: an
        object of the one pixel p gets its dot centred on pixel p.  Absent objects: coordinate 0 and visible False."""
        c = np.nan_to_num(self.centroids - 0.5, nan=0.0)
        return np.ascontiguousarray(c.transpose(1, 0, 2)), np.ascontiguousarray(self.present.T)

    def _on_device(self) -> bool:
        return isinstance(self.stats, torch.Tensor) and self.stats.is_cuda

    def windows(self, size, pad: float = 0.125, min_side: int = 8, smooth: int = 0, mask_size=None, frame_size=None, objects=None):
        """The crop windows (T, M, 8) int64 that follow the objects (default: ids 1 .. N - 1), by the window rule of
        metrics.object_windows_host: words 0 .. 3 in the pixels of mask_size = (h, w), the id map the statistics
        came from, words 4 .. 7 in those of frame_size = (H, W) (None: mask_size).  With `stats` on the GPU: one launch of
        ops.object_windows, the result stays there and nothing is read back; with host stats: the host contract, a numpy array."""
        if self._on_device():
            return ops.object_windows(self.stats, size, pad, min_side, smooth, mask_size, frame_size, objects)
        from . import metrics
        s = self.stats.detach().numpy() if isinstance(self.stats, torch.Tensor) else np.asarray(self.stats)
        return metrics.object_windows_host(s, size, pad, min_side, smooth, mask_size, frame_size, objects)

    def crops(self, frames_u8, size=(128, 128), pad: float = 0.125, min_side: int = 8, smooth: int = 0, mask_size=None, objects=None,
              masks: bool = False, ids=None, layout: str = "thwc", fill=None) -> "ObjectCrops":
        """An ObjectCrops of the uint8 RGB frames ((T, H, W, 3) 'thwc' or (T, 3, H, W) 'tchw'): every object's window (`windows`, with
        frame_size the frames' own, which may be larger than the mask: a clip tracked at 480p, cropped from its 1080p source) resampled
        onto `size` by the rule of viz.crop_windows_host.  masks=True with ids (T, h, w) uint8, the id map: also every object's mask in
        its window.  mask_size: None takes ids' size, without ids the frames'.  With `stats` on the GPU the frames (and ids) are GPU
        tensors and the chain is ops.object_windows + ops.object_crops: three launches, nothing read back, the results stay on the
        device.  With host stats: numpy arrays through the two host contracts."""
        if layout not in ops.INPUT_LAYOUTS:
            raise ValueError(f"layout={layout!r}: one of {ops.INPUT_LAYOUTS}")
        if masks and ids is None:
            raise ValueError("masks=True needs ids=, the (T, h, w) id map")
        shape = tuple(frames_u8.shape)
        if len(shape) != 4:
            raise ValueError(f"frames_u8: 4 dimensions, got {shape}")
        frame_size = shape[1:3] if layout == "thwc" else shape[2:4]
        if mask_size is None:
            mask_size = tuple(ids.shape[1:3]) if ids is not None else frame_size
        n_ids = self.stats.shape[1]
        objs = list(range(1, n_ids)) if objects is None else [int(o) for o in objects]
        win = self.windows(size, pad, min_side, smooth, mask_size, frame_size, objs)
        size = (int(size[0]), int(size[1]))
        if self._on_device():
            got = ops.object_crops(frames_u8, win, size, layout, fill, ids if masks else None, objs if masks else None)
        else:
            from . import viz
            f = frames_u8.detach().cpu().numpy() if isinstance(frames_u8, torch.Tensor) else np.asarray(frames_u8)
            m = None if not masks else (ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids))
            f = f if layout == "thwc" else f.transpose(0, 2, 3, 1)
            got = viz.crop_windows_host(f, win, size, None if fill is None else np.asarray(fill, np.uint8), m, objs if masks else None)
        c, mk = got if masks else (got, None)
        return ObjectCrops(c, mk, win, objs, size)


@dataclass
class ObjectCrops:
    """What ObjectTracks.crops returns: crops (T, M, S_h, S_w, 3) uint8, masks (T, M, S_h, S_w) uint8 or None, windows (T, M, 8) int64
    (tensors on the device or arrays, as the chain made them), objects (the M ids) and size = (S_h, S_w).  to_crop / from_crop are the
    affine map between frame pixels and crop pixels of window (t, j), on the host: frame x in [fx0, fx1) <-> crop x in [0, S_w)."""
    crops: object
    masks: object
    windows: object
    objects: List[int]
    size: Tuple[int, int]
    _host_windows: Optional[np.ndarray] = field(default=None, init=False, repr=False, compare=False)

    def _host(self) -> np.ndarray:
        if self._host_windows is None:
            w = self.windows
            self._host_windows = w.detach().cpu().numpy() if isinstance(w, torch.Tensor) else np.asarray(w)
        return self._host_windows

    def _win(self, t: int, j: int):
        x0, y0, x1, y1 = (float(v) for v in self._host()[t, j, -4:])
        if x1 <= x0 or y1 <= y0:
            raise ValueError(f"window ({t}, {j}) is empty: the object is absent on that frame")
        return x0, y0, x1, y1

    @property
    def valid(self) -> np.ndarray:
        """(T, M) bool: the window is not empty (the object is present on the frame)"""
        w = self._host()
        return (w[..., -2] > w[..., -4]) & (w[..., -1] > w[..., -3])

    def to_crop(self, xy, t: int, j: int, pixel_centers: bool = False) -> np.ndarray:
        """Frame coordinates (..., 2) as (x, y) -> coordinates in crop (t, j), float64.  The coordinates are continuous, a pixel p covering
        [p, p + 1); with pixel_centers=True they are pixel indices (the centre of pixel p is p) on both sides."""
        x0, y0, x1, y1 = self._win(t, j)
        p = np.asarray(xy, np.float64)
        if p.shape[-1] != 2:
            raise ValueError(f"xy: (..., 2) as (x, y), got {p.shape}")
        half = 0.5 if pixel_centers else 0.0
        s = np.array([self.size[1] / (x1 - x0), self.size[0] / (y1 - y0)])
        return (p + half - np.array([x0, y0])) * s - half

    def from_crop(self, xy, t: int, j: int, pixel_centers: bool = False) -> np.ndarray:
        """The inverse of to_crop: coordinates in crop (t, j) -> frame coordinates."""
        x0, y0, x1, y1 = self._win(t, j)
        p = np.asarray(xy, np.float64)
        if p.shape[-1] != 2:
            raise ValueError(f"xy: (..., 2) as (x, y), got {p.shape}")
        half = 0.5 if pixel_centers else 0.0
        s = np.array([(x1 - x0) / self.size[1], (y1 - y0) / self.size[0]])
        return (p + half) * s + np.array([x0, y0]) - half


def backward_fields(feats_hwc: torch.Tensor, Hf: int, Wf: int, cfg: LocalConfig, scale: int, stats: Optional[dict] = None) -> torch.Tensor:
    """The clip's T - 1 backward coordinate fields (T-1, HW, 2) f32, (x, y) image pixels interleaved: fields[g - 1] = get_coord(query =
    frame g, key = frame g - 1) (vanilla_tracker.py:445-488), the expected position in frame g - 1 of every feature cell of frame g.
    feats_hwc: f32 rows (T, HW, C) (L2-normalised iff cfg.with_norm) or their split_f16x2 form, as run_local_affinity takes them.
    `cfg`: a LocalConfig with precede_frames = 1 and with_first = False -- plan_local_clip then yields exactly the pairs (g, g - 1), run in
    chunked launches within cfg.pair_budget -- then ONE fgvc_topk_coord_rows_f32 launch.  `stats`: run_local_affinity's."""
    if cfg.precede_frames != 1 or cfg.with_first:
        raise ValueError("backward_fields: a LocalConfig with precede_frames=1 and with_first=False (one key slot per frame: the one before)")
    T = feats_hwc.shape[0]
    if T < 2:
        return torch.empty((0, Hf * Wf, 2), device=feats_hwc.device, dtype=torch.float32)
    plan = plan_local_clip(T, cfg, Hf * Wf)
    assert plan.pairs == [(g, g - 1) for g in range(1, T)]
    idx, _, weight = run_local_affinity(feats_hwc, Hf, Wf, plan, cfg, stats)
    return ops.topk_coord_rows(idx, weight, Hf, Wf, int(cfg.radius), int(scale))


def cycle_check(fields: torch.Tensor, traj: torch.Tensor, start: int, query_xy: torch.Tensor, scale: int, thresh: float,
                Hf: int, Wf: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One query-time group.  fields (T-1, HW, 2) = backward_fields of the clip; traj (T-start, P, 2) = the group's predicted (x, y) from
    its query frame `start` on (row 0 = the query frame itself); query_xy (P, 2) = x_s; thresh in feature cells.
    Returns visible (T-start, P) bool = err <= thresh * scale, err (T-start, P) f32 and back (T-start, P, 2) f32 = the back-tracked points.
    Row 0 (the query frame) is visible with err 0 and back = the query point."""
    n, P = traj.shape[0] - 1, traj.shape[1]
    assert n >= 0 and fields.shape[0] >= start + n
    dev = traj.device
    q = query_xy.to(dev, torch.float32)
    err = torch.zeros((n + 1, P), device=dev, dtype=torch.float32)
    back = torch.empty((n + 1, P, 2), device=dev, dtype=torch.float32)
    back[0] = q
    if n and P:
        b, e = ops.cycle_chase(fields[start:start + n], traj[1:], q, scale, Hf, Wf)
        back[1:], err[1:] = b, e
    return err <= float(thresh) * float(scale), err, back


def cycle_check_groups(fields: torch.Tensor, traj: torch.Tensor, times: torch.Tensor, query_xy: torch.Tensor, scale: int, thresh: float,
                       Hf: int, Wf: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """cycle_check for every query-time group of a regrouped clip: the fields are shared, the chase runs per group with its own start.
    traj (T, P, 2) and times (P,) int64 (host) / query_xy (P, 2) in the SAME point order (track_points' `order`: ascending query time).
    Returns visible (T, P) bool and err (T, P) f32; frames before a point's query time are not scored: visible 0, err +inf."""
    T, P = traj.shape[0], traj.shape[1]
    dev = traj.device
    vis = torch.zeros((T, P), device=dev, dtype=torch.bool)
    err = torch.full((T, P), float("inf"), device=dev, dtype=torch.float32)
    times = times.to("cpu", torch.int64)
    for s in sorted(set(times.tolist())):
        cols = (times == s).nonzero().flatten()
        q = query_xy[cols.to(query_xy.device)]
        cols = cols.to(dev)
        v, e, _ = cycle_check(fields, traj[s:, cols], s, q, scale, thresh, Hf, Wf)
        vis[s:, cols], err[s:, cols] = v, e
    return vis, err


# ---- dense optical flow between frames (test_cfg.flow, an extension key) ------------------------------------------------
#
# The window lists of a frame pair ARE a correspondence: the cycle check above reads them as coordinate fields on the feature grid.  Here
# both time directions of every pair `step` frames apart are planned as single-slot rows of ONE affinity run, read out to full resolution by
# one kernel, and checked against each other by one more.

FLOW_OCCLUSIONS = ("consistency", "fb_abs")


@dataclass
class FlowConfig:
    """test_cfg.flow = dict(type='window', radius=None, step=1, renorm=True, occlusion=None | 'consistency' | 'fb_abs', diff=1.5), parsed.
    `radius`: the local window of the lists, in feature cells; `step`: the frame distance of a pair; `renorm`: ops.flow_from_lists';
    `occlusion`: the forward-backward check to run on the two flows (ops.flow_consistency), `diff` its 'fb_abs' threshold in pixels."""
    radius: int = 12
    step: int = 1
    renorm: bool = True
    occlusion: Optional[str] = None
    diff: float = 1.5


def parse_flow(spec, default_radius: int) -> Optional[FlowConfig]:
    """None -> None (the option is off).  A mapping with type='window' -> FlowConfig; any other `type` (or none), an unknown key or a value
    out of range raises ValueError ('range_map', the reference's third occlusion mode, NotImplementedError: ops.flow_consistency says
    why), a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError("test_cfg.flow: a dict such as dict(type='window', radius=None, step=1, renorm=True, occlusion=None, diff=1.5), "
                        f"got {type(spec).__name__}")
    spec = dict(spec)
    typ = spec.pop("type", None)
    if typ != "window":
        raise ValueError(f"test_cfg.flow: type={typ!r} (only 'window': the read-out of the local window's top-k lists)")
    radius, step, renorm = spec.pop("radius", None), spec.pop("step", 1), spec.pop("renorm", True)
    occlusion, diff = spec.pop("occlusion", None), spec.pop("diff", 1.5)
    if spec:
        raise ValueError(f"test_cfg.flow: unknown key(s) {sorted(spec)} (type, radius, step, renorm, occlusion, diff)")
    radius = int(default_radius) if radius is None else int(radius)
    if radius < 0:
        raise ValueError(f"test_cfg.flow: radius={radius}")
    if isinstance(step, bool) or int(step) != step or int(step) < 1:
        raise ValueError(f"test_cfg.flow: step={step!r} (the frame distance of a pair: an integer >= 1)")
    if not isinstance(renorm, (bool, int)) or renorm not in (0, 1):
        raise ValueError(f"test_cfg.flow: renorm={renorm!r} (True or False)")
    if occlusion == "range_map":
        ops._flow_mode(occlusion)
    if occlusion is not None and occlusion not in FLOW_OCCLUSIONS:
        raise ValueError(f"test_cfg.flow: occlusion={occlusion!r} (None or one of {FLOW_OCCLUSIONS})")
    diff = float(diff)
    if not (math.isfinite(diff) and diff >= 0):
        raise ValueError(f"test_cfg.flow: diff={diff} (a finite number of pixels >= 0)")
    return FlowConfig(radius, int(step), bool(renorm), occlusion, diff)


def flow_plan(n_frames: int, step: int, HW: int, cfg: LocalConfig) -> LocalPlan:
    """The schedule of a clip's flow pairs, one key slot per row (t_max = 1): rows 0 .. T-step-1 are the forward pairs (query g, key
    g + step), the T - step rows after them the backward pairs (query g + step, key g).  Rows are chunked so that a chunk's pair lists
    (HW * topk * 8 bytes per pair) stay within cfg.pair_budget, as plan_local_clip chunks."""
    step = int(step)
    if step < 1:
        raise ValueError(f"flow_plan: step={step}")
    n = max(0, int(n_frames) - step)
    pairs = [(g, g + step) for g in range(n)] + [(g + step, g) for g in range(n)]
    pair_bytes = HW * int(cfg.topk) * 8
    if pairs and pair_bytes > cfg.pair_budget:
        raise ValueError(f"pair_budget={cfg.pair_budget} bytes holds less than one pair's lists ({pair_bytes} bytes)")
    per = max(1, int(cfg.pair_budget) // pair_bytes) if pairs else 1
    chunks = [(r0, min(r0 + per, len(pairs)), r0, min(r0 + per, len(pairs))) for r0 in range(0, len(pairs), per)]
    return LocalPlan(int(n_frames), pairs, [[p] for p in range(len(pairs))], [[kf] for _, kf in pairs], 1, chunks, pair_bytes)


def flow_fields(feats_hwc: torch.Tensor, Hf: int, Wf: int, cfg: LocalConfig, scale: int, size: Tuple[int, int],
                pad: Tuple[int, int] = (0, 0), step: int = 1, renorm: bool = True, stats: Optional[dict] = None):
    """Dense flow of every frame pair `step` apart, both directions: flow_fw[g] takes frame g to frame g + step, flow_bw[g] frame g + step
    to frame g.  feats_hwc as run_local_affinity takes them; `cfg`: a LocalConfig (its radius is the window; precede_frames / with_first are
    not read: the plan is flow_plan's); `scale` = padded frame / feature grid, `size` = the network size (h, w), `pad` = (left, top).
    Returns flow_fw, flow_bw (T-step, 2, h, w) f32 and valid_fw, valid_bw (T-step, h, w) uint8 -- one affinity run (chunked within
    cfg.pair_budget) and ONE fgvc_flow_from_lists_f32 launch for both directions.  `stats`: run_local_affinity's."""
    T, dev = feats_hwc.shape[0], feats_hwc.device
    n = max(0, T - int(step))
    h, w = (int(v) for v in size)
    if n == 0:
        z, v = torch.empty((0, 2, h, w), device=dev), torch.empty((0, h, w), device=dev, dtype=torch.uint8)
        return z, z.clone(), v, v.clone()
    plan = flow_plan(T, step, Hf * Wf, cfg)
    idx, _, weight = run_local_affinity(feats_hwc, Hf, Wf, plan, cfg, stats)
    flow, valid = ops.flow_from_lists(idx, weight, Hf, Wf, int(cfg.radius), int(scale), (h, w), pad, renorm)
    return flow[:n], flow[n:], valid[:n], valid[n:]


def flow_occlusion(flow_fw: torch.Tensor, flow_bw: torch.Tensor, mode: str = "consistency", diff: float = 1.5):
    """occ_fw, occ_bw (n, 1, h, w) f32, 1 = consistent: the reference's occlusion_estimation on the two flows (ops.flow_consistency)."""
    return ops.flow_consistency(flow_fw, flow_bw, mode, diff)


# ---- point tracks in both time directions by chaining the dense flow (test_cfg.chain, an extension key) ----------------
#
# The reference's TAP-Vid flow-chaining baseline (RAFT.forward_test, raft.py:247-289): positions are pushed forward through flow_fw, pinned to
# the query point at the query time, and pulled backward through flow_bw for every frame before it.  chain_points_host is the rule written
# down in float32 scalars, chain_points the product path (one fgvc_flow_chain_f32 launch).

CHAIN_VISIBILITIES = ("frame", "consistency")
CHAIN_LIMIT = 2.0 ** 23


@dataclass
class ChainConfig:
    """test_cfg.chain = dict(type='flow', visibility='frame' | 'consistency'), parsed.  'frame': the reference's rule, a point is visible
    while it is inside the frame; 'consistency': it also stays invisible past the first hop that starts outside the frame or on a pixel the
    flow's forward-backward check rejects."""
    visibility: str = "frame"


def parse_chain(spec) -> Optional[ChainConfig]:
    """None -> None (the option is off).  A mapping with type='flow' -> ChainConfig; any other `type` (or none), an unknown key or an unknown
    visibility raises ValueError, a non-mapping TypeError."""
    if spec is None:
        return None
    if not hasattr(spec, "keys"):
        raise TypeError(f"test_cfg.chain: a dict such as dict(type='flow', visibility='frame'), got {type(spec).__name__}")
    spec = dict(spec)
    typ = spec.pop("type", None)
    if typ != "flow":
        raise ValueError(f"test_cfg.chain: type={typ!r} (only 'flow': chaining the dense flow of test_cfg.flow)")
    visibility = spec.pop("visibility", "frame")
    if spec:
        raise ValueError(f"test_cfg.chain: unknown key(s) {sorted(spec)} (type, visibility)")
    if visibility not in CHAIN_VISIBILITIES:
        raise ValueError(f"test_cfg.chain: visibility={visibility!r} (one of {CHAIN_VISIBILITIES})")
    return ChainConfig(visibility)


def check_query_times(times, n_frames: int) -> None:
    """ValueError unless every query time (a host sequence or tensor) is an integer of [0, n_frames)."""
    t = torch.as_tensor(times).detach().to("cpu", torch.float64).flatten()
    bad = ~(torch.isfinite(t) & (t == t.floor()) & (t >= 0) & (t < n_frames))
    if bool(bad.any()):
        raise ValueError(f"query_points: query time {float(t[bad][0])} (integers in [0, {n_frames}) are tracked)")


def grid_queries(t: int, h: int, w: int, stride: int, offset=None) -> torch.Tensor:
    """(P, 3) f32 queries (t, x, y) on a regular grid of frame t: x = ox, ox + stride, ... < w and y alike, row-major (y outer).  `offset`
    = (ox, oy), default (stride // 2, stride // 2).  Dense tracks are the points call with these queries."""
    t, h, w, stride = int(t), int(h), int(w), int(stride)
    if stride < 1 or h < 1 or w < 1 or t < 0:
        raise ValueError(f"grid_queries: t={t}, {h} x {w}, stride={stride}")
    ox, oy = (stride // 2, stride // 2) if offset is None else (int(offset[0]), int(offset[1]))
    if not (0 <= ox < w and 0 <= oy < h):
        raise ValueError(f"grid_queries: offset=({ox}, {oy}) outside the {h} x {w} frame")
    ys, xs = torch.meshgrid(torch.arange(oy, h, stride, dtype=torch.float32), torch.arange(ox, w, stride, dtype=torch.float32), indexing="ij")
    return torch.stack([torch.full_like(xs, float(t)), xs, ys], -1).reshape(-1, 3)


def chain_points_host(flow_fw, flow_bw, query, ok_fw=None, ok_bw=None, visibility: str = "frame"):
    """The rule fgvc_flow_chain_f32 is held to, on numpy arrays in float32 scalars.  flow_fw / flow_bw (T-1, 2, h, w), query (P, 3) =
    (t, x, y), ok_fw / ok_bw (T-1, h, w) for visibility='consistency'.  Returns traj (T, P, 2) float32 and vis (T, P) uint8.

    Per point: traj[tq] = (x, y) as given; for t = tq+1 .. T-1: c = c + S(flow_fw[t-1], c); from the query point again, for t = tq-1 .. 0:
    c = c + S(flow_bw[t], c).  S is the reference's bilinear_sample2d (samp.py:5-99): taps at the clamped floor and floor + 1, weights from
    the unclamped ones, ((w00 i00 + w01 i01) + w10 i10) + w11 i11.  A position that is non-finite or at 2^23 or beyond is never turned into
    an index: that frame and every later one on that side are NaN and invisible (the query frame keeps the query); a query time that is no
    integer of [0, T) makes every frame of the point NaN."""
    import numpy as np
    f32 = np.float32
    if visibility not in CHAIN_VISIBILITIES:
        raise ValueError(f"visibility={visibility!r}: one of {CHAIN_VISIBILITIES}")
    flow_fw, flow_bw = np.asarray(flow_fw, f32), np.asarray(flow_bw, f32)
    query = np.asarray(query, f32)
    n, _, h, w = flow_fw.shape
    assert flow_fw.shape == flow_bw.shape == (n, 2, h, w) and query.ndim == 2 and query.shape[1] == 3
    sticky = visibility == "consistency"
    if sticky:
        if ok_fw is None or ok_bw is None:
            raise ValueError("visibility='consistency' needs ok_fw and ok_bw, (T-1, h, w)")
        ok_fw, ok_bw = np.asarray(ok_fw), np.asarray(ok_bw)
        assert ok_fw.shape == ok_bw.shape == (n, h, w)
    T, P = n + 1, query.shape[0]
    traj = np.full((T, P, 2), np.nan, f32)
    vis = np.zeros((T, P), np.uint8)
    one, half, wf, hf = f32(1), f32(0.5), f32(w), f32(h)

    def bad(x, y):
        return not (abs(x) < CHAIN_LIMIT and abs(y) < CHAIN_LIMIT)

    def inside(x, y):
        return bool(x >= 0 and y >= 0 and x < wf and y < hf)

    def clamp(v, hi):
        return min(max(int(v), 0), hi)

    def hop(field, ok, x, y):
        x0f, y0f = np.floor(x), np.floor(y)
        x1f, y1f = x0f + one, y0f + one
        xa, xb, ya, yb = clamp(x0f, w - 1), clamp(int(x0f) + 1, w - 1), clamp(y0f, h - 1), clamp(int(y0f) + 1, h - 1)
        w00, w01, w10, w11 = (x1f - x) * (y1f - y), (x - x0f) * (y1f - y), (x1f - x) * (y - y0f), (x - x0f) * (y - y0f)
        d = [((w00 * pl[ya, xa] + w01 * pl[ya, xb]) + w10 * pl[yb, xa]) + w11 * pl[yb, xb] for pl in (field[0], field[1])]
        good = True
        if sticky:
            good = inside(x, y) and ok[clamp(np.floor(y + half), h - 1), clamp(np.floor(x + half), w - 1)] != 0
        return x + d[0], y + d[1], good

    with np.errstate(all="ignore"):
        for p in range(P):
            qt, qx, qy = query[p]
            if not (qt >= 0 and qt < T and np.floor(qt) == qt):
                continue
            tq = int(qt)
            traj[tq, p] = (qx, qy)
            vis[tq, p] = inside(qx, qy)
            for frames, fields, oks, at in ((range(tq + 1, T), flow_fw, ok_fw, -1), (range(tq - 1, -1, -1), flow_bw, ok_bw, 0)):
                x, y, all_good = qx, qy, True
                for t in frames:
                    if bad(x, y):
                        break
                    x, y, good = hop(fields[t + at], oks[t + at] if sticky else None, x, y)
                    all_good = all_good and good
                    if bad(x, y):
                        break
                    traj[t, p] = (x, y)
                    vis[t, p] = inside(x, y) and (all_good or not sticky)
    return traj, vis


def chain_points(flow_fw: torch.Tensor, flow_bw: torch.Tensor, query: torch.Tensor, ok_fw: Optional[torch.Tensor] = None,
                 ok_bw: Optional[torch.Tensor] = None, visibility: str = "frame") -> Tuple[torch.Tensor, torch.Tensor]:
    """chain_points_host on the device: traj (T, P, 2) f32 and vis (T, P) uint8 from one fgvc_flow_chain_f32 launch (ops.flow_chain).
    query (P, 3) = (t, x, y), any float dtype, on any device."""
    q = query.to(flow_fw.device, torch.float32)
    return ops.flow_chain(flow_fw, flow_bw, q, ok_fw, ok_bw, visibility)


def chain_masks(flow: Dict[str, torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
    """ok_fw, ok_bw (T-1, h, w) uint8 of a forward_test_flow result with its forward-backward check: valid & (occ == 1)."""
    return tuple(((flow["valid_" + d] != 0) & (flow["occ_" + d][:, 0] == 1)).to(torch.uint8) for d in ("fw", "bw"))
