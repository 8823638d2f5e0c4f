#!/usr/bin/env python3
"""Time HRVanillaTracker's label-map path (forward_test_backward_save_mem on the local window) and print one JSON line:

  vos     8 x 480 x 854, 3 objects, neighbor_range = 30 (R = 15: 961 taps x up to 6 key slots), index maps -> masks;
  jhmdb   40 x 320 x 320, K = 15 joint heat maps (coords=True) -> (2, K, T) coordinates.

Per workload: ms per clip with the encoder / labels / affinity (pair top-k + merge) / propagation / read-out split by HIP events, and the
planned affinity (one pair launch + one merge launch per chunk) next to the per-frame loop the HR points path runs (one
fgvc_local_corr_topk_f16x3 call per frame: a gather of its key frames out of the same split bank, the pair kernel on <= 6 pairs, the merge).

    python tools/bench_hr_seg.py [--iters 10 --warmup 2]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import engine, ops  # noqa: E402
from fgvc_amd.datasets import pose_heatmaps  # noqa: E402

PHASES = ("labels", "affinity", "propagation", "readout", "end")
med = lambda v: sorted(v)[len(v) // 2]


def _model(dev, coords):
    torch.manual_seed(0)
    cfg = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, with_first=True, coords=coords)
    m = api.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                     pool_type="none")), test_cfg=api.ConfigDict(cfg))
    m.init_weights()
    return m.to(dev).eval()


def _run(model, frames, run_labels, iters, warmup):
    split = {k: [] for k in ("encoder", "labels", "affinity", "propagation", "readout", "total")}
    stats = {}
    with torch.no_grad():
        for it in range(warmup + iters):
            ev = {k: torch.cuda.Event(enable_timing=True) for k in ("start",) + PHASES}
            ev["start"].record()
            feats, Hf, Wf = model._label_feats(frames)
            out = run_labels(feats, Hf, Wf, ev, stats)
            torch.cuda.synchronize()
            if it >= warmup:
                seq = ("start",) + PHASES
                for k0, k1, name in zip(seq[:-1], seq[1:], ("encoder", "labels", "affinity", "propagation", "readout")):
                    split[name].append(ev[k0].elapsed_time(ev[k1]))
                split["total"].append(ev["start"].elapsed_time(ev["end"]))
    return feats, Hf, Wf, out, split, stats


def _affinity_ab(feats, Hf, Wf, cfg, iters):
    """The planned affinity against the per-frame loop on ONE split bank: ms each, and whether their lists agree bit for bit."""
    bank = ops.split_f16x2(feats)
    T = bank.shape[0]
    plan = engine.plan_local_clip(T, cfg, Hf * Wf)

    def planned():
        return engine.run_local_affinity(bank, Hf, Wf, plan, cfg)

    def per_frame():
        return [ops.local_corr_topk(bank[f:f + 1], bank[engine.key_slots(f, 0, cfg.precede_frames, cfg.with_first)], Hf, Wf, cfg.radius,
                                    cfg.topk, cfg.temperature, normalized=True, presplit=True) for f in range(1, T)]

    def timeit(fn):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters

    with torch.no_grad():
        a, b = planned(), per_frame()
        same = all(torch.equal(a[0][f - 1], b[f - 1][0]) and torch.equal(a[2][f - 1], b[f - 1][2]) for f in range(1, T))
        return {"planned_ms": round(timeit(planned), 3), "per_frame_loop_ms": round(timeit(per_frame), 3), "pairs": len(plan.pairs),
                "launches_planned": 2 * len(plan.chunks), "launches_per_frame": 2 * (T - 1), "bit_identical": same}


def bench_vos(dev, iters, warmup):
    T, h, w, objects = 8, 480, 854, 3
    model = _model(dev, coords=False)
    cfg = model._label_config()
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    seg = torch.zeros(h, w, dtype=torch.uint8)
    for k in range(objects):
        y0, x0 = 60 + 100 * k, 100 + 220 * k
        seg[y0:y0 + 120, x0:x0 + 160] = k + 1
    (hp, wp), pad = engine.pad_divide_by(h, w, model.stride)
    seg = F.pad(seg.to(dev), pad).contiguous()
    frames = F.pad(imgs[0, 0], pad).transpose(0, 1).contiguous()
    run = lambda feats, Hf, Wf, ev, st: engine.propagate_masks(feats, Hf, Wf, seg, pad, (h, w), cfg, events=ev, affinity_stats=st)
    feats, Hf, Wf, masks, split, stats = _run(model, frames, run, iters, warmup)
    return {"config": {"frames": T, "size": [h, w], "objects": objects, "feature_grid": [Hf, Wf], "R": cfg.radius, "taps": cfg.window ** 2,
                       "key_slots": cfg.precede_frames + 1, "topk": cfg.topk},
            "route": stats["route"], "chunks": stats["chunks"], "pair_list_mb": round(stats["workspace_bytes"] / 1e6, 1),
            "ms_per_clip": round(med(split["total"]), 3), "split_ms": {k: round(med(v), 3) for k, v in split.items() if k != "total"},
            "affinity_ab": _affinity_ab(feats, Hf, Wf, cfg, iters), "masks_frame_last_ids": sorted(torch.unique(masks[-1]).tolist())}


def bench_jhmdb(dev, iters, warmup):
    T, h, w, K = 40, 320, 320, 15
    model = _model(dev, coords=True)
    cfg = model._label_config()
    g = torch.Generator().manual_seed(2)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(40, 280, K), rng.uniform(40, 280, K)], 1)
    heat = torch.from_numpy(pose_heatmaps(pts, (h, w), 4, (h, w))).to(dev).contiguous()
    _, pad = engine.pad_divide_by(h, w, model.stride)
    _, map_pad = engine.pad_divide_by(h, w, model.stride)
    frames = F.pad(imgs[0, 0], pad).transpose(0, 1).contiguous()
    run = lambda feats, Hf, Wf, ev, st: engine.propagate_heatmaps(feats, Hf, Wf, heat, map_pad, (h, w), cfg, events=ev, affinity_stats=st)
    feats, Hf, Wf, coords, split, stats = _run(model, frames, run, iters, warmup)
    return {"config": {"frames": T, "size": [h, w], "joints": K, "feature_grid": [Hf, Wf], "R": cfg.radius, "topk": cfg.topk},
            "route": stats["route"], "chunks": stats["chunks"], "pair_list_mb": round(stats["workspace_bytes"] / 1e6, 1),
            "ms_per_clip": round(med(split["total"]), 3), "split_ms": {k: round(med(v), 3) for k, v in split.items() if k != "total"},
            "affinity_ab": _affinity_ab(feats, Hf, Wf, cfg, iters), "coords_finite": bool(torch.isfinite(coords).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"vos": bench_vos(dev, a.iters, a.warmup), "jhmdb": bench_jhmdb(dev, a.iters, a.warmup)}
    if ops.pair_f16x3_timed_out():
        raise SystemExit("fgvc_pair_topk_f16x3: a bounded wait timed out during the run")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
