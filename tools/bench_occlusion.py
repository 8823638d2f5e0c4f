#!/usr/bin/env python3
"""Time the visibility read-out (test_cfg.occlusion = dict(type='cycle')) and print one JSON line.  The geometries of
bench.py's cfg2 (8 frames of 480 x 854, strides (1, 2, 1, 1), 16 points) and cfg4 (64 frames of 256 x 256, strides (1, 1, 1, 4), 32 points),
VanillaTracker with the bench's test_cfg, query points at frame 0 and (second line of each geometry) spread over the first half of the clip.
Per geometry, medians of HIP-event times: the whole model call without the option and with it (their difference is what the option
adds), and inside the option's share the T - 1 backward fields (pair top-k under the square window + merge + fgvc_topk_coord_rows_f32) and
the chase (fgvc_cycle_chase_f32 + the comparison) each on its own.

    python tools/bench_occlusion.py [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import engine  # noqa: E402

TEST_CFG = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, step=512, with_first=True, with_first_neighbor=True, batch_step=8)


def build(strides, dev, **extra):
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=strides, out_indices=(2,),
                                                                       pool_type="none", zero_init_residual=False)),
                            train_cfg=None, test_cfg=api.ConfigDict(**TEST_CFG, **extra))
    torch.manual_seed(0)
    model.init_weights()
    return model.to(dev).eval()


def timed(fn, iters, warmup):
    """Median ms of fn() between HIP events."""
    ms = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


def run(dev, T, size, strides, P, iters, warmup, spread):
    h, w = size
    g = torch.Generator().manual_seed(1)
    rgbs = torch.randn(1, T, 3, h, w, generator=g).clamp(-1, 1).to(dev)
    t0 = torch.randint(0, max(1, T // 2), (P,), generator=g).float() if spread else torch.zeros(P)
    qp = torch.stack([t0, torch.rand(P, generator=g) * (w - 40) + 20, torch.rand(P, generator=g) * (h - 40) + 20], -1)[None].to(dev)
    traj, vis = torch.zeros(1, T, P, 2, device=dev), torch.ones(1, T, P, device=dev)
    plain, model = build(strides, dev), build(strides, dev, occlusion=dict(type="cycle"))
    call = lambda m: m(test_mode=True, rgbs=rgbs, query_points=qp, trajectories=traj, visibilities=vis)
    with torch.no_grad():
        off_ms = timed(lambda: call(plain), iters, warmup)
        on_ms = timed(lambda: call(model), iters, warmup)
        outs = call(model)
        occ = model._occlusion()
        feats, Hf, Wf = model.get_feats_hwc(rgbs[0], split=True)
        fields_ms = timed(lambda: model._cycle_fields(feats, Hf, Wf, w, occ), iters, warmup)
        fields, scale = model._cycle_fields(feats, Hf, Wf, w, occ)
        qo = outs[4][0]
        chase_ms = timed(lambda: engine.cycle_check_groups(fields, outs[2][0], qo[:, 0], qo[:, 1:], scale, occ.cycle_thresh, Hf, Wf), iters, warmup)
    return {"frames": T, "size": [h, w], "strides": list(strides), "points": P, "query_times": sorted(set(int(t) for t in t0)),
            "feature_grid": [Hf, Wf], "window_radius": occ.radius, "fields": T - 1, "fields_route": model.cycle_stats.get("route"),
            "fields_chunks": model.cycle_stats.get("chunks"), "call_ms_without": round(off_ms, 3), "call_ms_with": round(on_ms, 3),
            "added_ms": round(on_ms - off_ms, 3), "fields_ms": round(fields_ms, 3), "chase_ms": round(chase_ms, 3),
            "predicted_visible_share": round(float(outs[3].mean()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for name, T, size, strides, P in (("bench_480p_8f", 8, (480, 854), (1, 2, 1, 1), 16), ("davis_64f_256", 64, (256, 256), (1, 1, 1, 4), 32)):
        out[name] = run(dev, T, size, strides, P, a.iters, a.warmup, spread=False)
        out[name + "_spread_queries"] = run(dev, T, size, strides, P, a.iters, a.warmup, spread=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
