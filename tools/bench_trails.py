#!/usr/bin/env python3
"""Time the trail renderer (fgvc_render_trails_u8, fgvc_amd.viz), print one JSON line and write it to
profiles/trails_bench.json.

Inputs are synthetic and seeded: 8 frames of 480 x 854 uint8, trail = 8, line width 2, radius 7 (the reference's for this size).
(i)   "p256": 256 points on random walks (tools/bench_render.py's) -- one ops.render_trails call with everything on the device and `out`
      given: trails + dots, the trails alone (dots=False), and the dots-only ops.render_frames of the same clip, medians of HIP-event times;
      viz.render(trail=8, backend='host') on the same inputs, wall clock, the WHOLE clip.
(ii)  "grid4": the 25 560 points of engine.grid_queries(0, 480, 854, 4), each drifting smoothly with a little noise.  The same three kernel
      times, and "scan_only": the same call with every track moved 10^5 px out of the frame, so that every workgroup still walks all
      P min(t, L) candidate items and keeps none -- the gap to the full call is what the per-pixel doubles cost.  The host backend is timed on
      ONE frame (the last: a full history of 7 steps) and scaled by the clip's segment count over that frame's ("host_scaled": true).
(iii) "beside_the_model": the kernel on device tensors next to the raw-frames points call (16 points, as bench.py has them) whose tracks it
      draws, and next to the chained call (test_cfg.chain, grid4 queries) whose 25 560 tracks and visibility it draws, in this same run.
The kernel's output is compared with the host backend's with `==` before anything is timed (p256: the whole clip; grid4: the timed frame).
Caveats of every figure here: one GPU shared with other work, clocks as the box sets them -- compare the columns of one run with each
other, not with another run's.

    python tools/bench_trails.py [--iters 20] [--out profiles/trails_bench.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fgvc_amd import engine, ops, viz  # noqa: E402
from tools.bench_input import frames_u8  # noqa: E402
from tools.bench_jf import timed_events, timed_wall  # noqa: E402
from tools.bench_render import build, walks  # noqa: E402

TRAIL = 8


def drifting_grid(T, h, w, stride, seed):
    """(P, T, 2): the grid's points under one smooth motion field plus noise of 0.3 px a frame; all visible while inside the frame."""
    rng = np.random.default_rng(seed)
    q = engine.grid_queries(0, h, w, stride).numpy().astype(np.float64)[:, 1:]
    vel = np.stack([2.0 + 1.5 * np.sin(q[:, 1] / 60.0), 1.0 * np.cos(q[:, 0] / 90.0)], -1)
    tracks = q[:, None, :] + vel[:, None, :] * np.arange(T)[None, :, None] + np.cumsum(rng.normal(0.0, 0.3, (q.shape[0], T, 2)), 1)
    vis = (tracks[..., 0] >= 0) & (tracks[..., 1] >= 0) & (tracks[..., 0] < w) & (tracks[..., 1] < h)
    return tracks, vis


def kernel_times(u8, buf, tracks, vis, col, r, iters, warmup):
    kw = dict(visibles=vis, colors=col, trail=TRAIL, out=buf)
    far = tracks + 1.0e5
    return {"trails_and_dots_ms": round(timed_events(lambda: ops.render_trails(u8, tracks, radius=r, **kw), iters, warmup), 4),
            "trails_alone_ms": round(timed_events(lambda: ops.render_trails(u8, tracks, dots=False, **kw), iters, warmup), 4),
            "scan_only_ms": round(timed_events(lambda: ops.render_trails(u8, far, dots=False, **kw), iters, warmup), 4),
            "dots_only_render_ms": round(timed_events(lambda: ops.render_frames(u8, tracks=tracks, visibles=vis, colors=col, radius=r, out=buf),
                                                      iters, warmup), 4),
            "copy_ms": round(timed_events(lambda: ops.render_frames(u8, out=buf), iters, warmup), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trails_bench.json"))
    a = ap.parse_args()
    iters = max(10, a.iters)
    dev = torch.device("cuda:0")
    T, h, w = 8, 480, 854
    r = viz.default_radius(h, w)
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "frames": T, "size": [h, w], "trail": TRAIL, "linewidth": 2.0,
           "radius": r, "host_threads": torch.get_num_threads()}
    u8 = frames_u8(T, h, w, dev)
    u8_np = u8.cpu().numpy()
    buf = torch.empty_like(u8)

    def up(*xs):
        return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in xs)

    # (i) 256 points: the whole clip on the host
    tr_np, vis_np = walks(T, h, w, 256, 2)
    col_np = viz.track_colors(256)
    tr, vis, col = up(tr_np, vis_np, col_np)
    t0 = time.perf_counter()
    want = viz.render(u8_np, tracks=tr_np, visibles=vis_np, colors=col_np, radius=r, trail=TRAIL)
    host_s = time.perf_counter() - t0
    assert np.array_equal(ops.render_trails(u8, tr, vis, col, TRAIL, radius=r).cpu().numpy(), want), "p256: the kernel and the host backend differ"
    k = kernel_times(u8, buf, tr, vis, col, r, iters, a.warmup)
    k.update(P=256, host_render_s=round(host_s, 4), host_scaled=False, host_over_kernel=round(host_s * 1e3 / k["trails_and_dots_ms"], 1),
             over_dots_only_render=round(k["trails_and_dots_ms"] / k["dots_only_render_ms"], 2))
    out["p256"] = k
    print(f"# p256: {json.dumps(k)}", file=sys.stderr, flush=True)

    # (ii) the dense grid: one frame on the host, scaled
    tr_np, vis_np = drifting_grid(T, h, w, 4, 3)
    P = tr_np.shape[0]
    col_np = viz.track_colors(P)
    tr, vis, col = up(tr_np, vis_np, col_np)
    seg_ok = vis_np[:, :-1] & vis_np[:, 1:]
    clip_segments = int(sum(seg_ok[:, max(0, t - TRAIL):t].sum() for t in range(T)))
    frame_segments = int(seg_ok[:, max(0, T - 1 - TRAIL):T - 1].sum())
    canvas = u8_np[T - 1:T].copy()                                    # the host paints a frame at a time: its two stages on frame T - 1 alone
    t0 = time.perf_counter()
    ro2, g, reach = viz.trail_consts(2.0)
    stack = [None] * (T - 1) + [canvas[0]]
    viz._trails_host(stack, T - 1, tr_np, vis_np, col_np, TRAIL, ro2, g, reach, viz.trail_fade(TRAIL), None)
    trails_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    painted = viz.paint_point_track(canvas, tr_np[:, T - 1:T], vis_np[:, T - 1:T], col_np, radius=r)
    dots_s = time.perf_counter() - t0
    got = ops.render_trails(u8, tr, vis, col, TRAIL, radius=r)
    assert np.array_equal(got[T - 1].cpu().numpy(), painted[0]), "grid4: the kernel and the host backend differ on the timed frame"
    k = kernel_times(u8, buf, tr, vis, col, r, iters, a.warmup)
    host_clip_s = trails_s * clip_segments / max(1, frame_segments) + dots_s * T
    k.update(P=P, mean_step_px=round(float(np.hypot(*np.moveaxis(np.diff(tr_np, axis=1), -1, 0)).mean()), 2), segments_in_the_clip=clip_segments, segments_on_the_timed_frame=frame_segments, host_one_frame_trails_s=round(trails_s, 3),
             host_one_frame_dots_s=round(dots_s, 3), host_render_s=round(host_clip_s, 2), host_scaled=True,
             host_over_kernel=round(host_clip_s * 1e3 / k["trails_and_dots_ms"], 1),
             over_dots_only_render=round(k["trails_and_dots_ms"] / k["dots_only_render_ms"], 2),
             scan_share_of_trails_alone=round(k["scan_only_ms"] / k["trails_alone_ms"], 3))
    out["grid4"] = k
    print(f"# grid4: {json.dumps(k)}", file=sys.stderr, flush=True)

    # (iii) beside the calls whose output it draws
    gen = torch.Generator().manual_seed(1)
    Pq = 16
    qp = torch.stack([torch.zeros(Pq), torch.rand(Pq, generator=gen) * (w - 40) + 20, torch.rand(Pq, generator=gen) * (h - 40) + 20], -1)[None].to(dev)
    inp = dict(type="rgb8", size=None, layout="thwc")
    points_model = build(dev, input=inp)
    points_call = lambda: points_model(test_mode=True, rgbs=u8[None], query_points=qp, trajectories=torch.zeros(1, T, Pq, 2, device=dev),
                                       visibilities=torch.ones(1, T, Pq, device=dev))
    qg = engine.grid_queries(0, h, w, 4)[None].to(dev)
    chain_model = build(dev, input=inp, chain=dict(type="flow"))
    chain_call = lambda: chain_model(test_mode=True, rgbs=u8[None], query_points=qg, trajectories=torch.zeros(1, T, P, 2, device=dev),
                                     visibilities=torch.zeros(1, T, P, device=dev))
    n_model = max(5, iters // 3)
    with torch.no_grad():
        p_ms = timed_wall(points_call, n_model, 2)
        tr16 = points_call()[2][0].permute(1, 0, 2)                  # (16, T, 2): a strided view, read in place
        c_ms = timed_wall(chain_call, n_model, 2)
        res = chain_call()
        trc, visc = res[2][0].permute(1, 0, 2), (res[3][0] != 0).t()  # (P, T, 2), (P, T): strided views
    col16 = torch.from_numpy(viz.track_colors(Pq)).to(dev)
    rp = timed_wall(lambda: ops.render_trails(u8, tr16, None, col16, TRAIL, radius=r, out=buf), iters, a.warmup)
    rc = timed_wall(lambda: ops.render_trails(u8, trc, visc, col, TRAIL, radius=r, out=buf), iters, a.warmup)
    out["beside_the_model"] = {"points_call_ms": round(p_ms, 3), "trails_of_its_16_tracks_ms": round(rp, 4), "trails_over_points_call": round(rp / p_ms, 4),
                               "chain_call_grid4_ms": round(c_ms, 3), "trails_of_its_25560_tracks_ms": round(rc, 4),
                               "trails_over_chain_call": round(rc / c_ms, 4), "chain_visible_share": round(float(visc.float().mean()), 3),
                               "chain_mean_step_px": round(float((trc[:, 1:] - trc[:, :-1]).double().norm(dim=-1).nanmean()), 2),
                               "note": "wall clock with a device synchronisation on either side, Python included"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
