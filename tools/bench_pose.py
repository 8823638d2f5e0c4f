#!/usr/bin/env python3
"""Time the pose renderer (fgvc_render_pose_u8, fgvc_amd.viz) and the joint peaks (fgvc_heatmap_coords_peak_f32), print
one JSON line and write it to profiles/pose_bench.json.

Inputs are synthetic and seeded.  Two geometries: "jhmdb" 40 x 240 x 320 with K = 15 joints and viz.JHMDB_SKELETON, "davis" 8 x 480 x 854
with K = 16 joints on a chain of 15 limbs.  The maps come from a synthetic label bank on a stride-2 feature grid through
ops.softmap_readout (float32), the joints from ops.heatmap_coords on the same bank: what the tools draw.  Per geometry:
(i)   one ops.render_pose call with everything on the device and `out` given -- heat + limbs + dots, heat alone, limbs alone, heat + limbs
      -- beside the dots-only ops.render_frames and its plain copy, medians of HIP-event times; the bytes each call moves (frames in and
      out, 4 K bytes a pixel of maps) over its time, as a share of 8 TB/s;
(ii)  viz.render(..., backend='host') on the same inputs, wall clock, the whole clip, after an `==` check of the kernel against it;
(iii) the maps' way to the picture: softmap_readout + render_pose on the device, against copying the (T, K, h, w) float32 stack to the
      host (what looking at a return_maps=True result costs before any painting);
(iv)  the peak entry against the plain coordinate entry.
With --parent-lib PATH (the parent commit's libfgvc_hip.so) the two sibling kernels, fgvc_render_frames_u8 and fgvc_render_trails_u8, are
timed in THIS process through either library in turns, on tools/bench_trails.py's 256-point clip.
Caveats of every figure here: one GPU shared with other work, clocks as the box sets them -- compare the columns of one run with each
other, not with another run's.

    python tools/bench_pose.py [--iters 20] [--parent-lib build/parent/libfgvc_hip.so [--sibling-rounds 3] [--siblings-only]]
                               [--out profiles/pose_bench.json]
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fgvc_amd import _lib, engine, ops, viz  # noqa: E402
from tools.bench_input import frames_u8  # noqa: E402
from tools.bench_jf import timed_events, timed_wall  # noqa: E402
from tools.bench_render import walks  # noqa: E402

PEAK_BW = 8.0e12   # bytes / s, the MI355X's HBM figure the shares below are taken of


def label_bank(T, Hf, Wf, K, seed):
    """(T, HfWf, K) f32: one bump per joint, drifting over the frames, as propagated labels look."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:Hf, 0:Wf]
    c0 = np.stack([rng.uniform(0.2, 0.8, K) * Hf, rng.uniform(0.2, 0.8, K) * Wf], -1)
    vel = rng.normal(0.0, 0.6, (K, 2))
    b = np.zeros((T, Hf, Wf, K), np.float32)
    for t in range(T):
        for k in range(K):
            cy, cx = c0[k] + vel[k] * t
            b[t, :, :, k] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 2.5 ** 2)) * (1.0 - 0.01 * t)
    return torch.from_numpy(b.reshape(T, Hf * Wf, K))


def geometry(dev, name, T, h, w, K, skeleton, iters, warmup):
    d = 2
    _, map_pad = engine.pad_divide_by(h, w, d)
    Hf, Wf = (h + map_pad[2] + map_pad[3]) // d, (w + map_pad[0] + map_pad[1]) // d
    bank = label_bank(T, Hf, Wf, K, 5).to(dev)
    heat0 = bank[0].reshape(Hf, Wf, K).permute(2, 0, 1)[None]
    heat0 = torch.nn.functional.interpolate(heat0, size=(h + map_pad[2] + map_pad[3], w + map_pad[0] + map_pad[1]), mode="bilinear")[0]
    heat0 = heat0[:, map_pad[2]:map_pad[2] + h, map_pad[0]:map_pad[0] + w].contiguous()
    u8 = frames_u8(T, h, w, dev)
    buf = torch.empty_like(u8)
    r = viz.default_radius(h, w)
    maps = ops.softmap_readout(bank, heat0, Hf, Wf, map_pad, (h, w), out_dtype=torch.float32)
    coords, peak = ops.heatmap_coords(bank, heat0, Hf, Wf, map_pad, (h, w), peak=True)
    tracks = torch.from_numpy(viz.pose_tracks(coords.cpu().numpy())).to(dev)
    vis = torch.from_numpy(viz.pose_visibles(coords.cpu().numpy(), peak.cpu().numpy(), 0.05)).to(dev)
    col = torch.from_numpy(viz.track_colors(K)).to(dev)
    sk = np.ascontiguousarray(skeleton)                               # a host table: checked there, uploaded once (ops.render_pose)
    pts = dict(tracks=tracks, visibles=vis, colors=col)
    full = dict(pts, skeleton=sk, heat=maps, heat_colors=col, radius=r)

    t0 = time.perf_counter()
    want = viz.render(u8.cpu().numpy(), tracks=tracks.cpu().numpy(), visibles=vis.cpu().numpy(), colors=col.cpu().numpy(), radius=r,
                      skeleton=skeleton, heat=maps.cpu().numpy(), heat_colors=col.cpu().numpy())
    host_s = time.perf_counter() - t0
    assert np.array_equal(ops.render_pose(u8, **full).cpu().numpy(), want), f"{name}: the kernel and the host backend differ"

    def ms(fn):
        return round(timed_events(fn, iters, warmup), 4)
    k = {"frames": T, "size": [h, w], "K": K, "limbs": int(skeleton.shape[0]), "radius": r,
         "heat_limbs_dots_ms": ms(lambda: ops.render_pose(u8, out=buf, **full)),
         "heat_alone_ms": ms(lambda: ops.render_pose(u8, heat=maps, heat_colors=col, out=buf)),
         "limbs_alone_ms": ms(lambda: ops.render_pose(u8, skeleton=sk, dots=False, out=buf, **pts)),
         "heat_limbs_ms": ms(lambda: ops.render_pose(u8, skeleton=sk, heat=maps, heat_colors=col, dots=False, out=buf, **pts)),
         "dots_only_render_frames_ms": ms(lambda: ops.render_frames(u8, radius=r, out=buf, **pts)),
         "copy_ms": ms(lambda: ops.render_frames(u8, out=buf))}
    frame_bytes, map_bytes = 2 * u8.numel(), maps.numel() * 4
    k["bytes_moved_with_heat"] = frame_bytes + map_bytes
    k["heat_alone_gbps"] = round((frame_bytes + map_bytes) / k["heat_alone_ms"] / 1e6, 1)
    k["heat_alone_share_of_8tbps"] = round((frame_bytes + map_bytes) / (k["heat_alone_ms"] * 1e-3) / PEAK_BW, 4)
    k["copy_gbps"] = round(frame_bytes / k["copy_ms"] / 1e6, 1)
    k.update(host_render_s=round(host_s, 3), host_over_kernel=round(host_s * 1e3 / k["heat_limbs_dots_ms"], 1))
    # (iii) the maps' way to the picture
    mbuf = torch.empty_like(maps)
    k["softmap_readout_ms"] = ms(lambda: ops.softmap_readout(bank, heat0, Hf, Wf, map_pad, (h, w), out=mbuf))
    k["readout_plus_render_ms"] = ms(lambda: ops.render_pose(u8, heat=ops.softmap_readout(bank, heat0, Hf, Wf, map_pad, (h, w), out=mbuf),
                                                             heat_colors=col, out=buf))
    k["map_stack_bytes"] = map_bytes
    k["map_stack_to_host_ms"] = round(timed_wall(lambda: maps.cpu(), max(5, iters // 4), 1), 3)
    k["host_copy_over_readout_plus_render"] = round(k["map_stack_to_host_ms"] / k["readout_plus_render_ms"], 1)
    # (iv) the peaks
    k["heatmap_coords_ms"] = ms(lambda: ops.heatmap_coords(bank, heat0, Hf, Wf, map_pad, (h, w)))
    k["heatmap_coords_peak_ms"] = ms(lambda: ops.heatmap_coords(bank, heat0, Hf, Wf, map_pad, (h, w), peak=True))
    print(f"# {name}: {json.dumps(k)}", file=sys.stderr, flush=True)
    return k


@contextlib.contextmanager
def through(lib):
    """ops' calls go to `lib` inside the block (as _lib.ablations() does for the experiment library)."""
    prod = _lib.load()
    _lib._lib = lib
    try:
        yield
    finally:
        _lib._lib = prod


def siblings(dev, parent_path, iters, warmup, rounds=3):
    """fgvc_render_frames_u8 and fgvc_render_trails_u8 through the parent commit's library and this one, in turns, in one process."""
    parent = ctypes.CDLL(parent_path)
    for name in ("fgvc_render_frames_u8", "fgvc_render_trails_u8", "fgvc_last_error"):    # (the parent has no pose entry: only what is timed)
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    T, h, w = 8, 480, 854
    r = viz.default_radius(h, w)
    u8 = frames_u8(T, h, w, dev)
    buf = torch.empty_like(u8)
    tr_np, vis_np = walks(T, h, w, 256, 2)
    tr, vis = torch.from_numpy(tr_np).to(dev), torch.from_numpy(vis_np).to(dev)
    col = torch.from_numpy(viz.track_colors(256)).to(dev)
    fade = torch.from_numpy(np.array(viz.trail_fade(8))).to(dev)
    calls = {"render_frames_ms": lambda: ops.render_frames(u8, tracks=tr, visibles=vis, colors=col, radius=r, out=buf),
             "render_trails_ms": lambda: ops.render_trails(u8, tr, vis, col, 8, fade=fade, radius=r, out=buf)}
    res = {"parent": {k: [] for k in calls}, "change": {k: [] for k in calls}}
    got = {}
    for _ in range(rounds):
        for arm, lib in (("parent", parent), ("change", _lib.load())):
            with through(lib):
                for k, fn in calls.items():
                    res[arm][k].append(round(timed_events(fn, iters, warmup), 4))
                    got[(arm, k)] = buf.clone()
    for k in calls:
        assert torch.equal(got[("parent", k)], got[("change", k)]), f"{k}: the two libraries paint different bytes"
    out = {"points": 256, "frames": T, "size": [h, w], "rounds": rounds}
    for arm in res:
        for k, v in res[arm].items():
            out[f"{arm}_{k}"] = {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v)}
    print(f"# siblings: {json.dumps(out)}", file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libfgvc_hip.so built from the parent commit: time the two sibling kernels through both")
    ap.add_argument("--sibling-rounds", type=int, default=3, help="with --parent-lib: turns per library")
    ap.add_argument("--siblings-only", action="store_true", help="with --parent-lib: skip the two geometries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_bench.json"))
    a = ap.parse_args()
    iters = max(10, a.iters)
    dev = torch.device("cuda:0")
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "host_threads": torch.get_num_threads(),
           "date": time.strftime("%Y-%m-%d")}
    if a.siblings_only and not a.parent_lib:
        ap.error("--siblings-only goes with --parent-lib")
    if not a.siblings_only:
        out["jhmdb"] = geometry(dev, "jhmdb", 40, 240, 320, 15, viz.JHMDB_SKELETON, iters, a.warmup)
        chain = np.stack([np.arange(15), np.arange(1, 16)], -1).astype(np.int32)
        out["davis"] = geometry(dev, "davis", 8, 480, 854, 16, chain, iters, a.warmup)
    if a.parent_lib:
        out["siblings"] = siblings(dev, a.parent_lib, iters, a.warmup, max(1, a.sibling_rounds))
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
