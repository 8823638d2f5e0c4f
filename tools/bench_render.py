#!/usr/bin/env python3
"""Time the renderer (fgvc_render_frames_u8, fgvc_amd.viz), print one JSON line and write it to
profiles/render_bench.json.

Inputs are synthetic and seeded: 8 frames of 480 x 854 uint8, 256 points on random walks (a few leave the frame, a tenth invisible), id maps
of 3 objects (moving ellipses, tools/bench_jf.py's).  Radius 7, the reference's for this size.
(i)   "kernel": one ops.render_frames call with everything on the device and `out` given -- overlay + points, overlay alone, points alone,
      neither (a copy) -- median of HIP-event times, and the time per call of 20 calls between one pair of events ("in_a_burst": a single call
      between two events also counts its own start-up).  The kernel's algorithmic bytes, T H W 7 (3 read + 1 id + 3 written), over its time
      as a share of the 8 TB/s HBM figure the README uses;
(ii)  "host": viz.render(backend='host') on the same inputs, wall clock, on the threads this process was granted (numpy: one of them);
(iii) "beside_the_model": the raw-frames points call (VanillaTracker, test_cfg.input, 16 points as bench.py has them) and the mask call
      (test_cfg.masks='device') on a clip of the same size, each next to the render call that annotates ITS output, in this same run.
The kernel's output is compared with the host backend's with `==` before anything is timed.  Caveats of every figure here: one GPU shared
with other work, clocks as the box sets them -- compare the columns of one run with each other, not with another run's.

    python tools/bench_render.py [--iters 30] [--out profiles/render_bench.json]
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
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import ops, viz  # noqa: E402
from tools.bench_input import frames_u8  # noqa: E402
from tools.bench_jf import ellipse_masks, timed_events, timed_wall  # noqa: E402

TEST_CFG = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, step=512, with_first=True, with_first_neighbor=True, batch_step=8)
HBM_TBPS = 8.0
BURST = 20


def walks(T, h, w, P, seed):
    rng = np.random.default_rng(seed)
    start = np.stack([rng.uniform(-4.0, w + 4.0, P), rng.uniform(-4.0, h + 4.0, P)], -1)
    tracks = start[:, None, :] + np.cumsum(rng.normal(0.0, 2.5, (P, T, 2)), 1)
    return tracks, rng.random((P, T)) > 0.1


def build(dev, **extra):
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,),
                                                                       pool_type="none", zero_init_residual=False)),
                            train_cfg=None, test_cfg=api.ConfigDict(**TEST_CFG, **extra))
    torch.manual_seed(0)
    model.init_weights()
    return model.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    a = ap.parse_args()
    iters = max(20, a.iters)
    dev = torch.device("cuda:0")
    T, h, w, P, n = 8, 480, 854, 256, 3
    r = viz.default_radius(h, w)
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "frames": T, "size": [h, w], "points": P, "objects": n,
           "radius": r, "host_threads": torch.get_num_threads()}

    u8 = frames_u8(T, h, w, dev)
    ids_np = ellipse_masks(T, h, w, n, 1)
    tracks_np, vis_np = walks(T, h, w, P, 2)
    col_np = viz.track_colors(P)
    ids, tracks, vis, col = (torch.from_numpy(x).to(dev) for x in (ids_np, tracks_np, vis_np, col_np))
    buf = torch.empty_like(u8)
    full = dict(ids=ids, tracks=tracks, visibles=vis, colors=col, radius=r)

    # the same bytes as the host backend, before anything is timed; (ii) the host backend's wall clock on the way
    t0 = time.perf_counter()
    want = viz.render(u8.cpu().numpy(), ids=ids_np, tracks=tracks_np, visibles=vis_np, colors=col_np, radius=r)
    host_s = time.perf_counter() - t0
    assert np.array_equal(ops.render_frames(u8, out=buf, **full).cpu().numpy(), want), "the kernel and the host backend differ"
    t0 = time.perf_counter()
    viz.paint_point_track(u8.cpu().numpy(), tracks_np, vis_np, col_np, radius=r)
    out["host"] = {"render_s": round(host_s, 4), "points_alone_s": round(time.perf_counter() - t0, 4),
                   "painted_pixels": int((want != u8.cpu().numpy()).any(-1).sum())}

    # (i) the kernel alone
    nbytes = T * h * w * 7
    k = {}
    for name, kw in (("overlay_and_points", full), ("overlay", dict(ids=ids)), ("points", {x: full[x] for x in ("tracks", "visibles", "colors", "radius")}),
                     ("copy", {})):
        one = timed_events(lambda: ops.render_frames(u8, out=buf, **kw), iters, a.warmup)
        many = timed_events(lambda: [ops.render_frames(u8, out=buf, **kw) for _ in range(BURST)], iters, a.warmup) / BURST
        k[name] = {"kernel_ms": round(one, 4), "kernel_ms_in_a_burst": round(many, 4)}
    one, many = k["overlay_and_points"]["kernel_ms"], k["overlay_and_points"]["kernel_ms_in_a_burst"]
    k.update(algorithmic_bytes=nbytes, tbps=round(nbytes / (one * 1e-3) / 1e12, 3), share_of_hbm_8tbps=round(nbytes / (one * 1e-3) / 1e12 / HBM_TBPS, 4),
             tbps_in_a_burst=round(nbytes / (many * 1e-3) / 1e12, 3), share_of_hbm_8tbps_in_a_burst=round(nbytes / (many * 1e-3) / 1e12 / HBM_TBPS, 4),
             host_render_over_kernel=round(host_s * 1e3 / one, 1))
    out["kernel"] = k

    # (iii) beside the model calls it annotates
    g = torch.Generator().manual_seed(1)
    Pq = 16
    qp = torch.stack([torch.zeros(Pq), torch.rand(Pq, generator=g) * (w - 40) + 20, torch.rand(Pq, generator=g) * (h - 40) + 20], -1)[None].to(dev)
    traj0, vis0 = torch.zeros(1, T, Pq, 2, device=dev), torch.ones(1, T, Pq, device=dev)
    points_model = build(dev, input=dict(type="rgb8", size=None, layout="thwc"))
    mask_model = build(dev, input=dict(type="rgb8", size=None, layout="thwc"), masks="device")
    points_call = lambda: points_model(test_mode=True, rgbs=u8[None], query_points=qp, trajectories=traj0, visibilities=vis0)
    mask_call = lambda: mask_model(test_mode=True, imgs=u8[None, None], ref_seg_map=ids[:1], img_meta=[dict(original_shape=(h, w))])
    with torch.no_grad():
        p_ms = timed_wall(points_call, max(5, iters // 3), 3)
        m_ms = timed_wall(mask_call, max(5, iters // 3), 3)
        tr16 = points_call()[2][0].permute(1, 0, 2)                  # (16, T, 2): a strided view, read in place
        pred = mask_call()[0]
    rp = timed_wall(lambda: ops.render_frames(u8, tracks=tr16, radius=r, out=buf), iters, a.warmup)
    rm = timed_wall(lambda: ops.render_frames(u8, ids=pred, out=buf), iters, a.warmup)
    rf = timed_wall(lambda: ops.render_frames(u8, out=buf, **full), iters, a.warmup)
    out["beside_the_model"] = {"points_call_ms": round(p_ms, 3), "render_its_16_tracks_ms": round(rp, 4), "mask_call_ms": round(m_ms, 3),
                               "render_its_masks_ms": round(rm, 4), "render_256_points_and_masks_ms": round(rf, 4),
                               "render_over_points_call": round(rp / p_ms, 4), "render_over_mask_call": round(rm / m_ms, 4),
                               "note": "wall clock with a device synchronisation on either side, Python included"}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
