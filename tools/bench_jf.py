#!/usr/bin/env python3
"""Time the J&F scorer (fgvc_jf_counts_u8, metrics' backend='hip') and print one JSON line.

Inputs are synthetic and seeded: 480 x 854 id maps of moving ellipses plus one small object, the prediction a shifted, slightly scaled
copy of the annotation.
(a) "host_s_per_object_frame": metrics.davis_jf (the host scorer, unchanged) on --host-frames frames x 2 objects, wall clock over the
    object-frames it scores, on the threads this process was granted;
(b) "kernel_ms": one ops.jf_counts call on 70 frames x 3 objects already on the device, median of HIP-event times; "kernel_ms_in_a_burst":
    time per call of 10 calls between one pair of events (a single call between two events also counts its own start-up).  The
    kernel's 2 T h w bytes over its time are printed as "kernel_gbps_of_id_bytes": NOT a share of a roofline -- the kernel is bound by
    LDS traffic and instruction issue, and re-reads the maps once per object from cache;
(c) "davis_jf_hip_ms": metrics.davis_jf(backend='hip') end to end for that sequence, wall clock with a device synchronisation, once with
    the annotation and prediction as host arrays (uint8 / float64: rounding, upload) and once with both on the device;
(d) "mask_call_ms": the mask call (VanillaTracker, test_cfg.masks='device') on an 8-frame clip of the same size, for scale, and
    "davis_jf_hip_8f_ms": the device-side score of those 8 frames.
Medians over --iters runs (at least 20 for the kernel) after --warmup.  Caveats of every figure here: one GPU shared with other work,
clocks as the box sets them -- compare the columns of one run with each other, not with another run's.

    python tools/bench_jf.py [--iters 30] [--host-frames 8]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import metrics, ops  # noqa: E402

TEST_CFG = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, step=512, with_first=True, with_first_neighbor=True, batch_step=8)
BURST = 10


def ellipse_masks(T, h, w, n, seed, shift=(0.0, 0.0), scale=1.0):
    """(T, h, w) uint8 ids: n - 1 moving ellipses (later ids on top) and one small object (id n)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    m = np.zeros((T, h, w), np.uint8)
    for k in range(1, n + 1):
        small = k == n
        c = np.array([rng.uniform(0.3, 0.7) * h, rng.uniform(0.25, 0.75) * w])
        v = rng.uniform(-1.0, 1.0, 2) * np.array([h, w]) / 150.0
        ax = np.array([0.03 * h, 0.02 * w]) if small else np.array([rng.uniform(0.12, 0.25) * h, rng.uniform(0.08, 0.2) * w])
        for t in range(T):
            cy, cx = c + v * t + np.asarray(shift)
            m[t][((yy - cy) / (ax[0] * scale)) ** 2 + ((xx - cx) / (ax[1] * scale)) ** 2 <= 1.0] = k
    return m


def timed_events(fn, iters, warmup):
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


def timed_wall(fn, iters, warmup):
    ms = []
    for it in range(warmup + iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-frames", type=int, default=8)
    ap.add_argument("--frames", type=int, default=70)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    a = ap.parse_args()
    iters = max(20, a.iters)
    h, w = a.size
    dev = torch.device("cuda:0")
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "size": [h, w], "radius": metrics.jf_radius((h, w)),
           "host_threads": torch.get_num_threads()}

    # (a) the host scorer, a few frames only
    gt2, pr2 = ellipse_masks(a.host_frames, h, w, 2, 0), ellipse_masks(a.host_frames, h, w, 2, 0, shift=(3.0, -2.0), scale=1.05)
    t0 = time.perf_counter()
    host = metrics.davis_jf({"s": (gt2, pr2.astype(np.float64))})
    dt = time.perf_counter() - t0
    scored = (a.host_frames - 2 if a.host_frames > 2 else a.host_frames) * 2
    out["host"] = {"frames": a.host_frames, "objects": 2, "seconds": round(dt, 3), "host_s_per_object_frame": round(dt / scored, 4)}
    assert metrics.davis_jf({"s": (gt2, pr2.astype(np.float64))}, backend="hip") == host       # the same numbers

    # (b) the kernel alone, (c) the scorer end to end: 70 frames x 3 objects
    T, n, r = a.frames, 3, metrics.jf_radius((h, w))
    gt, pr = ellipse_masks(T, h, w, n, 1), ellipse_masks(T, h, w, n, 1, shift=(3.0, -2.0), scale=1.05)
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pr).to(dev)
    counts = torch.empty((T, n, 6), device=dev, dtype=torch.int64)
    k_ms = timed_events(lambda: ops.jf_counts(g, p, n, r, out=counts), iters, a.warmup)
    b_ms = timed_events(lambda: [ops.jf_counts(g, p, n, r, out=counts) for _ in range(BURST)], iters, a.warmup) / BURST
    nbytes = 2 * T * h * w
    out["kernel"] = {"frames": T, "objects": n, "kernel_ms": round(k_ms, 4), "kernel_ms_in_a_burst": round(b_ms, 4), "id_bytes": nbytes,
                     "kernel_gbps_of_id_bytes": round(nbytes / (k_ms * 1e-3) / 1e9, 1),
                     "kernel_us_per_object_frame": round(k_ms * 1e3 / (T * n), 3)}
    pr64 = pr.astype(np.float64)
    e_host = timed_wall(lambda: metrics.davis_jf({"s": (gt, pr64)}, backend="hip"), max(5, iters // 4), 2)
    e_dev = timed_wall(lambda: metrics.davis_jf({"s": (g, p)}, backend="hip"), iters, a.warmup)
    up = timed_wall(lambda: (torch.from_numpy(gt).to(dev), metrics._device_ids(pr64, n)), max(5, iters // 4), 2)
    fin = timed_wall(lambda: metrics.jf_from_counts(counts), iters, a.warmup)
    out["davis_jf_hip_ms"] = {"frames": T, "objects": n, "host_arrays_in": round(e_host, 3), "device_tensors_in": round(e_dev, 3),
                              "of_which_round_and_upload_ms": round(up, 3), "of_which_counts_to_JF_on_host_ms": round(fin, 3)}

    # (d) the mask call on 8 frames of the same size, and the device-side score of the same 8 frames
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,),
                                                                       pool_type="none", zero_init_residual=False)),
                            train_cfg=None, test_cfg=api.ConfigDict(**TEST_CFG, masks="device"))
    torch.manual_seed(0)
    model.init_weights()
    model = model.to(dev).eval()
    gen = torch.Generator().manual_seed(2)
    imgs = torch.randn(1, 1, 3, 8, h, w, generator=gen).to(dev)
    call = dict(test_mode=True, imgs=imgs, ref_seg_map=g[:1], img_meta=[dict(original_shape=(h, w))])
    with torch.no_grad():
        m_ms = timed_wall(lambda: model(**call), max(5, iters // 3), 3)
        pred8 = model(**call)[0]
    s_ms = timed_wall(lambda: metrics.davis_jf({"s": (g[:8], pred8)}, backend="hip"), iters, a.warmup)
    out["mask_call_8f"] = {"frames": 8, "mask_call_ms": round(m_ms, 3), "davis_jf_hip_8f_ms": round(s_ms, 3),
                           "score_over_mask_call": round(s_ms / m_ms, 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
