#!/usr/bin/env python3
"""Time the input stage (fgvc_frames_rgb8_to_lab_f32, test_cfg.input) and print one JSON line.

(a) the datasets' torch chain (datasets.preprocess_tapvid_frames on the device: some sixty element-wise launches) against the kernel alone,
    on uint8 frames already on the device: 8 x 480 x 854 at the same size and 8 x 1080 x 1920 -> 480 x 854;
(b) one whole points call at bench.py's geometry (8 frames of 480 x 854, strides (1, 2, 1, 1), 16 points): the chain followed by the call
    on its float frames, against the call on the uint8 frames with test_cfg.input set;
(c) the kernel's bytes (uint8 read once + f32 written once) over its time, against the 8 TB/s HBM figure the README uses; "in_a_burst" is
    the time per launch of 20 launches between one pair of events (a single launch between two events also counts its own start-up; at
    the same size the burst re-reads 10 MB of frames that the 256 MiB cache then holds, the 39 MB written per launch go out).
Per geometry also E_chain / E_kernel, the largest absolute error of either against the float64 restatement of the contract.
Medians of HIP-event times over --iters runs (at least 20) after --warmup.  Caveats of every figure here: one GPU shared with other work,
clocks as the box sets them -- compare the columns of one run with each other, not with another run's.

    python tools/bench_input.py [--iters 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import ops  # noqa: E402
from fgvc_amd.datasets import preprocess_tapvid_frames  # noqa: E402
from tests.input_cases import preprocess_f64  # noqa: E402

TEST_CFG = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, step=512, with_first=True, with_first_neighbor=True, batch_step=8)
HBM_TBPS = 8.0
BURST = 20          # launches between one pair of events for "in_a_burst": the launch's own latency overlaps the launch before it


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


def frames_u8(T, h, w, dev, seed=0):
    """A smooth random texture plus noise, as decoded video is: every byte value occurs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.nn.functional.interpolate(torch.rand(T, 3, h // 8 + 2, w // 8 + 2, generator=g), size=(h, w), mode="bilinear", align_corners=False)
    x = (x * 300.0 - 22.0 + 6.0 * torch.randn(T, 3, h, w, generator=g)).round().clamp(0, 255).to(torch.uint8)
    return x.permute(0, 2, 3, 1).contiguous().to(dev)


def kernel_vs_chain(dev, T, src, size, iters, warmup):
    u8 = frames_u8(T, src[0], src[1], dev)
    out = torch.empty((T, 3, size[0], size[1]), device=dev, dtype=torch.float32)
    chain_ms = timed(lambda: preprocess_tapvid_frames(u8, size), iters, warmup)
    kernel_ms = timed(lambda: ops.frames_to_lab(u8, size, out=out), iters, warmup)
    many_ms = timed(lambda: [ops.frames_to_lab(u8, size, out=out) for _ in range(BURST)], iters, warmup) / BURST
    nbytes = u8.numel() + out.numel() * 4
    r = {"frames": T, "source": list(src), "size": list(size), "chain_ms": round(chain_ms, 4), "kernel_ms": round(kernel_ms, 4),
         "kernel_ms_in_a_burst": round(many_ms, 4), "chain_over_kernel": round(chain_ms / kernel_ms, 2), "kernel_bytes": nbytes,
         "kernel_tbps": round(nbytes / (kernel_ms * 1e-3) / 1e12, 3), "share_of_hbm_8tbps": round(nbytes / (kernel_ms * 1e-3) / 1e12 / HBM_TBPS, 3),
         "kernel_tbps_in_a_burst": round(nbytes / (many_ms * 1e-3) / 1e12, 3)}
    # both against the float64 restatement of the contract (tests/input_cases.py, on the CPU), first two frames: the rows of DESIGN's error table
    want = preprocess_f64(u8[:2], size)
    r["E_chain_vs_float64"] = float((preprocess_tapvid_frames(u8[:2], size)[0].cpu().double() - want).abs().max())
    r["E_kernel_vs_float64"] = float((out[:2].cpu().double() - want).abs().max())
    return r


def whole_call(dev, T, size, strides, P, iters, warmup):
    h, w = size
    u8 = frames_u8(T, h, w, dev, seed=1)
    g = torch.Generator().manual_seed(1)
    qp = torch.stack([torch.zeros(P), torch.rand(P, generator=g) * (w - 40) + 20, torch.rand(P, generator=g) * (h - 40) + 20], -1)[None].to(dev)
    traj, vis = torch.zeros(1, T, P, 2, device=dev), torch.ones(1, T, P, device=dev)
    model = build(strides, dev, input=dict(type="rgb8", size=None, layout="thwc"))
    floats = lambda: model(test_mode=True, rgbs=preprocess_tapvid_frames(u8, size), query_points=qp, trajectories=traj, visibilities=vis)
    raw = lambda: model(test_mode=True, rgbs=u8[None], query_points=qp, trajectories=traj, visibilities=vis)
    lab = preprocess_tapvid_frames(u8, size)
    call_only = lambda: model(test_mode=True, rgbs=lab, query_points=qp, trajectories=traj, visibilities=vis)
    with torch.no_grad():
        a1 = timed(floats, iters, warmup)
        b1 = timed(raw, iters, warmup)
        c1 = timed(call_only, iters, warmup)
        a2 = timed(floats, iters, warmup)                        # the same two again, the other way round: the spread of the box
        b2 = timed(raw, iters, warmup)
        d = float((floats()[2] - raw()[2]).abs().max())
    return {"frames": T, "size": [h, w], "strides": list(strides), "points": P, "chain_plus_call_ms": [round(a1, 3), round(a2, 3)],
            "raw_call_ms": [round(b1, 3), round(b2, 3)], "call_on_float_frames_ms": round(c1, 3),
            "chain_plus_call_over_raw_call": round(min(a1, a2) / min(b1, b2), 3), "max_abs_traj_difference_px": d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    iters = max(20, a.iters)
    dev = torch.device("cuda:0")
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    out["same_size_8x480x854"] = kernel_vs_chain(dev, 8, (480, 854), (480, 854), iters, a.warmup)
    out["resize_8x1080x1920_to_480x854"] = kernel_vs_chain(dev, 8, (1080, 1920), (480, 854), iters, a.warmup)
    out["points_call_bench_480p_8f"] = whole_call(dev, 8, (480, 854), (1, 2, 1, 1), 16, iters, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
