#!/usr/bin/env python3
"""Time the YUV 4:2:0 output stage (fgvc_frames_rgb8_to_yuv420, ops.rgb_frames_to_yuv420, viz.frames_to_yuv420) and print
one JSON line.

(a) per format (I420, NV12) and size (8 x 480 x 854, 8 x 1080 x 1920), on RGB frames already on the device: the kernel against
    datasets.rgb8_to_yuv420 followed by datasets.pack_yuv420 run as torch launches on the same tensors (the contract, on the same GPU); beside
    it fgvc_frames_yuv420_to_rgb8 on the encoded clip, the sibling that moves the same bytes the other way; each kernel's bytes (frames read
    once + planes written once: 4.5 a pixel) over its time against the 8 TB/s figure; the kernel alone in a burst of launches (what a launch
    costs drops out); and E_bytes, the bytes in which the kernel differs from the chain (the contract: 0).
(b) at bench.py's geometry (8 frames of 480 x 854, strides (1, 2, 1, 1), 16 points): the points call, the render launch, the encode launch,
    render + encode, and the copy to the host of the packed frames (1.5 bytes a pixel) next to that of the RGB frames (3).
Medians of HIP-event times over --iters runs (at least 20) after --warmup, each with its 10th and 90th percentile.  One GPU shared with other
work, clocks as the box sets them: compare the columns of one run with each other, not with another run's.

    python tools/bench_yuv_out.py [--iters 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgvc_amd import datasets, ops, viz  # noqa: E402
from tools.bench_input import build, frames_u8  # noqa: E402

HBM_TBPS = 8.0
BURST = 20
YUV = dict(matrix="bt709", range="limited", siting="left")


def timed(fn, iters, warmup):
    """[median, 10th percentile, 90th percentile] ms of fn() between HIP events."""
    ms = []
    for it in range(warmup + iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if it >= warmup:
            ms.append(e0.elapsed_time(e1))
    ms.sort()
    return [round(ms[len(ms) // 2], 4), round(ms[len(ms) // 10], 4), round(ms[len(ms) * 9 // 10], 4)]


def kernel_vs_chain(dev, T, h, w, fmt, iters, warmup):
    rgb = frames_u8(T, h, w, dev)
    out = torch.empty((T, 3 * h // 2, w), device=dev, dtype=torch.uint8)
    back = torch.empty((T, h, w, 3), device=dev, dtype=torch.uint8)
    planes = ops.yuv420_planes(out, fmt)
    chain = timed(lambda: datasets.pack_yuv420(*datasets.rgb8_to_yuv420(rgb, **YUV), fmt), iters, warmup)
    kernel = timed(lambda: ops.rgb_frames_to_yuv420(rgb, fmt, out=out, **YUV), iters, warmup)
    burst = [round(x / BURST, 4) for x in timed(lambda: [ops.rgb_frames_to_yuv420(rgb, fmt, out=out, **YUV) for _ in range(BURST)], iters, warmup)]
    sibling = timed(lambda: ops.yuv_frames_to_rgb8(*planes, out=back, **YUV), iters, warmup)
    nbytes = rgb.numel() + out.numel()
    want = datasets.pack_yuv420(*datasets.rgb8_to_yuv420(rgb, **YUV), fmt)
    return {"format": fmt, "frames": T, "size": [h, w], "chain_ms": chain, "kernel_ms": kernel, "kernel_ms_in_a_burst": burst,
            "chain_over_kernel": round(chain[0] / kernel[0], 2), "sibling_yuv420_to_rgb8_ms": sibling, "bytes": nbytes,
            "kernel_tbps": round(nbytes / (kernel[0] * 1e-3) / 1e12, 3), "share_of_hbm_8tbps": round(nbytes / (kernel[0] * 1e-3) / 1e12 / HBM_TBPS, 3),
            "kernel_tbps_in_a_burst": round(nbytes / (burst[0] * 1e-3) / 1e12, 3),
            "share_of_hbm_8tbps_in_a_burst": round(nbytes / (burst[0] * 1e-3) / 1e12 / HBM_TBPS, 3),
            "sibling_tbps": round(nbytes / (sibling[0] * 1e-3) / 1e12, 3), "E_bytes_vs_chain": int((out != want).sum())}


def next_to_the_points_call(dev, T, size, strides, P, iters, warmup):
    h, w = size
    rgb = frames_u8(T, h, w, dev, seed=1)
    g = torch.Generator().manual_seed(1)
    qp = torch.stack([torch.zeros(P), torch.rand(P, generator=g) * (w - 40) + 20, torch.rand(P, generator=g) * (h - 40) + 20], -1)[None].to(dev)
    kw = dict(query_points=qp, trajectories=torch.zeros(1, T, P, 2, device=dev), visibilities=torch.ones(1, T, P, device=dev))
    model = build(strides, dev, input=dict(type="rgb8", size=None, layout="thwc"))
    with torch.no_grad():
        call = timed(lambda: model(test_mode=True, rgbs=rgb[None], **kw), iters, warmup)
        tracks = model(test_mode=True, rgbs=rgb[None], **kw)[2][0].permute(1, 0, 2).double().contiguous()          # (P, T, 2)
    painted = torch.empty_like(rgb)
    packed = torch.empty((T, 3 * h // 2, w), device=dev, dtype=torch.uint8)
    render = timed(lambda: ops.render_frames(rgb, tracks=tracks, out=painted), iters, warmup)
    encode = timed(lambda: ops.rgb_frames_to_yuv420(painted, "i420", out=packed, **YUV), iters, warmup)
    both = timed(lambda: ops.rgb_frames_to_yuv420(ops.render_frames(rgb, tracks=tracks, out=painted), "i420", out=packed, **YUV), iters, warmup)
    to_host_rgb = timed(lambda: painted.cpu(), iters, warmup)
    to_host_packed = timed(lambda: packed.cpu(), iters, warmup)
    assert torch.equal(packed.cpu(), torch.from_numpy(viz.frames_to_yuv420(painted.cpu().numpy(), "i420", backend="host", **YUV)))
    return {"frames": T, "size": [h, w], "strides": list(strides), "points": P, "points_call_ms": call, "render_ms": render, "encode_ms": encode,
            "render_plus_encode_ms": both, "render_plus_encode_over_points_call": round(both[0] / call[0], 4),
            "to_host_rgb_ms": to_host_rgb, "to_host_packed_ms": to_host_packed}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    iters = max(20, a.iters)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_yuv_out.py times the GPU (fgvc_amd has no CPU path)")
    dev = torch.device("cuda:0")
    out = {"iters": iters, "warmup": a.warmup, "times": "[median, 10th percentile, 90th percentile] ms", "device": torch.cuda.get_device_name(0)}
    for fmt in ("i420", "nv12"):
        for h, w in ((480, 854), (1080, 1920)):
            out[f"8x{h}x{w}_{fmt}"] = kernel_vs_chain(dev, 8, h, w, fmt, iters, a.warmup)
    out["next_to_the_points_call_480p_8f"] = next_to_the_points_call(dev, 8, (480, 854), (1, 2, 1, 1), 16, iters, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
