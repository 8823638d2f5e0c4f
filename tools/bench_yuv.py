#!/usr/bin/env python3
"""Time the YUV 4:2:0 input stage (fgvc_frames_yuv420_to_lab_f32, fgvc_frames_yuv420_to_rgb8, test_cfg.input type='nv12' | 'i420'; DESIGN.md
section 19) and print one JSON line.

(a) per format (NV12, I420) and geometry (8 x 480 x 854 at the same size; 8 x 1080 x 1920 -> 480 x 854), on planes already on the device:
    the Lab kernel against datasets.preprocess_yuv420_frames (the torch chain on the same GPU), the bytes kernel against
    datasets.yuv420_to_rgb8, each kernel's bytes (planes read once + output written once) over its time, and E_chain / E_kernel, the largest
    absolute error of the chain and of the Lab kernel against the float64 restatement of the contract (tests/yuv_cases.py, first two frames);
    E_bytes counts the bytes of the bytes kernel that differ from the numpy float32 restatement (the contract: 0).
(b) one whole points call at bench.py's geometry (8 frames of 480 x 854, strides (1, 2, 1, 1), 16 points) on packed I420 frames with
    test_cfg.input = dict(type='i420'), against the torch chain followed by the call on its float frames, and against the rgb8 call on
    ops.yuv_frames_to_rgb8's bytes (the conversion included).
Medians of HIP-event times over --iters runs (at least 20) after --warmup.  One GPU shared with other work, clocks as the box sets them:
compare the columns of one run with each other, not with another run's.  "required" holds what DESIGN.md section 19 asks of a run.

    python tools/bench_yuv.py [--iters 30]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fgvc_amd import ops  # noqa: E402
from fgvc_amd.datasets import preprocess_yuv420_frames, yuv420_to_rgb8  # noqa: E402
from tests import yuv_cases as YC  # noqa: E402
from tools.bench_input import build, frames_u8, timed  # noqa: E402

HBM_TBPS = 8.0
YUV = dict(matrix="bt709", range="limited", siting="left")


def planes(T, h, w, dev, fmt, seed=0):
    """Packed frames of `fmt` on the device from bench_input's texture (Y its first channel, U and V the others at every second pixel) and
    their plane views."""
    t = frames_u8(T, h, w, torch.device("cpu"), seed)
    packed = YC.pack(t[..., 0].contiguous(), t[:, ::2, ::2, 1].contiguous(), t[:, ::2, ::2, 2].contiguous(), fmt).to(dev)
    return packed, ops.yuv420_planes(packed, fmt)


def kernels_vs_chains(dev, T, src, size, fmt, iters, warmup):
    packed, (y, u, v) = planes(T, src[0], src[1], dev, fmt)
    out = torch.empty((T, 3, size[0], size[1]), device=dev, dtype=torch.float32)
    out8 = torch.empty((T, src[0], src[1], 3), device=dev, dtype=torch.uint8)
    chain_ms = timed(lambda: preprocess_yuv420_frames(y, u, v, size, **YUV), iters, warmup)
    kernel_ms = timed(lambda: ops.yuv_frames_to_lab(y, u, v, size, out=out, **YUV), iters, warmup)
    chain8_ms = timed(lambda: yuv420_to_rgb8(y, u, v, **YUV), iters, warmup)
    kernel8_ms = timed(lambda: ops.yuv_frames_to_rgb8(y, u, v, out=out8, **YUV), iters, warmup)
    nbytes, nbytes8 = packed.numel() + out.numel() * 4, packed.numel() + out8.numel()
    r = {"format": fmt, "frames": T, "source": list(src), "size": list(size),
         "lab_chain_ms": round(chain_ms, 4), "lab_kernel_ms": round(kernel_ms, 4), "lab_chain_over_kernel": round(chain_ms / kernel_ms, 2),
         "lab_kernel_bytes": nbytes, "lab_kernel_tbps": round(nbytes / (kernel_ms * 1e-3) / 1e12, 3),
         "lab_share_of_hbm_8tbps": round(nbytes / (kernel_ms * 1e-3) / 1e12 / HBM_TBPS, 3),
         "rgb8_chain_ms": round(chain8_ms, 4), "rgb8_kernel_ms": round(kernel8_ms, 4), "rgb8_chain_over_kernel": round(chain8_ms / kernel8_ms, 2),
         "rgb8_kernel_bytes": nbytes8, "rgb8_kernel_tbps": round(nbytes8 / (kernel8_ms * 1e-3) / 1e12, 3)}
    host = tuple(p[:2].cpu().numpy() for p in (y, u, v))
    want = YC.preprocess_f64(*host, size, YUV["matrix"], YUV["range"], YUV["siting"])
    r["E_chain_vs_float64"] = float((preprocess_yuv420_frames(y[:2], u[:2], v[:2], size, **YUV)[0].cpu().double() - want).abs().max())
    r["E_kernel_vs_float64"] = float((out[:2].cpu().double() - want).abs().max())
    r["E_bytes_vs_float32_restatement"] = int((out8[:2].cpu().numpy() != YC.rgb8_f32(*host, YUV["matrix"], YUV["range"], YUV["siting"])).sum())
    r["E_bytes_vs_float64"] = int((out8[:2].cpu().numpy() != YC.rgb8_f64(*host, YUV["matrix"], YUV["range"], YUV["siting"])).sum())
    return r


def whole_call(dev, T, size, strides, P, iters, warmup):
    h, w = size
    packed, (y, u, v) = planes(T, h, w, dev, "i420", seed=1)
    g = torch.Generator().manual_seed(1)
    qp = torch.stack([torch.zeros(P), torch.rand(P, generator=g) * (w - 40) + 20, torch.rand(P, generator=g) * (h - 40) + 20], -1)[None].to(dev)
    kw = dict(query_points=qp, trajectories=torch.zeros(1, T, P, 2, device=dev), visibilities=torch.ones(1, T, P, device=dev))
    model = build(strides, dev, input=dict(type="i420", size=None, **YUV))
    rgb_model = build(strides, dev, input=dict(type="rgb8", size=None, layout="thwc"))
    floats = lambda: model(test_mode=True, rgbs=preprocess_yuv420_frames(y, u, v, size, **YUV), **kw)
    raw = lambda: model(test_mode=True, rgbs=packed[None], **kw)
    via_rgb = lambda: rgb_model(test_mode=True, rgbs=ops.yuv_frames_to_rgb8(y, u, v, **YUV)[None], **kw)
    with torch.no_grad():
        a1 = timed(floats, iters, warmup)
        b1 = timed(raw, iters, warmup)
        c1 = timed(via_rgb, iters, warmup)
        a2 = timed(floats, iters, warmup)                        # the same again, the other way round: the spread of the box
        b2 = timed(raw, iters, warmup)
        c2 = timed(via_rgb, iters, warmup)
        d = float((floats()[2] - raw()[2]).abs().max())
        d8 = float((via_rgb()[2] - raw()[2]).abs().max())
    return {"frames": T, "size": [h, w], "strides": list(strides), "points": P, "chain_plus_call_ms": [round(a1, 3), round(a2, 3)],
            "raw_i420_call_ms": [round(b1, 3), round(b2, 3)], "rgb8_bytes_plus_rgb8_call_ms": [round(c1, 3), round(c2, 3)],
            "chain_plus_call_over_raw_call": round(min(a1, a2) / min(b1, b2), 3), "rgb8_route_over_raw_call": round(min(c1, c2) / min(b1, b2), 3),
            "max_abs_traj_difference_px_vs_chain": d, "max_abs_traj_difference_px_vs_rgb8_route": d8}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    iters = max(20, a.iters)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_yuv.py times the GPU (fgvc_amd has no CPU path)")
    dev = torch.device("cuda:0")
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    rows = []
    for fmt in ("nv12", "i420"):
        rows.append(kernels_vs_chains(dev, 8, (480, 854), (480, 854), fmt, iters, a.warmup))
        out[f"same_size_8x480x854_{fmt}"] = rows[-1]
        rows.append(kernels_vs_chains(dev, 8, (1080, 1920), (480, 854), fmt, iters, a.warmup))
        out[f"resize_8x1080x1920_to_480x854_{fmt}"] = rows[-1]
    call = out["points_call_bench_480p_8f"] = whole_call(dev, 8, (480, 854), (1, 2, 1, 1), 16, iters, a.warmup)
    out["required"] = {"each_kernel_below_its_chain": all(r["lab_kernel_ms"] < r["lab_chain_ms"] and r["rgb8_kernel_ms"] < r["rgb8_chain_ms"] for r in rows),
                       "raw_call_not_slower_than_chain_plus_call": min(call["raw_i420_call_ms"]) <= min(call["chain_plus_call_ms"])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
