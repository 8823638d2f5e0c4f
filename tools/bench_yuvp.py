#!/usr/bin/env python3
"""Time the input stage for Y'CbCr at 8 to 16 bits, 4:2:0 / 4:2:2 / 4:4:4 (fgvc_frames_yuvp_to_lab_f32, fgvc_frames_yuvp_to_rgb8,
test_cfg.input type = an ops.YUV_PIXEL_FORMATS name) and print one JSON line.

(a) per format (p010, yuv422p10, yuv444p10) and geometry (8 x 480 x 854 at the same size; 8 x 1080 x 1920 -> 480 x 854), on planes already on
    the device: the Lab kernel against datasets.preprocess_yuv_frames (the torch chain on the same GPU) and against
    fgvc_frames_yuv420_to_lab_f32 on an 8-bit I420 clip of the same geometry in the same process; the bytes kernel against
    datasets.yuv_to_rgb8 and against fgvc_frames_yuv420_to_rgb8; each kernel's bytes (planes read once + output written once) over its time;
    E_chain / E_kernel against the float64 restatement (tests/yuvp_cases.py, first two frames) and the bytes that differ from the float32
    restatement (the contract: 0).
(b) one whole points call at bench.py's geometry (8 frames of 480 x 854, strides (1, 2, 1, 1), 16 points) on packed P010 frames with
    test_cfg.input = dict(type='p010'), against the torch chain followed by the call on its float frames.
Medians of HIP-event times over --iters runs (at least 20) after --warmup; everything is measured twice ("run1", "run2") one after the other:
the spread of the box.  One GPU shared with other work, clocks as the box sets them: compare the columns of one run with each other.

    python tools/bench_yuvp.py [--iters 30]
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
from fgvc_amd.datasets import preprocess_yuv_frames, yuv_to_rgb8  # noqa: E402
from tests import yuv_cases as YC  # noqa: E402
from tests import yuvp_cases as PC  # noqa: E402
from tools.bench_input import build, frames_u8, timed  # noqa: E402

YUV = dict(matrix="bt709", range="limited", siting="left")
FORMATS = ("p010", "yuv422p10", "yuv444p10")


def clip(T, h, w, dev, fmt, seed=0):
    """Packed frames of `fmt` on the device from bench_input's texture -- Y its first channel, U and V the others at the format's
    subsampling, scaled to the depth with noise in the new low bits and in the unused bits of the word --, their plane views, the format's
    arguments and the planes on the host."""
    _, sx, sy, depth, _, _ = PC.FORMATS[fmt]
    t = frames_u8(T, h, w, torch.device("cpu"), seed).numpy().astype(np.int64)
    rs = np.random.RandomState(seed)
    s = 1 << (depth - 8)
    planes = tuple(PC.words(p * s + rs.randint(0, s, size=p.shape), fmt, rs) for p in (t[..., 0], t[:, ::sy, ::sx, 1], t[:, ::sy, ::sx, 2]))
    packed = PC.pack(*planes, fmt).to(dev)
    return packed, ops.yuv_planes(packed, fmt), PC.fmt_args(fmt), planes


def clip8(T, h, w, dev, seed=0):
    t = frames_u8(T, h, w, torch.device("cpu"), seed)
    packed = YC.pack(t[..., 0].contiguous(), t[:, ::2, ::2, 1].contiguous(), t[:, ::2, ::2, 2].contiguous(), "i420").to(dev)
    return packed, ops.yuv420_planes(packed, "i420")


def kernels(dev, T, src, size, fmt, iters, warmup):
    packed, (y, u, v), fa, planes = clip(T, src[0], src[1], dev, fmt)
    packed8, (y8, u8, v8) = clip8(T, src[0], src[1], dev)
    kw = dict(YUV) if fa["subsampling"][0] == 2 else {k: YUV[k] for k in ("matrix", "range")}
    out = torch.empty((T, 3, size[0], size[1]), device=dev, dtype=torch.float32)
    out8 = torch.empty((T, src[0], src[1], 3), device=dev, dtype=torch.uint8)
    runs = []
    for _ in range(2):
        runs.append(dict(
            lab_chain_ms=timed(lambda: preprocess_yuv_frames(y, u, v, size=size, **fa, **kw), iters, warmup),
            lab_kernel_ms=timed(lambda: ops.yuv_planes_to_lab(y, u, v, size=size, out=out, **fa, **kw), iters, warmup),
            lab_kernel_8bit_420_ms=timed(lambda: ops.yuv_frames_to_lab(y8, u8, v8, size, out=out, **YUV), iters, warmup),
            rgb8_chain_ms=timed(lambda: yuv_to_rgb8(y, u, v, **fa, **kw), iters, warmup),
            rgb8_kernel_ms=timed(lambda: ops.yuv_planes_to_rgb8(y, u, v, out=out8, **fa, **kw), iters, warmup),
            rgb8_kernel_8bit_420_ms=timed(lambda: ops.yuv_frames_to_rgb8(y8, u8, v8, out=out8, **YUV), iters, warmup)))
    ops.yuv_planes_to_lab(y, u, v, size=size, out=out, **fa, **kw)
    ops.yuv_planes_to_rgb8(y, u, v, out=out8, **fa, **kw)
    best = {k: min(r[k] for r in runs) for k in runs[0]}
    nbytes = packed.numel() * packed.element_size() + out.numel() * 4
    r = {"format": fmt, "frames": T, "source": list(src), "size": list(size), "run1": {k: round(x, 4) for k, x in runs[0].items()},
         "run2": {k: round(x, 4) for k, x in runs[1].items()}, "input_bytes": packed.numel() * packed.element_size(),
         "input_bytes_8bit_420": packed8.numel(), "lab_chain_over_kernel": round(best["lab_chain_ms"] / best["lab_kernel_ms"], 2),
         "lab_kernel_over_8bit_420_kernel": round(best["lab_kernel_ms"] / best["lab_kernel_8bit_420_ms"], 3),
         "rgb8_chain_over_kernel": round(best["rgb8_chain_ms"] / best["rgb8_kernel_ms"], 2),
         "rgb8_kernel_over_8bit_420_kernel": round(best["rgb8_kernel_ms"] / best["rgb8_kernel_8bit_420_ms"], 3),
         "lab_kernel_bytes": nbytes, "lab_kernel_tbps": round(nbytes / (best["lab_kernel_ms"] * 1e-3) / 1e12, 3)}
    host = tuple(p[:2] for p in planes)
    sit = kw.get("siting", "left")
    want = PC.preprocess_f64(*host, fmt, size, YUV["matrix"], YUV["range"], sit)
    chain = preprocess_yuv_frames(y[:2], u[:2], v[:2], size=size, **fa, **kw)[0]
    r["E_chain_vs_float64"] = float((chain.cpu().double() - want).abs().max())
    r["E_kernel_vs_float64"] = float((out[:2].cpu().double() - want).abs().max())
    r["E_bytes_vs_float32_restatement"] = int((out8[:2].cpu().numpy() != PC.rgb8_f32(*host, fmt, YUV["matrix"], YUV["range"], sit)).sum())
    return r


def whole_call(dev, T, size, strides, P, iters, warmup):
    h, w = size
    packed, (y, u, v), fa, _ = clip(T, h, w, dev, "p010", seed=1)
    g = torch.Generator().manual_seed(1)
    qp = torch.stack([torch.zeros(P), torch.rand(P, generator=g) * (w - 40) + 20, torch.rand(P, generator=g) * (h - 40) + 20], -1)[None].to(dev)
    kw = dict(query_points=qp, trajectories=torch.zeros(1, T, P, 2, device=dev), visibilities=torch.ones(1, T, P, device=dev))
    model = build(strides, dev, input=dict(type="p010", size=None, **YUV))
    floats = lambda: model(test_mode=True, rgbs=preprocess_yuv_frames(y, u, v, size=size, **fa, **YUV), **kw)     # noqa: E731
    raw = lambda: model(test_mode=True, rgbs=packed[None], **kw)                                                    # noqa: E731
    with torch.no_grad():
        a1 = timed(floats, iters, warmup)
        b1 = timed(raw, iters, warmup)
        a2 = timed(floats, iters, warmup)
        b2 = timed(raw, iters, warmup)
        d = float((floats()[2] - raw()[2]).abs().max())
    return {"frames": T, "size": [h, w], "strides": list(strides), "points": P, "chain_plus_call_ms": [round(a1, 3), round(a2, 3)],
            "raw_p010_call_ms": [round(b1, 3), round(b2, 3)], "chain_plus_call_over_raw_call": round(min(a1, a2) / min(b1, b2), 3),
            "max_abs_traj_difference_px_vs_chain": d}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    iters = max(20, a.iters)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_yuvp.py times the GPU (fgvc_amd has no CPU path)")
    dev = torch.device("cuda:0")
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for fmt in FORMATS:
        out[f"same_size_8x480x854_{fmt}"] = kernels(dev, 8, (480, 854), (480, 854), fmt, iters, a.warmup)
        out[f"resize_8x1080x1920_to_480x854_{fmt}"] = kernels(dev, 8, (1080, 1920), (480, 854), fmt, iters, a.warmup)
    out["points_call_bench_480p_8f"] = whole_call(dev, 8, (480, 854), (1, 2, 1, 1), 16, iters, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
