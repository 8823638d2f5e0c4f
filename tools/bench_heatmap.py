#!/usr/bin/env python3
"""Time the heat-map path (VanillaTracker.forward_test with soft first-frame labels and coords=True) and print one JSON line.  Two
geometries: JHMDB (40 frames of 320 x 320, K = 15 joints, coordinates at the video's 240 x 320) and 8 frames of 480 x 854 with K = 16.
Per geometry: ms per clip with the encoder / labels / affinity (pair top-k + merge) / propagation / read-out split out by HIP events,
and the coordinate read-out's us per frame beside a GPU torch chain on the same labels (frame >= 1: F.interpolate to the padded size,
unpad, F.interpolate to the output size, topk(5), the top-5 normalisation, the coordinates), with the bytes each moves (the kernel's: the
bank rows it reads and the coordinates; the chain's: every tensor it materialises written once and read once).

    python tools/bench_heatmap.py [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import engine, ops  # noqa: E402


def torch_chain(bank, Hf, Wf, map_pad, hw_map, out_shape):
    """img2coord of frames 1.. materialised with torch (f32), as the reference computes them (:770-784, :172-191) but on the GPU."""
    n, _, K = bank.shape
    hm, wm = hw_map
    lw, uw, lh, uh = map_pad
    hp, wp = hm + lh + uh, wm + lw + uw
    x = bank.reshape(n, Hf, Wf, K).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=(hp, wp), mode="bilinear", align_corners=False)[:, :, lh:hp - uh, lw:wp - uw]
    x = F.interpolate(x, size=out_shape, mode="bilinear", align_corners=False)
    flat = x.flatten(2)
    v, i = flat.topk(5, dim=-1)
    v = v / (v.sum(-1, keepdim=True) + 1e-9)
    w0 = out_shape[1]
    xy = torch.stack([((i % w0).double() * v.double()).sum(-1), ((i // w0).double() * v.double()).sum(-1)])
    return torch.where((flat.sum(-1) == 0)[None], torch.full_like(xy, -1.0), xy)


def run(model, dev, T, size, K, out_shape, iters, warmup):
    cfg = model.engine_config()
    h, w = size
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    cy, cx = torch.rand(K, generator=g, dtype=torch.float64) * h, torch.rand(K, generator=g, dtype=torch.float64) * w
    heat = torch.exp(-((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2) / 32.0).to(dev)   # sigma 4, f64
    d = model.output_stride()
    _, pad = engine.pad_divide_by(h, w, d)
    _, map_pad = engine.pad_divide_by(h, w, d)
    frames = F.pad(imgs[0, 0], pad).transpose(0, 1).contiguous()
    names = ("labels", "affinity", "propagation", "readout", "end")
    split = {k: [] for k in ("encoder",) + names[:-1] + ("total",)}
    with torch.no_grad():
        for it in range(warmup + iters):
            ev = {k: torch.cuda.Event(enable_timing=True) for k in ("start",) + names}
            ev["start"].record()
            feats, Hf, Wf = model.get_feats_hwc(frames, split=True)
            coords = engine.propagate_heatmaps(feats, Hf, Wf, heat, map_pad, out_shape, cfg, channels=model.feat_channels, events=ev)
            torch.cuda.synchronize()
            if it >= warmup:
                seq = ("start",) + names
                for k0, k1, name in zip(seq[:-1], seq[1:], ("encoder",) + names[:-1]):
                    split[name].append(ev[k0].elapsed_time(ev[k1]))
                split["total"].append(ev["start"].elapsed_time(ev["end"]))
        bank = torch.rand(T, Hf * Wf, K, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) ** 8

        def timeit(fn):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / iters * 1000.0 / T          # us per frame

        k_us = timeit(lambda: ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape))
        t_us = timeit(lambda: torch_chain(bank[1:], Hf, Wf, map_pad, (h, w), out_shape))
        diff = (ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape, f64_arith=False)[:, :, 1:]
                - torch_chain(bank[1:], Hf, Wf, map_pad, (h, w), out_shape).transpose(1, 2)).abs().max().item()
    med = lambda v: sorted(v)[len(v) // 2]
    h0, w0 = out_shape
    lab = Hf * Wf * K * 4
    k_bytes = lab + 2 * K * 8                                                    # one bank row read per frame, (2, K) coordinates written
    hp, wp = h + map_pad[2] + map_pad[3], w + map_pad[0] + map_pad[1]
    t_bytes = lab + 2 * K * hp * wp * 4 + 2 * K * h0 * w0 * 4 + K * h0 * w0 * 4 + K * 5 * 12   # interp, interp, topk read, lists
    return {"frames": T, "size": [h, w], "joints": K, "out_shape": [h0, w0], "feature_grid": [Hf, Wf], "pair_split_fmt": cfg.pair_split_fmt,
            "ms_per_clip": round(med(split["total"]), 3), "split_ms": {k: round(med(v), 3) for k, v in split.items() if k != "total"},
            "readout_us_per_frame": {"kernel": round(k_us, 2), "torch_chain": round(t_us, 2)},
            "readout_bytes_per_frame": {"kernel": k_bytes, "torch_chain": t_bytes},
            "readout_max_px_vs_f32_torch_chain": diff, "coords_frame_last_joint0": coords[:, 0, -1].tolist()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")),
                            test_cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, with_first=True,
                                          with_first_neighbor=True, coords=True))
    model.init_weights()
    model = model.to(dev).eval()
    out = {"jhmdb": run(model, dev, 40, (320, 320), 15, (240, 320), a.iters, a.warmup),
           "davis_480p": run(model, dev, 8, (480, 854), 16, (480, 854), a.iters, a.warmup)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
