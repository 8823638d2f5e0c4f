#!/usr/bin/env python3
"""Time the soft-map path (VanillaTracker.forward_test with soft first-frame labels and return_maps=True) and print one JSON line.  The
geometries of tools/bench_heatmap.py: JHMDB (40 frames of 320 x 320, K = 15 joints, maps at the video's 240 x 320) and 8 frames of
480 x 854 with K = 16.  Per geometry: ms per clip with the encoder / labels / affinity / propagation / read-out / copy-to-host phases
split out by HIP events (the copy: the whole stack into an existing, touched pageable host array, as engine.softmaps_to_host copies its
chunks; softmaps_to_host_wall_ms is that function's wall time, allocation of the host array included), and the read-out kernel alone on a random bank, both
output dtypes: us per clip, the bytes it writes and bytes/s.

    python tools/bench_softmap.py [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import engine, ops  # noqa: E402


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
    split = {k: [] for k in ("encoder",) + names[:-1] + ("copy_to_host", "total")}
    host = None
    with torch.no_grad():
        for it in range(warmup + iters):
            ev = {k: torch.cuda.Event(enable_timing=True) for k in ("start",) + names}
            ev["start"].record()
            feats, Hf, Wf = model.get_feats_hwc(frames, split=True)
            bank, _ = engine.propagate_soft_bank(feats, Hf, Wf, heat, map_pad, cfg, channels=model.feat_channels, events=ev)
            ev["readout"].record()
            maps = ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape)
            ev["end"].record()
            # the copy as softmaps_to_host makes it (a synchronous copy into pageable host memory), between HIP events, into a host array
            # that exists and has been touched: neither its allocation nor its first-touch page faults are in the figure
            if host is None:
                host = torch.zeros(maps.shape, dtype=maps.dtype)
            c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            c0.record()
            host.copy_(maps)
            c1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                seq = ("start",) + names
                for k0, k1, name in zip(seq[:-1], seq[1:], ("encoder",) + names[:-1]):
                    split[name].append(ev[k0].elapsed_time(ev[k1]))
                split["copy_to_host"].append(c0.elapsed_time(c1))
                split["total"].append(ev["start"].elapsed_time(ev["end"]) + split["copy_to_host"][-1])
        t0 = time.perf_counter()
        result = engine.softmaps_to_host(bank, heat, Hf, Wf, map_pad, out_shape)      # what the model call runs: allocation + read-out + copies
        to_host_ms = (time.perf_counter() - t0) * 1e3
        host = result
        del maps
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
            return e0.elapsed_time(e1) / iters * 1000.0              # us per call

        kernel = {}
        for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
            out = torch.empty((T, K, *out_shape), device=dev, dtype=dt)
            us = timeit(lambda: ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape, out=out))
            us0 = timeit(lambda: ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape, frames=(0, 1), out=out[:1]))
            us1 = timeit(lambda: ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape, frames=(1, T), out=out[1:]))
            kernel[name] = {"us_per_clip": round(us, 2), "frame0_us": round(us0, 2), "later_frames_us": round(us1, 2),
                            "later_frames_written_TB_per_s": round(out[1:].numel() * out.element_size() / us1 / 1e6, 3),
                            "bytes_written": out.numel() * out.element_size(),
                            "bytes_read_bank": bank.numel() * 4, "written_TB_per_s": round(out.numel() * out.element_size() / us / 1e6, 3)}
            del out
    med = lambda v: sorted(v)[len(v) // 2]
    return {"frames": T, "size": [h, w], "maps": K, "out_shape": list(out_shape), "feature_grid": [Hf, Wf], "map_dtype": "float64",
            "pair_split_fmt": cfg.pair_split_fmt, "result_bytes": int(host.nbytes), "softmaps_to_host_wall_ms": round(to_host_ms, 3),
            "ms_per_clip": round(med(split["total"]), 3), "split_ms": {k: round(med(v), 3) for k, v in split.items() if k != "total"},
            "readout_kernel": kernel, "maps_last_frame_map0_max": float(host[-1, 0].max())}


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
                                          with_first_neighbor=True, return_maps=True))
    model.init_weights()
    model = model.to(dev).eval()
    out = {"jhmdb": run(model, dev, 40, (320, 320), 15, (240, 320), a.iters, a.warmup),
           "davis_480p": run(model, dev, 8, (480, 854), 16, (480, 854), a.iters, a.warmup)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
