#!/usr/bin/env python3
"""Time the segmentation-mask path (VanillaTracker.forward_test_seg's GPU work) on an 8-frame 480 x 854 clip with 3 objects and print
one JSON line: ms per clip with the encoder / affinity (pair top-k + merge) / propagation / read-out split out by HIP events, and the
read-out kernel's us per frame beside the torch chain it replaces (F.interpolate x 2, min-max normalisation, argmax) on the same labels,
with the bytes each moves (the kernel's: labels read by its two passes + masks written; the chain's: every tensor it materialises
written once and read once, the (C, hp, wp) f32 maps among them).

    python tools/bench_seg.py [--frames 8 --size 480 854 --objects 3 --iters 20]
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


def torch_chain(soft, Hf, Wf, pad_shape, pad, out_shape):
    n, _, C = soft.shape
    x = soft.reshape(n, Hf, Wf, C).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=pad_shape, mode="bilinear", align_corners=False)
    lw, uw, lh, uh = pad
    x = x[:, :, lh:pad_shape[0] - uh, lw:pad_shape[1] - uw]
    x = F.interpolate(x, size=out_shape, mode="bilinear", align_corners=False)
    mn = x.flatten(2).min(-1)[0][..., None, None]
    mx = x.flatten(2).max(-1)[0][..., None, None]
    x = torch.where(mx > 0, (x - mn) / (mx - mn + 1e-12), x)
    return x.argmax(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, (h, w) = a.frames, a.size
    torch.manual_seed(0)
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")),
                            test_cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, with_first=True,
                                          with_first_neighbor=True))
    model.init_weights()
    model = model.to(dev).eval()
    cfg = model.engine_config()
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    seg = torch.zeros(h, w, dtype=torch.uint8)
    for k in range(a.objects):
        y0, x0 = 60 + 100 * k, 100 + 220 * k
        seg[y0:y0 + 120, x0:x0 + 160] = k + 1
    d = model.output_stride()
    (hp, wp), pad = engine.pad_divide_by(h, w, d)
    seg = F.pad(seg.to(dev), pad).contiguous()
    frames = F.pad(imgs[0, 0], pad).transpose(0, 1).contiguous()
    names = ("labels", "affinity", "propagation", "readout", "end")
    split = {k: [] for k in ("encoder", "labels", "affinity", "propagation", "readout", "total")}
    with torch.no_grad():
        for it in range(a.warmup + a.iters):
            ev = {k: torch.cuda.Event(enable_timing=True) for k in ("start",) + names}
            ev["start"].record()
            feats, Hf, Wf = model.get_feats_hwc(frames, split=True)
            masks = engine.propagate_masks(feats, Hf, Wf, seg, pad, (h, w), cfg, channels=model.feat_channels, events=ev)
            torch.cuda.synchronize()
            if it >= a.warmup:
                seq = ("start",) + names
                for k0, k1, name in zip(seq[:-1], seq[1:], ("encoder", "labels", "affinity", "propagation", "readout")):
                    split[name].append(ev[k0].elapsed_time(ev[k1]))
                split["total"].append(ev["start"].elapsed_time(ev["end"]))
        # the read-out alone against the torch chain, on the same soft labels
        C = int(ops.seg_max_label(seg, Hf, Wf).item()) + 1
        soft = torch.rand(T - 1, Hf * Wf, C, device=dev, generator=torch.Generator(device=dev).manual_seed(2)) ** 3
        out = torch.empty((T - 1, h, w), device=dev, dtype=torch.uint8)

        def timeit(fn, n=a.iters):
            for _ in range(3):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / n * 1000.0 / (T - 1)          # us per frame

        k_us = timeit(lambda: ops.seg_readout(soft, Hf, Wf, (hp, wp), pad, (h, w), True, out=out))
        t_us = timeit(lambda: torch_chain(soft, Hf, Wf, (hp, wp), pad, (h, w)))
        same = int((out.long() != torch_chain(soft, Hf, Wf, (hp, wp), pad, (h, w))).sum())
    med = lambda v: sorted(v)[len(v) // 2]
    lab_bytes = Hf * Wf * C * 4
    k_bytes = 2 * lab_bytes + h * w                                       # two passes over the labels (L2-resident) + the mask
    full_p, full_o = C * hp * wp * 4, C * h * w * 4
    t_bytes = lab_bytes + 2 * full_p + 2 * full_o + 2 * full_o + 2 * full_o + h * w * 8   # interp, interp, min/max read, where, argmax
    print(json.dumps({"config": {"frames": T, "size": [h, w], "objects": a.objects, "classes": C, "feature_grid": [Hf, Wf], "stride": d,
                                 "pair_split_fmt": cfg.pair_split_fmt, "iters": a.iters},
                      "ms_per_clip": round(med(split["total"]), 3),
                      "split_ms": {k: round(med(v), 3) for k, v in split.items() if k != "total"},
                      "readout_us_per_frame": {"kernel": round(k_us, 2), "torch_chain": round(t_us, 2)},
                      "readout_bytes_per_frame": {"kernel": k_bytes, "torch_chain": t_bytes},
                      "readout_pixels_differing_from_f32_torch_chain": same,
                      "masks_frame_last_ids": sorted(torch.unique(masks[-1]).tolist())}))


if __name__ == "__main__":
    main()
