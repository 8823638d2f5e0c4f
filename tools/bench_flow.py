#!/usr/bin/env python3
"""Time dense optical flow (test_cfg.flow = dict(type='window', ...)) and print one JSON line.  8 frames of 480 x 854,
strides (1, 2, 1, 1), both trackers at their default window radius (VanillaTracker: neighbor_range 30 -> 15, HRVanillaTracker: 24 -> 12;
the latter built with stride=4, the encoder's output stride, so that its padded frame holds a feature cell on every 4th pixel).
Per tracker, medians of HIP-event times of
  * the affinity of the 14 pairs, both directions (engine.run_local_affinity on engine.flow_plan);
  * fgvc_flow_from_lists_f32, beside a plain torch chain with the same result (ops.topk_coord_rows, a subtraction, F.interpolate, a crop;
    renorm=False, which is what that chain computes) and the largest difference between the two;
  * fgvc_flow_consistency_f32, beside the reference's occlusion_estimation restated with F.grid_sample on the device, and how many pixels
    of the two results differ;
  * the whole forward_test_flow call (encoder included),
and the achieved bytes per second of the read-out against its own traffic (lists in, flow and validity out).

    python tools/bench_flow.py [--iters 20] [--warmup 5]
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

VANILLA = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, step=512, with_first=True, with_first_neighbor=True, batch_step=8)
HR = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=24, with_first=True, batch_step=8)


def build(typ, cfg, dev, **extra):
    unit = dict(stride=4) if typ == "HRVanillaTracker" else {}           # pad to the encoder's output stride: a feature cell every 4th pixel
    model = api.build_model(dict(type=typ, **unit, backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,), pool_type="none",
                                                         zero_init_residual=False)),
                            train_cfg=None, test_cfg=api.ConfigDict(**cfg, **extra))
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


def readout_chain(idx, weight, Hf, Wf, R, scale, size, pad):
    """The read-out in plain torch launches (renorm=False): get_coord's field, minus the cell's own coordinate, upsampled so that cell c sits
    on padded pixel c * scale, the last cell repeated beyond it, the pad cropped."""
    (h, w), (left, top) = size, pad
    rows = idx.shape[0]
    fields = ops.topk_coord_rows(idx, weight, Hf, Wf, R, scale).view(rows, Hf, Wf, 2)
    ys, xs = torch.meshgrid(torch.arange(Hf, device=idx.device), torch.arange(Wf, device=idx.device), indexing="ij")
    disp = (fields - torch.stack([xs, ys], -1).float() * scale).permute(0, 3, 1, 2)
    up = F.interpolate(disp, size=((Hf - 1) * scale + 1, (Wf - 1) * scale + 1), mode="bilinear", align_corners=True)
    up = F.pad(up, (0, scale - 1, 0, scale - 1), mode="replicate")
    return up[:, :, top:top + h, left:left + w].contiguous()


def _warp(feat, flow):
    """Warp() of the reference (align_corners=False, grid normalised by size - 1, zeros, the 0.9999 mask) in torch launches."""
    N, _, H, W = flow.shape
    ys, xs = torch.meshgrid(torch.arange(H, device=flow.device), torch.arange(W, device=flow.device), indexing="ij")
    grid = torch.stack([xs, ys], 0).float()[None] + flow
    gx, gy = grid[:, 0] * 2. / max(W - 1, 1) - 1., grid[:, 1] * 2. / max(H - 1, 1) - 1.
    g = torch.stack([gx, gy], -1)
    out = F.grid_sample(feat, g, mode="bilinear", padding_mode="zeros", align_corners=False)
    mask = F.grid_sample(torch.ones_like(feat), g, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out * (mask > 0.9999).float()


def consistency_chain(fw, bw, mode, diff):
    def one(a, b):
        wb = _warp(b, a)
        sq = ((a + wb) ** 2).sum(1, keepdim=True)
        if mode == "fb_abs":
            return (sq ** 0.5 < diff).to(a)
        return (sq < (a * 2 + wb ** 2).sum(1, keepdim=True) * 0.01 + 0.5).to(a)
    return one(fw, bw), one(bw, fw)


def run(dev, typ, cfg, T, size, iters, warmup):
    h, w = size
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    model = build(typ, cfg, dev, flow=dict(type="window", occlusion="consistency"))
    fc = model._flow()
    with torch.no_grad():
        call_ms = timed(lambda: model(test_mode=True, imgs=imgs), iters, warmup)
        frames, _, pad = model._label_frames(imgs)
        feats, Hf, Wf = model._label_feats(frames)
        rows, lc = model._window_rows(feats, Hf, Wf, fc.radius, "flow")
        scale, pad = frames.shape[-1] // Wf, (pad[0], pad[2])
        plan = engine.flow_plan(T, fc.step, Hf * Wf, lc)
        stats = {}
        aff_ms = timed(lambda: engine.run_local_affinity(rows, Hf, Wf, plan, lc, stats), iters, warmup)
        idx, _, weight = engine.run_local_affinity(rows, Hf, Wf, plan, lc)
        n = idx.shape[0]
        k_ms = timed(lambda: ops.flow_from_lists(idx, weight, Hf, Wf, fc.radius, scale, (h, w), pad, False), iters, warmup)
        c_ms = timed(lambda: readout_chain(idx, weight, Hf, Wf, fc.radius, scale, (h, w), pad), iters, warmup)
        d = float((ops.flow_from_lists(idx, weight, Hf, Wf, fc.radius, scale, (h, w), pad, False)[0]
                   - readout_chain(idx, weight, Hf, Wf, fc.radius, scale, (h, w), pad)).abs().max())
        flow, _ = ops.flow_from_lists(idx, weight, Hf, Wf, fc.radius, scale, (h, w), pad, True)
        fw, bw = flow[:n // 2], flow[n // 2:]
        occ_ms = timed(lambda: ops.flow_consistency(fw, bw, "consistency"), iters, warmup)
        occ_chain_ms = timed(lambda: consistency_chain(fw, bw, "consistency", 1.5), iters, warmup)
        a, b = ops.flow_consistency(fw, bw, "consistency"), consistency_chain(fw, bw, "consistency", 1.5)
        differ = int((a[0] != b[0]).sum() + (a[1] != b[1]).sum())
    traffic = idx.numel() * 8 + n * h * w * 9
    occ_traffic = fw.numel() * 4 * 2 + fw.shape[0] * h * w * 4 * 2
    return {"tracker": typ, "frames": T, "size": [h, w], "feature_grid": [Hf, Wf], "scale": scale, "window_radius": fc.radius, "topk": int(lc.topk),
            "rows": n, "route": stats.get("route"), "chunks": stats.get("chunks"),
            "call_ms": round(call_ms, 3), "affinity_ms": round(aff_ms, 3),
            "flow_from_lists_ms": round(k_ms, 4), "flow_from_lists_torch_chain_ms": round(c_ms, 4), "flow_from_lists_vs_chain_max_abs": d,
            "flow_from_lists_bytes": traffic, "flow_from_lists_GBps": round(traffic / (k_ms * 1e-3) / 1e9, 1),
            "flow_consistency_ms": round(occ_ms, 4), "flow_consistency_torch_chain_ms": round(occ_chain_ms, 4),
            "flow_consistency_pixels_differing_from_chain": differ, "flow_consistency_pixels": int(2 * a[0].numel()),
            "flow_consistency_bytes": occ_traffic, "flow_consistency_GBps": round(occ_traffic / (occ_ms * 1e-3) / 1e9, 1),
            "consistent_share": round(float(a[0].mean()), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_flow.py times kernels on the GPU (fgvc_amd has no CPU path)")
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0)}
    for name, typ, cfg in (("vanilla", "VanillaTracker", VANILLA), ("hr", "HRVanillaTracker", HR)):
        out[name] = run(dev, typ, cfg, a.frames, tuple(a.size), a.iters, a.warmup)
        print(f"# {name}: {json.dumps(out[name])}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
