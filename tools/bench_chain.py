#!/usr/bin/env python3
"""Time the flow-chaining point tracker (test_cfg.chain = dict(type='flow', ...)) and print one JSON line.  One clip of
8 frames of 480 x 854, strides (1, 2, 1, 1), at P = 256 random queries and at the dense grid engine.grid_queries(0, 480, 854, 4).  Medians
of HIP-event times of
  * fgvc_flow_chain_f32 alone, on the flows the tracker's own flow call produced;
  * the same chain issued as torch launches on the device (the rule restated with torch ops, every point at once, frame by frame), and how
    many entries of the two results differ;
  * the whole chained points call (encoder and flow included) of both trackers, next to the whole label-propagation points call on the
    same frames and queries (P = 256 only: the label path holds a (T, cells, P) label bank, 21 GB at the dense grid).

    python tools/bench_chain.py [--iters 20] [--warmup 5]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

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


def sample_torch(field, x, y):
    """bilinear_sample2d of field (2, h, w) at x, y (P,) in torch launches, the reference's order."""
    h, w = field.shape[-2:]
    x0f, y0f = x.floor(), y.floor()
    x1f, y1f = x0f + 1, y0f + 1
    x0, y0 = x0f.long(), y0f.long()
    xa, xb, ya, yb = x0.clamp(0, w - 1), (x0 + 1).clamp(0, w - 1), y0.clamp(0, h - 1), (y0 + 1).clamp(0, h - 1)
    flat = field.reshape(2, -1)
    i00, i01, i10, i11 = flat[:, ya * w + xa], flat[:, ya * w + xb], flat[:, yb * w + xa], flat[:, yb * w + xb]
    w00, w01, w10, w11 = (x1f - x) * (y1f - y), (x - x0f) * (y1f - y), (x1f - x) * (y - y0f), (x - x0f) * (y - y0f)
    return ((w00 * i00 + w01 * i01) + w10 * i10) + w11 * i11


def chain_torch(fw, bw, query):
    """RAFT.forward_test's chain (raft.py:247-289) on the device in torch launches: traj (T, P, 2), vis (T, P).  Positions stay finite and
    far from 2^23 on the bench's flows, so the fail-closed rule has nothing to do."""
    n, _, h, w = fw.shape
    tq, qxy = query[:, 0], query[:, 1:].t().contiguous()
    cur, coords = torch.zeros_like(qxy), []
    for t in range(n + 1):
        if t:
            cur = cur + sample_torch(fw[t - 1], cur[0], cur[1])
        cur = torch.where(tq == t, qxy, cur)
        coords.append(cur)
    for t in range(n - 1, -1, -1):
        nxt = coords[t + 1]
        coords[t] = torch.where(tq > t, nxt + sample_torch(bw[t], nxt[0], nxt[1]), coords[t])
    traj = torch.stack(coords).transpose(1, 2).contiguous()
    vis = (traj[..., 0] >= 0) & (traj[..., 1] >= 0) & (traj[..., 0] < w) & (traj[..., 1] < h)
    return traj, vis.to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_chain.py times kernels on the GPU (fgvc_amd has no CPU path)")
    dev = torch.device("cuda:0")
    T, (h, w) = a.frames, a.size
    g = torch.Generator().manual_seed(1)
    rgbs = torch.randn(1, T, 3, h, w, generator=g).clamp(-1, 1).to(dev)
    sparse = torch.stack([torch.randint(0, T, (256,), generator=g).float(), torch.rand(256, generator=g) * (w - 1),
                          torch.rand(256, generator=g) * (h - 1)], -1)
    sets = (("p256", sparse.to(dev)), ("grid4", engine.grid_queries(0, h, w, 4).to(dev)))
    out = {"device": torch.cuda.get_device_name(0), "frames": T, "size": [h, w]}
    with torch.no_grad():
        for name, typ, cfg in (("vanilla", "VanillaTracker", VANILLA), ("hr", "HRVanillaTracker", HR)):
            model = build(typ, cfg, dev, chain=dict(type="flow"))
            labels = build(typ, cfg, dev)
            r = {}
            for key, q in sets:
                P = q.shape[0]
                tr, vi = torch.zeros(1, T, P, 2, device=dev), torch.zeros(1, T, P, device=dev)
                call = lambda m: m(test_mode=True, rgbs=rgbs, query_points=q[None], trajectories=tr, visibilities=vi)
                r[key] = {"P": P, "chain_call_ms": round(timed(lambda: call(model), a.iters, a.warmup), 3)}
                if key == "p256":
                    r[key]["label_propagation_call_ms"] = round(timed(lambda: call(labels), a.iters, a.warmup), 3)
                if name == "vanilla":
                    fw, bw = model.last_flow["flow_fw"], model.last_flow["flow_bw"]
                    k_ms = timed(lambda: ops.flow_chain(fw, bw, q), a.iters, a.warmup)
                    t_ms = timed(lambda: chain_torch(fw, bw, q), a.iters, a.warmup)
                    (kt, kv), (tt, tv) = ops.flow_chain(fw, bw, q), chain_torch(fw, bw, q)
                    r[key].update(flow_chain_ms=round(k_ms, 4), torch_chain_ms=round(t_ms, 4),
                                  entries_differing_from_torch_chain=int((kt.view(torch.int32) != tt.view(torch.int32)).sum() + (kv != tv).sum()),
                                  visible_share=round(float(kv.float().mean()), 3))
            out[name] = r
            print(f"# {name}: {json.dumps(r)}", file=sys.stderr, flush=True)
            del model, labels
    print(json.dumps(out))


if __name__ == "__main__":
    main()
