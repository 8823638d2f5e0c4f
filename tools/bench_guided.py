#!/usr/bin/env python3
"""Time the edge-aware read-out (test_cfg.readout = dict(type='guided')) on an 8-frame 480 x 854 clip with 3 objects
and print one JSON line, every figure a median of HIP-event times:

  readout_us                  ops.seg_readout (fgvc_seg_readout_u8) on the bank of T - 1 frames: the plain read-out, the yardstick;
  guide_cells_us              ops.guide_cells on the T - 1 padded frames (the guided read-out's own pre-pass when no cells are handed in);
  guided_us / guided_conf_us  ops.seg_readout_guided and its conf=True form with the cells handed in (extremes pre-pass + the one launch);
  guided_total_us             the same without cells: guide_cells + the read-out, what the mask call pays;
  mask_call_ms / mask_call_guided_ms    the model's whole mask call without and with the key;
  readout_parent_us ...       fgvc_seg_readout_u8 of --parent-lib (the library built from the parent commit) measured twice beside this
                              build's in the same run; the spread of the two parent figures is the noise the difference is held against.

    python tools/bench_guided.py [--frames 8 --size 480 854 --objects 3 --iters 20 --radius 2] [--parent-lib PATH/libfgvc_hip.so]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import _lib, engine, ops  # noqa: E402


def timed(fn, iters, warmup):
    """Median milliseconds of fn() by HIP events, one pair per call."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def readout_with(lib, soft, Hf, Wf, pad_shape, pad, out_shape, out, ws):
    n, C = soft.shape[0], soft.shape[2]
    (hp, wp), (lw, uw, lh, uh), (h0, w0) = pad_shape, pad, out_shape
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.fgvc_seg_readout_u8(ctypes.c_void_p(soft.data_ptr()), n, Hf, Wf, C, hp, wp, lh, lw, hp - lh - uh, wp - lw - uw, h0, w0, 1,
                                 ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), stream)
    assert rc == 0, rc


def build(dev, **extra):
    torch.manual_seed(0)
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")),
                            test_cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, with_first=True,
                                          with_first_neighbor=True, masks="device", **extra))
    model.init_weights()
    return model.to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libfgvc_hip.so built from the parent commit: its fgvc_seg_readout_u8 is timed beside this build's")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, (h, w) = a.frames, a.size
    readout = dict(type="guided", radius=a.radius, sigma_space=1.0, sigma_range=0.1)
    plain, guided = build(dev), build(dev, readout=readout)
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    seg = torch.zeros(h, w, dtype=torch.uint8)
    for k in range(a.objects):
        y0, x0 = 60 + 100 * k, 100 + 220 * k
        seg[y0:y0 + 120, x0:x0 + 160] = k + 1
    meta = [dict(original_shape=(h, w))]
    ref = seg[None].to(dev)
    res = dict(frames=T, size=[h, w], objects=a.objects, iters=a.iters, radius=a.radius)

    with torch.no_grad():
        res["mask_call_ms"] = timed(lambda: plain(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta), a.iters, a.warmup)
        res["mask_call_guided_ms"] = timed(lambda: guided(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta), a.iters, a.warmup)
        # the read-outs on one bank: the soft rows of the clip above
        cfg = guided._label_config()
        frames, _, pad = guided._label_frames(imgs)
        feats, Hf, Wf = guided._label_feats(frames, index_map=True)
        hp, wp = frames.shape[-2:]
        C = a.objects + 1
        bank = torch.zeros((T, Hf * Wf, C), device=dev)
        ops.seg_onehot_labels(torch.nn.functional.pad(seg.to(dev), pad).contiguous(), Hf, Wf, C, out=bank[0])
        engine._sweep_labels(bank, bank, engine.label_affinity(feats, Hf, Wf, T, cfg, guided.feat_channels), Hf, Wf)
        soft, guide = bank[1:].contiguous(), frames.float().contiguous()[1:]
    res.update(grid=[Hf, Wf], padded=[hp, wp], channels=C)
    args = (soft, Hf, Wf, (hp, wp), pad, (h, w))
    gargs = (soft, guide, Hf, Wf, (hp, wp), pad, (h, w), True, a.radius, 1.0, 0.1)
    out = torch.empty((T - 1, h, w), device=dev, dtype=torch.uint8)
    conf = torch.empty_like(out)
    cells = ops.guide_cells(guide, Hf, Wf)
    res["readout_us"] = 1e3 * timed(lambda: ops.seg_readout(*args, True, out=out), a.iters, a.warmup)
    res["guide_cells_us"] = 1e3 * timed(lambda: ops.guide_cells(guide, Hf, Wf, out=cells), a.iters, a.warmup)
    res["guided_us"] = 1e3 * timed(lambda: ops.seg_readout_guided(*gargs, out=out, cells=cells), a.iters, a.warmup)
    res["guided_conf_us"] = 1e3 * timed(lambda: ops.seg_readout_guided(*gargs, conf=True, out=(out, conf), cells=cells), a.iters, a.warmup)
    res["guided_total_us"] = 1e3 * timed(lambda: ops.seg_readout_guided(*gargs, out=out), a.iters, a.warmup)
    res["changed_pixel_share"] = float((ops.seg_readout_guided(*gargs) != ops.seg_readout(*args, True)).float().mean())
    if a.parent_lib:
        this, parent = _lib.load(), ctypes.CDLL(a.parent_lib)
        ws = torch.empty((this.fgvc_seg_readout_workspace_bytes(T - 1, C) + 3) // 4, device=dev)
        want = ops.seg_readout(*args, True)
        for name, lib in (("readout_parent_us", parent), ("readout_this_us", this), ("readout_parent_again_us", parent)):
            res[name] = 1e3 * timed(lambda: readout_with(lib, *args, out, ws), a.iters, a.warmup)
            assert torch.equal(out, want), name                   # the same bytes from either build
        res["readout_parent_spread_us"] = abs(res["readout_parent_us"] - res["readout_parent_again_us"])
    print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
