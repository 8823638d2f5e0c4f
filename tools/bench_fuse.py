#!/usr/bin/env python3
"""Time the fused forward / backward label sweeps (test_cfg.refs fuse='linear') on an 8-frame 480 x 854 clip with
3 objects and complete maps at frames {0, 3, 6}, and print one JSON line.  Every figure is measured --runs times (default 2), one after
the other in this process, and reported as a list: the spread of a list is the noise a difference is held against.

  plain_second_ms       a session's second propagate with direction='both', override='all' and no fuse: the forward sweep, two injections
                        and the read-out.  This path issues the parent commit's launches in its order;
  fused_second_ms       the same call with fuse='linear': the forward sweep, the backward sweep from the last map, ONE fuse launch, the
                        same read-out, and the host read of the disagreement counts;
  fuse_launch_us        ops.seg_fuse_rows alone on stacks of the clip's size (the four frames between the maps), its argument checks and
                        the copy of the item records included;
  fuse_kernel_us        the C entry alone on ready item records, 20 launches back to back, per launch (fuse_bytes: what one moves);
  readout_rows_us / readout_fused_us    ops.seg_readout on the forward pass's rows before and after the fuse launch wrote over them;
  readout_parent_us     fgvc_seg_readout_u8 of --parent-lib (the library built from the parent commit) beside this build's
                        (readout_this_us) on the fused rows.

    python tools/bench_fuse.py [--frames 8 --size 480 854 --objects 3 --iters 20 --runs 2] [--parent-lib PATH/libfgvc_hip.so]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import struct
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import _lib, engine, ops  # noqa: E402
from tools.bench_refs import readout_with, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libfgvc_hip.so built from the parent commit: its fgvc_seg_readout_u8 is timed beside this build's")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    T, (h, w) = a.frames, a.size
    if T < 7:
        ap.error("--frames: at least 7 (maps at frames 0, 3 and 6)")
    torch.manual_seed(0)
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")),
                            test_cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, with_first=True,
                                          with_first_neighbor=True, masks="device", refs=dict(direction="both", override="all")))
    model.init_weights()
    model = model.to(dev).eval()
    g = torch.Generator().manual_seed(1)
    imgs = torch.randn(1, 1, 3, T, h, w, generator=g).clamp(-1, 1).to(dev)
    seg = torch.zeros(h, w, dtype=torch.uint8)
    for k in range(a.objects):
        y0, x0 = 60 + 100 * k, 100 + 220 * k
        seg[y0:y0 + 120, x0:x0 + 160] = k + 1
    maps = {t: torch.roll(seg, (2 * t, 2 * t), dims=(0, 1)).to(dev) for t in (0, 3, 6)}     # complete maps that move with time
    meta = [dict(original_shape=(h, w))]
    res = dict(frames=T, size=[h, w], objects=a.objects, iters=a.iters, runs=a.runs)

    def runs(fn, scale=1.0):
        return [round(scale * timed(fn, a.iters, a.warmup), 3) for _ in range(a.runs)]

    with torch.no_grad():
        session = model.open_label_session(imgs, meta)
        session.propagate({0: maps[0], 6: maps[6]})
        session.propagate({0: maps[0], 6: maps[6]}, fuse="linear")
        res["plain_second_ms"] = runs(lambda: session.propagate(maps))
        res["fused_second_ms"] = runs(lambda: session.propagate(maps, fuse="linear"))
        res["disagree"] = session.last_disagree.tolist()
        res["plain_second_again_ms"] = runs(lambda: session.propagate(maps))
        res["counters"] = dict(session.counters)
        res["sweeps_kept"] = sorted(f"{s}{d}" for s, d in session._sweeps)

        # the fuse launch and the read-out alone, on the two passes' rows of this clip
        Hf, Wf, pad = session.Hf, session.Wf, session.pad
        hp, wp = h + pad[2] + pad[3], w + pad[0] + pad[1]
        C = a.objects + 1
        segs = {t: torch.nn.functional.pad(m, pad).contiguous() for t, m in maps.items()}
        every = ops.label_set_words(range(C)).to(dev)

        def sweep(n, first, sw, inject):
            bank = torch.zeros((n, Hf * Wf, C), device=dev)
            ops.seg_onehot_labels(segs[first], Hf, Wf, C, out=bank[0])
            engine._sweep_refs(bank, bank, sw, Hf, Wf, False, inject)
            return bank
        soft_f = sweep(T, 0, session._sweeps[(0, "fw")], {3: (segs[3], every), 6: (segs[6], every)})
        soft_b = sweep(7, 6, session._sweeps[(6, "bw")], {3: (segs[3], every), 6: (segs[0], every)})
        session.close()
    mid = [1, 2, 4, 5]
    weights = [2 / 3, 1 / 3, 2 / 3, 1 / 3]
    out = torch.empty((len(mid), Hf * Wf, C), device=dev)
    res["fuse_launch_us"] = runs(lambda: ops.seg_fuse_rows(soft_f, soft_b, mid, [6 - t for t in mid], weights, out=out,
                                                           out_index=list(range(len(mid)))), 1e3)
    # the kernel without the wrapper's checks and item copy: BACK launches of the C entry back to back on ready item records, per launch
    BACK = 20
    bits = struct.unpack("<4i", struct.pack("<4f", *weights))
    items = torch.tensor([[t, 6 - t, i, b] for i, (t, b) in enumerate(zip(mid, bits))], dtype=torch.int32).to(dev)
    counts = torch.empty((len(mid),), device=dev, dtype=torch.int64)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def back_to_back():
        for _ in range(BACK):
            _lib.call("fgvc_seg_fuse_rows_f32", p(soft_f), p(soft_b), p(out), p(items), len(mid), T, 7, len(mid), Hf * Wf, C, p(counts), stream)
    res["fuse_kernel_us"] = runs(back_to_back, 1e3 / BACK)
    res["fuse_bytes"] = 3 * out.numel() * 4
    args = (Hf, Wf, (hp, wp), pad, (h, w))
    masks = torch.empty((T - 1, h, w), device=dev, dtype=torch.uint8)
    res["readout_rows_us"] = runs(lambda: ops.seg_readout(soft_f[1:], *args, True, out=masks), 1e3)
    ops.seg_fuse_rows(soft_f, soft_b, mid, [6 - t for t in mid], weights)
    res["readout_fused_us"] = runs(lambda: ops.seg_readout(soft_f[1:], *args, True, out=masks), 1e3)
    if a.parent_lib:
        this, parent = _lib.load(), ctypes.CDLL(a.parent_lib)
        ws = torch.empty((this.fgvc_seg_readout_workspace_bytes(T - 1, C) + 3) // 4, device=dev)
        want = ops.seg_readout(soft_f[1:], *args, True)
        for name, lib in (("readout_parent_us", parent), ("readout_this_us", this)):
            res[name] = runs(lambda: readout_with(lib, soft_f[1:], *args, masks, ws), 1e3)
            assert torch.equal(masks, want), name                   # the same bytes from either build
    print(json.dumps(res))


if __name__ == "__main__":
    main()
