#!/usr/bin/env python3
"""Time the object crops (fgvc_seg_object_windows_i64, fgvc_frames_object_crops_u8) and print one JSON line.

Inputs are synthetic and seeded: 480 x 854 id maps of two moving ellipses and one small object (tools/bench_jf.py's) with 3 objects, at 8
and at 70 frames, crops of 128 x 128 with smooth = 2; the frames are random bytes, once at the masks' size and once at 1080 x 1920 (the
clip tracked at 480p, the crops taken from its source).  Per case:
(a) "windows_ms", "crops_ms", "crops_with_masks_ms": one ops.object_windows / ops.object_crops call on tensors already on the device,
    median of HIP-event times; "..._in_a_burst": time per call of 10 calls between one pair of events; "c_entries_ms_in_a_burst": the C
    entries (windows, then crops with masks) back to back, without the Python wrappers' checks and allocations;
(b) "bytes": what the chain has to move at least -- the frame bytes under the windows (clipped to the frame) once, the id bytes under the
    mask-space windows once, the crops and masks once -- and "share_of_8tbps": those bytes over the burst time against 8 TB/s.  The source
    rows of neighbouring bands overlap and each row is read once per column chunk, so the kernel reads more than that from the caches;
(c) "pillow_ms": the host loop a caller writes today -- Image.resize(size, BILINEAR, box=window) per frame and object on the host copy,
    wall clock; the same rule where no tap leaves the frame;
(d) "interpolate_ms": a loop of F.interpolate(window, size, mode='bilinear', antialias=True) on the same GPU over the windows clipped to
    the frame, HIP events: a time reference only, its rounding is float32 and not this rule's.
The device results are compared with viz.crop_windows_host on the first frames before anything is timed.  Medians over --iters runs (at
least 20) after --warmup.  One GPU shared with other work, clocks as the box sets them: compare the columns of one run with each other.

    python tools/bench_crops.py [--iters 30]
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fgvc_amd import _lib, metrics, ops, viz  # noqa: E402

BURST = 10


def _bench_jf():
    spec = importlib.util.spec_from_file_location("fgvc_bench_jf", os.path.join(ROOT, "tools", "bench_jf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def moved_bytes(win: np.ndarray, H: int, W: int, h: int, w: int, size, masks: bool) -> int:
    S_h, S_w = size
    total = 0
    for row in win.reshape(-1, 8).tolist():
        x0, y0, x1, y1, X0, Y0, X1, Y1 = row
        if X1 <= X0 or Y1 <= Y0:
            total += S_h * S_w * (4 if masks else 3)
            continue
        total += 3 * max(0, min(X1, W) - max(X0, 0)) * max(0, min(Y1, H) - max(Y0, 0)) + 3 * S_h * S_w
        if masks:
            total += min(S_w, max(0, min(x1, w) - max(x0, 0))) * min(S_h, max(0, min(y1, h) - max(y0, 0))) + S_h * S_w
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    ap.add_argument("--source", type=int, nargs=2, default=(1080, 1920))
    ap.add_argument("--crop-size", type=int, nargs=2, default=(128, 128))
    ap.add_argument("--frames", type=int, nargs="+", default=(8, 70))
    ap.add_argument("--smooth", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_crops.py times kernels on the GPU (fgvc_amd has no CPU path)")
    from PIL import Image
    bj = _bench_jf()
    iters = max(20, a.iters)
    h, w = a.size
    size = tuple(a.crop_size)
    dev = torch.device("cuda:0")
    n, n_ids = 3, 4
    objs = list(range(1, n_ids))
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "mask_size": [h, w], "objects": n, "crop_size": list(size),
           "smooth": a.smooth, "host_threads": torch.get_num_threads()}
    lib = _lib.load()
    for T in a.frames:
        ids_h = bj.ellipse_masks(T, h, w, n, 1)
        ids = torch.from_numpy(ids_h).to(dev)
        stats = ops.object_stats(ids, n_ids)
        stats_h = stats.cpu().numpy()
        for H, W in ((h, w), tuple(a.source)):
            frames_h = np.random.default_rng(0).integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)
            frames = torch.from_numpy(frames_h).to(dev)
            kw = dict(pad=0.125, min_side=8, smooth=a.smooth, mask_size=(h, w), frame_size=(H, W))
            win = torch.empty((T, n, 8), device=dev, dtype=torch.int64)
            crops = torch.empty((T, n, *size, 3), device=dev, dtype=torch.uint8)
            masks = torch.empty((T, n, *size), device=dev, dtype=torch.uint8)
            taps = viz.crop_default_taps((H, W), size)
            ws = torch.empty(ops.object_crops_workspace_bytes(T, n, size, (H, W)), device=dev, dtype=torch.uint8)
            ops.object_windows(stats, size, objects=objs, out=win, **kw)
            ops.object_crops(frames, win, size, ids=ids, objects=objs, out=crops, mask_out=masks, workspace=ws)
            win_h = metrics.object_windows_host(stats_h, size, objects=objs, **kw)
            assert np.array_equal(win.cpu().numpy(), win_h)
            k = min(T, 2)                                                  # the contract on the first frames: the same bytes
            want, wm = viz.crop_windows_host(frames_h[:k], win_h[:k], size, ids=ids_h[:k], objects=objs, max_taps=taps)
            assert np.array_equal(crops[:k].cpu().numpy(), want) and np.array_equal(masks[:k].cpu().numpy(), wm)

            r = {"max_taps": taps, "workspace_bytes": ws.numel()}
            r["windows_ms"] = round(bj.timed_events(lambda: ops.object_windows(stats, size, objects=objs, out=win, **kw), iters, a.warmup), 4)
            r["crops_ms"] = round(bj.timed_events(lambda: ops.object_crops(frames, win, size, out=crops, workspace=ws), iters, a.warmup), 4)
            with_masks = lambda: ops.object_crops(frames, win, size, ids=ids, objects=objs, out=crops, mask_out=masks, workspace=ws)  # noqa: E731
            r["crops_with_masks_ms"] = round(bj.timed_events(with_masks, iters, a.warmup), 4)
            r["crops_with_masks_ms_in_a_burst"] = round(bj.timed_events(lambda: [with_masks() for _ in range(BURST)], iters, a.warmup) / BURST, 4)
            seen, call = {}, _lib.call
            _lib.call = lambda name, *args: (seen.__setitem__(name, args), call(name, *args))[1]
            try:
                ops.object_windows(stats, size, objects=objs, out=win, **kw)
                with_masks()
            finally:
                _lib.call = call
            f_w, a_w = lib.fgvc_seg_object_windows_i64, seen["fgvc_seg_object_windows_i64"]
            f_c, a_c = lib.fgvc_frames_object_crops_u8, seen["fgvc_frames_object_crops_u8"]
            hold = [stats, win, ids, frames, crops, masks, ws]              # (the pointers in a_w / a_c stay alive)
            c_ms = bj.timed_events(lambda: [(f_w(*a_w), f_c(*a_c)) for _ in range(BURST)], iters, a.warmup) / BURST
            only = bj.timed_events(lambda: [f_c(*a_c) for _ in range(BURST)], iters, a.warmup) / BURST
            del hold
            nbytes = moved_bytes(win_h, H, W, h, w, size, True)
            r.update(c_entries_ms_in_a_burst=round(c_ms, 4), crops_c_entry_ms_in_a_burst=round(only, 4), bytes=nbytes,
                     gbps=round(nbytes / (only * 1e-3) / 1e9, 1), share_of_8tbps=round(nbytes / (only * 1e-3) / 8e12, 4))

            # (c) the host loop with Pillow
            reps = max(1, min(3, 200 // T))
            t0 = time.perf_counter()
            for _ in range(reps):
                for t in range(T):
                    im = Image.fromarray(frames_h[t])
                    for j in range(n):
                        X0, Y0, X1, Y1 = win_h[t, j, 4:].tolist()
                        if X1 > X0 and Y1 > Y0:
                            np.asarray(im.resize((size[1], size[0]), Image.BILINEAR, box=(max(X0, 0), max(Y0, 0), min(X1, W), min(Y1, H))))
            r["pillow_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 2)

            # (d) F.interpolate with antialias on the same GPU, window by window
            chw = frames.permute(0, 3, 1, 2).float().contiguous()

            def interpolate():
                for t in range(T):
                    for j in range(n):
                        X0, Y0, X1, Y1 = win_h[t, j, 4:].tolist()
                        if X1 > X0 and Y1 > Y0:
                            torch.nn.functional.interpolate(chw[t:t + 1, :, max(Y0, 0):min(Y1, H), max(X0, 0):min(X1, W)], size=size,
                                                            mode="bilinear", antialias=True, align_corners=False)
            r["interpolate_ms"] = round(bj.timed_events(interpolate, max(5, iters // 4), 2), 3)
            out[f"{T}_frames_from_{H}x{W}"] = r
            del frames, chw
    print(json.dumps(out))


if __name__ == "__main__":
    main()
