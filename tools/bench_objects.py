#!/usr/bin/env python3
"""Time the object statistics kernel and the box stage of the renderer (fgvc_seg_object_stats_u8, fgvc_render_boxes_u8; DESIGN.md
section 27) and print one JSON line.

Inputs are synthetic and seeded: 480 x 854 id maps of two moving ellipses and one small object (tools/bench_jf.py's), at 8 and at 70 frames.
Per clip length:
(a) "object_stats_ms": one ops.object_stats call on maps already on the device, median of HIP-event times; "..._in_a_burst": time per call of
    10 calls between one pair of events (a single call between two events also counts its own start-up); "c_entry_ms_in_a_burst": the C
    entry itself back to back, without the Python wrapper's checks.  The kernel reads T h w bytes once; "gbps_of_id_bytes" is those
    bytes over the burst time, NOT a share of a roofline (one workgroup a frame: a clip of few frames leaves most of the chip idle);
(b) "torch_ms": the same eight words as torch launches on the same GPU (a dozen launches per id: masks, sums, any / argmax for the box);
(c) "host_contract_ms": metrics.object_stats_host on the host copy, wall clock, on the threads this process was granted;
(d) "render_boxes_ms" / "render_frames_ms": ops.render_boxes / ops.render_frames with the overlay, with and without boxes and id tags,
    alternating, HIP events; "..._c_entry_ms_in_a_burst": the two C entries back to back (the box wrapper reads two range flags back
    per call, which the event pair counts);
(e) 8 frames only: the mask call (VanillaTracker, test_cfg.masks='device') with and without test_cfg.objects, alternating, wall clock with
    a device synchronisation.
Medians over --iters runs (at least 20) after --warmup.  One GPU shared with other work, clocks as the box sets them: compare the
columns of one run with each other, not with another run's.

    python tools/bench_objects.py [--iters 30]
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
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import _lib, engine, metrics, ops  # noqa: E402

BURST = 10


def _bench_jf():
    spec = importlib.util.spec_from_file_location("fgvc_bench_jf", os.path.join(ROOT, "tools", "bench_jf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def torch_stats(ids: torch.Tensor, n_ids: int) -> torch.Tensor:
    """The eight words with torch operators, per id: what a user without the kernel launches."""
    T, h, w = ids.shape
    xs = torch.arange(w, device=ids.device)
    ys = torch.arange(h, device=ids.device)
    out = torch.zeros((T, n_ids, 8), device=ids.device, dtype=torch.int64)
    for o in range(n_ids):
        m = ids == o
        cols, rows = m.sum(1), m.sum(2)                                   # (T, w), (T, h)
        area = cols.sum(1)
        hx, hy = cols > 0, rows > 0
        x0, y0 = hx.int().argmax(1), hy.int().argmax(1)
        x1, y1 = w - hx.flip(1).int().argmax(1), h - hy.flip(1).int().argmax(1)
        border = m[:, 0].sum(1) + m[:, -1].sum(1) + m[:, 1:-1, 0].sum(1) + m[:, 1:-1, -1].sum(1)
        row = torch.stack([area, x0, y0, x1, y1, (cols * xs).sum(1), (rows * ys).sum(1), border], 1)
        out[:, o] = torch.where(area[:, None] > 0, row, torch.zeros_like(row))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    ap.add_argument("--frames", type=int, nargs="+", default=(8, 70))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_objects.py times kernels on the GPU (fgvc_amd has no CPU path)")
    bj = _bench_jf()
    iters = max(20, a.iters)
    h, w = a.size
    dev = torch.device("cuda:0")
    n, n_ids = 3, 4
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "size": [h, w], "objects": n,
           "host_threads": torch.get_num_threads()}
    from fgvc_amd import viz
    for T in a.frames:
        ids_h = bj.ellipse_masks(T, h, w, n, 1)
        ids = torch.from_numpy(ids_h).to(dev)
        stats = torch.empty((T, n_ids, 8), device=dev, dtype=torch.int64)
        want = torch.from_numpy(metrics.object_stats_host(ids_h, n_ids))
        assert torch.equal(ops.object_stats(ids, n_ids, out=stats).cpu(), want) and torch.equal(torch_stats(ids, n_ids).cpu(), want)
        k_ms = bj.timed_events(lambda: ops.object_stats(ids, n_ids, out=stats), iters, a.warmup)
        b_ms = bj.timed_events(lambda: [ops.object_stats(ids, n_ids, out=stats) for _ in range(BURST)], iters, a.warmup) / BURST
        lib, args = _lib.load(), (ops._ptr(ids), ids.stride(0), ids.stride(1), T, h, w, n_ids, ops._ptr(stats), ops._stream(ids))
        c_ms = bj.timed_events(lambda: [lib.fgvc_seg_object_stats_u8(*args) for _ in range(BURST)], iters, a.warmup) / BURST
        t_ms = bj.timed_events(lambda: torch_stats(ids, n_ids), iters, a.warmup)
        reps = max(3, iters // 10)
        t0 = time.perf_counter()
        for _ in range(reps):
            metrics.object_stats_host(ids_h, n_ids)
        h_ms = (time.perf_counter() - t0) * 1e3 / reps
        r = {"object_stats_ms": round(k_ms, 4), "object_stats_ms_in_a_burst": round(b_ms, 4), "c_entry_ms_in_a_burst": round(c_ms, 4),
             "id_bytes": T * h * w, "gbps_of_id_bytes": round(T * h * w / (c_ms * 1e-3) / 1e9, 1), "torch_ms": round(t_ms, 3),
             "host_contract_ms": round(h_ms, 2)}

        # (d) the renderer with and without the boxes, alternating
        frames = torch.from_numpy(np.random.default_rng(0).integers(0, 256, size=(T, h, w, 3), dtype=np.uint8)).to(dev)
        tr = engine.ObjectTracks(stats)
        present = tr.present.copy()
        present[:, 0] = False
        boxes, vis = torch.from_numpy(tr.boxes.copy()).to(dev).to(torch.int32), torch.from_numpy(present).to(dev)
        labels = torch.arange(n_ids, device=dev, dtype=torch.int32)
        rendered = torch.empty_like(frames)
        plain, boxed = [], []
        for it in range(a.warmup + iters):
            for fn, acc in ((lambda: ops.render_frames(frames, ids=ids, out=rendered), plain),
                            (lambda: ops.render_boxes(frames, boxes, vis, box_labels=labels, ids=ids, out=rendered), boxed)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                torch.cuda.synchronize()
                if it >= a.warmup:
                    acc.append(e0.elapsed_time(e1))
        r.update(render_frames_ms=round(sorted(plain)[len(plain) // 2], 4), render_boxes_ms=round(sorted(boxed)[len(boxed) // 2], 4),
                 render_frames_ms_range=[round(min(plain), 4), round(max(plain), 4)],
                 render_boxes_ms_range=[round(min(boxed), 4), round(max(boxed), 4)])
        # the two C entries back to back, with the arguments the wrappers passed (ops.render_boxes reads two flags back per call -- the
        # coordinate and label ranges it refuses by name -- and the device waits for the host meanwhile: the wrapper's time is not the kernel's)
        seen, call = {}, _lib.call
        _lib.call = lambda name, *args: (seen.__setitem__(name, args), call(name, *args))[1]
        try:
            ops.render_frames(frames, ids=ids, out=rendered)
            ops.render_boxes(frames, boxes, vis, box_labels=labels, ids=ids, out=rendered)       # (int32 inputs: the wrapper passes them as they are)
        finally:
            _lib.call = call
        for name, key in (("fgvc_render_frames_u8", "render_frames_c_entry_ms_in_a_burst"), ("fgvc_render_boxes_u8", "render_boxes_c_entry_ms_in_a_burst")):
            fn, args = getattr(lib, name), seen[name]
            r[key] = round(bj.timed_events(lambda: [fn(*args) for _ in range(BURST)], iters, a.warmup) / BURST, 4)
        host = viz.render(frames.cpu().numpy(), ids=ids_h, boxes=tr.boxes, box_visibles=present, box_labels=np.arange(n_ids))
        assert np.array_equal(ops.render_boxes(frames, boxes, vis, box_labels=labels, ids=ids).cpu().numpy(), host)       # the same bytes
        out[f"{T}_frames"] = r

    # (e) the mask call with and without the key, 8 frames
    def model(**extra):
        m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,),
                                                                       pool_type="none", zero_init_residual=False)),
                            train_cfg=None, test_cfg=api.ConfigDict(**bj.TEST_CFG, masks="device", **extra))
        torch.manual_seed(0)
        m.init_weights()
        return m.to(dev).eval()
    without, with_key = model(), model(objects=dict(stats=True))
    gen = torch.Generator().manual_seed(2)
    imgs = torch.randn(1, 1, 3, 8, h, w, generator=gen).to(dev)
    ref = torch.from_numpy(bj.ellipse_masks(1, h, w, n, 1)).to(dev)
    call = dict(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=[dict(original_shape=(h, w))])
    times = {"mask_call_ms": [], "mask_call_with_objects_ms": []}
    reps = max(5, iters // 3)
    with torch.no_grad():
        for it in range(3 + reps):
            for m, key in ((without, "mask_call_ms"), (with_key, "mask_call_with_objects_ms")):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m(**call)
                torch.cuda.synchronize()
                if it >= 3:
                    times[key].append((time.perf_counter() - t0) * 1e3)
    out["mask_call_8f"] = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
    out["mask_call_8f"].update({k + "_range": [round(min(v), 3), round(max(v), 3)] for k, v in times.items()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
