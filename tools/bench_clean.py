#!/usr/bin/env python3
"""Time connected components and the cleaning rule on the device (fgvc_seg_components_i32, fgvc_seg_clean_u8) and
print one JSON line.

Maps, 480 x 854 with 3 objects, at 8 and at 70 frames:
  "speckle": tools/bench_jf.py's moving ellipses with planted specks (0.5 % of the pixels take a random id) and holes (0.5 % become 0);
  "model":   the untrained benchmark model's own masks of a random clip (VanillaTracker, test_cfg.masks='device').
Per map and clip length:
(a) "components_ms": one ops.seg_components call (three launches), median of HIP-event times; "clean_*_ms": one ops.seg_clean call with
    min_area alone (four launches), with keep='largest' too (five), and with fill_holes too (nine) -- the launches are not timed one by
    one, the three specs differ by whole launches; "..._c_entry_ms_in_a_burst": the C entry of the full spec back to back, 10 calls between
    one pair of events; "px_per_us": pixels over that time;
(b) "scipy_label_ms": scipy.ndimage.label per frame and id on the host copy (labelling alone: no areas, no drop, no fill), wall clock, when
    scipy is importable;
(c) "object_stats_ms": ops.object_stats of the map before and after the cleaning, in this process;
(d) 8 frames only: the mask call with and without test_cfg.clean, alternating, wall clock with a device synchronisation.
One frame of every map is held to metrics.clean_masks_host first.  Medians over --iters runs (at least 20) after --warmup, the whole
measurement twice ("run_0", "run_1").  One GPU shared with other work, clocks as the box sets them: compare the columns of one run with
each other, not with another run's.

    python tools/bench_clean.py [--iters 30]
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
from fgvc_amd import _lib, metrics, ops  # noqa: E402

BURST = 10
SPECS = {"min_area": dict(min_area=16), "min_area_largest": dict(min_area=16, keep="largest"),
         "min_area_largest_fill": dict(min_area=16, keep="largest", fill_holes=True)}
FULL = SPECS["min_area_largest_fill"]


def _bench_jf():
    spec = importlib.util.spec_from_file_location("fgvc_bench_jf", os.path.join(ROOT, "tools", "bench_jf.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def speckle(ids: np.ndarray, n: int, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    m = ids.copy()
    r = rng.random(m.shape)
    m[r < 0.005] = rng.integers(1, n + 1, size=int((r < 0.005).sum()), dtype=np.uint8)
    m[r > 0.995] = 0
    return m


def scipy_label_ms(ids_h: np.ndarray, n_ids: int):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    eight = ndimage.generate_binary_structure(2, 2)
    t0 = time.perf_counter()
    for frame in ids_h:
        for o in range(1, n_ids):
            ndimage.label(frame == o, structure=eight)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=2, default=(480, 854))
    ap.add_argument("--frames", type=int, nargs="+", default=(8, 70))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("tools/bench_clean.py times kernels on the GPU (fgvc_amd has no CPU path)")
    bj = _bench_jf()
    iters = max(20, a.iters)
    h, w = a.size
    dev = torch.device("cuda:0")
    n, n_ids = 3, 4
    lib = _lib.load()
    out = {"iters": iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "size": [h, w], "objects": n,
           "host_threads": torch.get_num_threads()}

    def model(**extra):
        m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,),
                                                                       pool_type="none", zero_init_residual=False)),
                            train_cfg=None, test_cfg=api.ConfigDict(**bj.TEST_CFG, masks="device", **extra))
        torch.manual_seed(0)
        m.init_weights()
        return m.to(dev).eval()
    without, with_key = model(), model(clean=dict(FULL))
    ref = torch.from_numpy(bj.ellipse_masks(1, h, w, n, 1)).to(dev)

    def clip(T):
        gen = torch.Generator().manual_seed(2)
        return dict(test_mode=True, imgs=torch.randn(1, 1, 3, T, h, w, generator=gen).to(dev), ref_seg_map=ref,
                    img_meta=[dict(original_shape=(h, w))])

    maps = {}
    for T in a.frames:
        maps[("speckle", T)] = torch.from_numpy(speckle(bj.ellipse_masks(T, h, w, n, 1), n, 7)).to(dev)
        with torch.no_grad():
            maps[("model", T)] = without(**clip(T))[0].clone()
    for (name, T), ids in maps.items():                                           # one frame of every map against the contract
        t = min(1, T - 1)
        got, st = ops.seg_clean(ids[t:t + 1], n_ids, **FULL)
        want, want_st = metrics.clean_masks_host(ids[t:t + 1].cpu().numpy(), n_ids, **FULL)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(st.cpu().numpy(), want_st), (name, T)

    for run in range(2):
        res = {}
        for (name, T), ids in maps.items():
            labels = torch.empty((T, h, w), device=dev, dtype=torch.int32)
            cleaned, stats = torch.empty_like(ids), torch.empty((T, n_ids, 4), device=dev, dtype=torch.int64)
            ws = torch.empty(ops.seg_clean_workspace_bytes(T, h, w, n_ids), device=dev, dtype=torch.uint8)
            r = {"components_ms": round(bj.timed_events(lambda: ops.seg_components(ids, out=labels), iters, a.warmup), 4)}
            for key, spec in SPECS.items():
                r[f"clean_{key}_ms"] = round(bj.timed_events(lambda: ops.seg_clean(ids, n_ids, out=cleaned, stats=stats, workspace=ws, **spec),
                                                            iters, a.warmup), 4)
            args = (ops._ptr(ids), ids.stride(0), ids.stride(1), T, h, w, n_ids, 8, FULL["min_area"], 1, 1, -1, None, ops._ptr(cleaned),
                    cleaned.stride(0), cleaned.stride(1), ops._ptr(stats), ops._ptr(ws), ws.numel(), ops._stream(ids))
            c_ms = bj.timed_events(lambda: [lib.fgvc_seg_clean_u8(*args) for _ in range(BURST)], iters, a.warmup) / BURST
            r["clean_min_area_largest_fill_c_entry_ms_in_a_burst"] = round(c_ms, 4)
            r["px_per_us"] = round(T * h * w / (c_ms * 1e3), 1)
            st = stats.cpu()[:, 1:].sum((0, 1)).tolist()
            r["components"], r["kept"], r["dropped_px"], r["filled_px"] = st
            if run == 0:
                ms = scipy_label_ms(ids.cpu().numpy(), n_ids)
                if ms is not None:
                    r["scipy_label_ms"] = round(ms, 1)
            o8 = torch.empty((T, n_ids, 8), device=dev, dtype=torch.int64)
            r["object_stats_ms_before"] = round(bj.timed_events(lambda: ops.object_stats(ids, n_ids, out=o8), iters, a.warmup), 4)
            r["object_stats_ms_after"] = round(bj.timed_events(lambda: ops.object_stats(cleaned, n_ids, out=o8), iters, a.warmup), 4)
            res[f"{name}_{T}f"] = r
        # (d) the mask call with and without the key, 8 frames
        call = clip(8)
        times = {"mask_call_ms": [], "mask_call_with_clean_ms": []}
        reps = max(5, iters // 3)
        with torch.no_grad():
            for it in range(3 + reps):
                for m, key in ((without, "mask_call_ms"), (with_key, "mask_call_with_clean_ms")):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    m(**call)
                    torch.cuda.synchronize()
                    if it >= 3:
                        times[key].append((time.perf_counter() - t0) * 1e3)
        res["mask_call_8f"] = {k: round(sorted(v)[len(v) // 2], 3) for k, v in times.items()}
        res["mask_call_8f"].update({k + "_range": [round(min(v), 3), round(max(v), 3)] for k, v in times.items()})
        out[f"run_{run}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
