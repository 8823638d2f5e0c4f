"""Time fgvc_merge_refine_topk_f32 alone on the lists of the flagship clip (cfg2: 8 frames of 480 x 854, 7 output rows x 25 680 queries,
T = 6): bench.py's model and seeds, the encoder and the pair kernel once, then ops.merge_refine_topk in rounds of launches between
device events.

    python tools/bench_refine.py                               # this tree's library
    python tools/bench_refine.py --arm parent=PATH/libfgvc_hip.so --arm change=fgvc_amd/lib/libfgvc_hip.so
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_refine.py --rounds 2      # the kernels one by one

With several arms (libraries built from different trees: the Python above them is this tree's) the rounds alternate between them, the
first round of each is thrown away, and the outputs and the statistics words of every arm are compared with the first arm's: idx,
logit and weight bit for bit, words 0-3, 6, 7 equal, words 4 and 5 (maxima) equal.  A gain counts when it exceeds three times the
larger arm's spread (max - min over the rounds)."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from fgvc_amd import _lib, engine, ops

ap = argparse.ArgumentParser()
ap.add_argument("--arm", action="append", default=[], help="NAME=PATH of a libfgvc_hip.so; default: this tree's library alone")
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--launches", type=int, default=100)
a = ap.parse_args()

dev = torch.device("cuda", 0)
wl = bench.WORKLOADS["cfg2_480p_8f"]
T, h, w = wl["frames"], wl["h"], wl["w"]
model = bench.build_tracker(wl, dev)
cfg = model.engine_config()
cfg.regroup = False
g = torch.Generator(device="cpu").manual_seed(1000)
rgbs = torch.stack([torch.randn(3, h, w, generator=g) for _ in range(T)]).to(dev)       # bench.py's video, frame by frame
with torch.no_grad():
    feats, Hf, Wf = model.get_feats_hwc(rgbs, split=True)
plan = engine.plan_clip(T, [0], cfg)
pl = engine.run_pairs(feats, Hf, Wf, plan, cfg)
assert pl.exact is not None, "the flagship configuration runs the refining merge"
pairs_dev, slot_pair, _ = plan.tables(dev)
n_out, n_slots = slot_pair.shape
ws = ops.merge_refine_workspace(n_out, Hf * Wf, dev)
torch.cuda.synchronize()
print(f"lists: {tuple(pl.idx.shape)} pairs x queries x k, {n_out} output rows, T = {n_slots}, grid {Hf} x {Wf}")


def open_lib(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib.SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib


prod = _lib.load()
arms = {"this tree": prod}
if a.arm:
    arms = {kv.partition("=")[0]: open_lib(kv.partition("=")[2]) for kv in a.arm}


def merge():
    return ops.merge_refine_topk(pl.idx, pl.score, slot_pair, pairs_dev, pl.exact, pl.exact, Hf, Wf, Hf, Wf, cfg.mask, cfg.topk,
                                 cfg.softmax_temperature(pl.channels), cfg.mode, eps=cfg.pair_refine_eps, workspace=ws)


def timeit(n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        merge()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


first = None
for name, lib in arms.items():
    _lib._lib = lib
    out = [x.clone() for x in merge()]
    torch.cuda.synchronize()
    words = out[3].cpu().tolist()
    print(f"{name:12s} statistics words {words}")
    if first is None:
        first = (name, out, words)
    else:
        for what, x, y in zip(("idx", "logit", "weight"), first[1], out):
            same = torch.equal(x.view(torch.int32), y.view(torch.int32))
            print(f"{name:12s} {what:6s} bit-identical to {first[0]}: {same}")
            assert same, what
        assert words == first[2], (words, first[2])
times = {name: [] for name in arms}
for r in range(a.rounds + 1):
    for name, lib in arms.items():
        _lib._lib = lib
        ms = timeit(a.launches)
        if r:
            times[name].append(ms)
_lib._lib = prod
for name, v in times.items():
    print(f"merge_refine_topk {name:12s} median {statistics.median(v) * 1e3:8.1f} us  (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f}; "
          f"{a.rounds} rounds x {a.launches} launches)")
if len(times) > 1:
    names = list(times)
    spread = max(max(v) - min(v) for v in times.values())
    for name in names[1:]:
        gain = statistics.median(times[names[0]]) - statistics.median(times[name])
        print(f"{names[0]} - {name} = {gain * 1e3:.1f} us against 3 x spread {3e3 * spread:.1f} us: {'clear' if gain > 3 * spread else 'NOT clear'}")
