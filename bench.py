#!/usr/bin/env python3
"""Benchmark of the label-propagation hot path on MI355X (contract: see the task prompt / DESIGN.md section 6).

    python bench.py [--gpus N] [--steps K] [--warmup W]          # N > 1 without WORLD_SIZE in the environment: bench.py starts the N ranks
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W                  # ... or the launcher does (the driver's form)

A "step" = one synthetic 480x854 video of N x 8 frames (BASELINE.json configs[1]: an 8-frame 480p clip per GPU) through the
whole path, inputs resident in HBM, SHARDED BY CLIP over the N ranks exactly as BASELINE.json's north_star describes
(fgvc_amd.dist.track_points_sharded with the product backend): every rank encodes its own 8-frame clip (hand-written HIP ResNet-18
trunk on the matrix pipe; `--enc-arith`: f16 main product + block-scaled FP6 cross terms by default), rank 0 broadcasts the first-frame ("query") features over RCCL/xGMI, the 5-frame halo in front
of a clip comes from the previous rank by a point-to-point message, windowed correlation + top-10 for the clip's (query, key) frame
pairs (fgvc_pair_topk_f16f6: f16 main product + FP6 cross terms on the matrix pipe, f32 accumulate; `--pair-fmt f16`: three f16 products), slot merge + softmax,
all_gather of the merged lists, then the sequential label sweep + fused upsample / top-5 soft-argmax read-out over the whole video
(replicated; on a side stream so that the next step's encoder starts under it).  Nothing is skipped or cached across steps.
At N = 1 the same function runs without any collective (27 pairs, 7 propagations: the single-GPU figure of configs[1]).
Per-GPU work is fixed as N grows (one 8-frame clip each): scaling = "weak"; value = all frames of the video / time.
`--mode clips` times the reference's own data parallelism instead (independent 8-frame clips per rank, no data-path collective).

Rank 0 prints ONE JSON line.  `roofline` = the time-dominant kernel of the step (fgvc_conv_split_f32 256 -> 256 3x3, four
launches per clip and lane), priced both as algorithmic f32 FLOPs and as executed 16-bit pipe units (1.5 per product by default); `kernels` = the other
hand-written kernels of the step, each with its own roofline object (launch durations from HIP events inside the timed region, on
the launch stream); `corr_volume` = the dense materialised volume kernel that BASELINE.json's "ms/corr-volume" and the
>= 50 % HBM-roofline target refer to, timed right after the steps; `mfma_util` / `traffic` come from the committed rocprofv3 PMC
passes of the same kernels at the same shapes (profiles/r04_pmc.json, else the newest earlier one: counters cannot be read from inside this process);
`cpu_baseline` = the oracle (CPU restatement of the reference) timed on this box's host cores.

A plain run sets up, warms up, times the K steps and prints the line (`value`, `ms_per_step`, the figures read from the timed
steps' own HIP events).  Everything that takes runs of its own -- the repeat blocks and one-step latency, the pair kernel alone,
`clips_mode`, `value_f16x3` / `value_unrefined`, `corr_volume`, `cpu_baseline` -- runs with `--full` only.
`--dump-outputs DIR` writes what the last timed step returned (rank 0): DIR/traj.npy (T, P, 2) and, for a video, DIR/order.npy (P,),
float64.  The inputs are seeded: the same arguments give the same inputs on every run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

F32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
BF16_MFMA_PEAK_TFLOPS = 2500.0    # MI355X_MICROARCH.md: dense bf16 / f16 MFMA peak (no sparsity)
# pipe units (16-bit MFMA times) per f32-grade product of the pair kernels: fgvc_pair_topk_f16x3 = three f16 products (h*h, l*h, h*l),
# fgvc_pair_topk_f16f6 = one f16 product + both cross sums in FP6 (a quarter unit each)
PAIR_UNITS = {"f16": 3.0, "f16f6": 1.5}
# pipe units (16-bit MFMA times) per f32-grade product of fgvc_conv_split_f32, by arithmetic: bf16x3 / f16x3 = three 16-bit products,
# f16f8 = one f16 product + both cross sums in one K-64 fp8 MFMA (half a unit each), f16f6 = the same MFMA on FP6 operands (a quarter each)
CONV_UNITS = {"bf16x3": 3.0, "f16x3": 3.0, "f16f8": 2.0, "f16f6": 1.5}
HBM_PEAK_GBPS = 8000.0            # MI355X_MICROARCH.md: HBM3E spec peak (6.29 TB/s measured copy)
# what the board SUSTAINS on matrix work alone at its 1.4 kW cap (tools/micro/mfma_sustained.hip, profiles/r03_mfma_sustained.log): the
# 16-bit shapes do not reach the 2.4 GHz figure the roofline is priced against
SUSTAINED_TFLOPS = {"f16": 1750.0, "bf16": 1950.0, "fp8": 4900.0, "f16f8_mix_per_f16_unit": 2375.0}
STORE_CEILING_GBPS = 5680.0       # measured: plain dword stores over a 2.64 GB footprint (profiles/r03_store_footprint.log)

WORKLOADS = {
    # BASELINE.json configs[1]: 8 x 480x854 -> stride-4 features 120x214x256
    "cfg2_480p_8f": dict(frames=8, h=480, w=854, strides=(1, 2, 1, 1), out_indices=(2,), points=16),
    # configs[0] shape (CPU-runnable plumbing case), also handy for quick runs
    "cfg1_256_2f": dict(frames=2, h=256, w=256, strides=(1, 1, 1, 4), out_indices=(2,), points=8),
    # configs[4] shape: 720p 24-frame clip (stride-4 features 180x320x256)
    "cfg5_720p_24f": dict(frames=24, h=720, w=1280, strides=(1, 2, 1, 1), out_indices=(2,), points=16),
    # configs[3] shape: TAP-Vid-DAVIS-like clip
    "cfg4_davis_64f": dict(frames=64, h=256, w=256, strides=(1, 1, 1, 4), out_indices=(2,), points=32),
}


def encoder_flops(wl, n_frames: int) -> float:
    """ALGORITHMIC f32 FLOPs (2 x MACs) of the ResNet-18 trunk up to the output stage for n_frames frames: 7x7 stride-2 stem, no pool,
    stages of two BasicBlocks (two 3x3 convolutions each, a 1x1 projection where the block changes width or stride) --
    resnet.py:457-466, 254-325."""
    h, w = (wl["h"] - 1) // 2 + 1, (wl["w"] - 1) // 2 + 1
    fl = 2.0 * h * w * 3 * 64 * 49
    cin = 64
    for stage in range(wl["out_indices"][0] + 1):
        cout, stride = 64 * 2 ** stage, wl["strides"][stage]
        for blk in range(2):
            st = stride if blk == 0 else 1
            ho, wo = (h - 1) // st + 1, (w - 1) // st + 1
            fl += 2.0 * ho * wo * cin * cout * 9 + 2.0 * ho * wo * cout * cout * 9
            if blk == 0 and (st != 1 or cin != cout):
                fl += 2.0 * ho * wo * cin * cout
            h, w, cin = ho, wo, cout
    return fl * n_frames


def pmc(kernel: str):
    """Offline rocprofv3 PMC figures of `kernel` at the cfg2 shapes (profiles/r04_pmc.json, written by tools/pmc_report.py from
    separate --pmc passes, corrected as MI355X_MICROARCH.md prescribes); {} if absent."""
    for name in ("r05_pmc.json", "r04_pmc.json", "r03_pmc.json", "r02_pmc.json", "r01_pmc_traffic.json"):
        try:
            with open(os.path.join(ROOT, "profiles", name)) as f:
                d = json.load(f)
            if kernel in d:
                return d[kernel]
        except Exception:
            pass
    return {}


def build_tracker(wl, dev):
    import fgvc_amd.mmpt_api as api
    test_cfg = api.ConfigDict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=30, step=512,
                              with_first=True, with_first_neighbor=True, batch_step=8)
    model = api.build_model(dict(type="VanillaTracker",
                                 backbone=dict(type="ResNet", depth=18, strides=wl["strides"],
                                               out_indices=wl["out_indices"], pool_type="none",
                                               zero_init_residual=False)),
                            train_cfg=None, test_cfg=test_cfg)
    torch.manual_seed(0)
    model.init_weights()           # random-init weights of the named architecture (no checkpoints offline)
    return model.to(dev).eval()


def host_cpu():
    """(model name, physical cores, logical cpus) of this box, from /proc/cpuinfo."""
    model, phys, logical = "unknown", set(), 0
    try:
        pid = cid = None
        for line in open("/proc/cpuinfo"):
            k, _, v = line.partition(":")
            k, v = k.strip(), v.strip()
            if k == "model name":
                model = v
            elif k == "processor":
                logical += 1
            elif k == "physical id":
                pid = v
            elif k == "core id":
                cid = v
                phys.add((pid, cid))
    except Exception:
        pass
    return model, (len(phys) or None), (logical or os.cpu_count())


def cpu_baseline(wl, runs=3):
    """The oracle on the host cores: ONE whole query frame of the workload measured (median of `runs`): encoder for one frame, the
    masked affinity + top-k + propagation of the clip's last frame (every 512-query chunk, all its key slots, plain torch.topk and a
    pre-built mask like the reference), read-out of one frame; the clip's other frames are scaled by their key-slot counts."""
    import statistics
    from oracle import fgvc_oracle as O
    model, phys, logical = host_cpu()
    g = torch.Generator().manual_seed(0)
    h, w, T, P = wl["h"], wl["w"], wl["frames"], wl["points"]
    net = O.ResNet18(wl["strides"], wl["out_indices"][0], "none").eval()
    x = torch.randn(1, 3, h, w, generator=g)
    with torch.no_grad():
        f = net(torch.randn(1, 3, 64, 64, generator=g))                # spin up the thread pool / oneDNN
        f = net(x)
    C, Hf, Wf = f.shape[1:]
    HW = Hf * Wf
    ks = O.key_slots(T - 1)
    q = O.l2_normalize(torch.randn(C, Hf, Wf, generator=g), 0).reshape(C, -1)
    key = O.l2_normalize(torch.randn(C, len(ks), Hf, Wf, generator=g), 0).reshape(C, -1)
    val = torch.rand(P, len(ks) * HW, generator=g)
    lab = torch.rand(P, Hf, Wf, generator=g)
    step = 512
    chunks = [torch.arange(c0, min(HW, c0 + step)) for c0 in range(0, HW, step)]
    slots = sum(len(O.key_slots(fi)) for fi in range(1, T))               # 32 key slots for an 8-frame clip

    def one_frame():
        t0 = time.perf_counter()
        with torch.no_grad():
            net(x)
        t_enc = time.perf_counter() - t0
        t_mask = t_aff = 0.0
        for qi in chunks:
            t0 = time.perf_counter()
            m = O.mask_slab(Hf, Wf, Hf, Wf, len(ks), qi, 30, "circle")    # (the reference builds its mask once per video: timed apart)
            t_mask += time.perf_counter() - t0
            t0 = time.perf_counter()
            # the reference's per-chunk op sequence (local_attention.py:321-375): einsum, masked_fill_, plain topk, gather, softmax, sum
            idx, logit = O.affinity_chunk(key, q[:, qi], m, 10, 0.07, canonical=False)
            O.propagate_topk(val, idx, O.topk_weights(logit))
            t_aff += time.perf_counter() - t0
        t0 = time.perf_counter()
        O.img2coord(O.upsample_bilinear(lab, h, w).unsqueeze(0).numpy())
        t_read = time.perf_counter() - t0
        return t_enc, t_aff, t_read, t_mask / len(ks)

    def measure(threads, n):
        torch.set_num_threads(threads)
        O.affinity_chunk(key[:, :4096], q[:, :64], None, 10, 0.07, canonical=False)      # warm-up at this thread count
        rs = [one_frame() for _ in range(n)]
        med = [statistics.median(r[i] for r in rs) for i in range(4)]
        clip_s = T * med[0] + med[1] * slots / len(ks) + T * med[2] + med[3]
        return dict(threads=threads, runs=n, encoder_s_per_frame=med[0], attention_s_last_frame=med[1], readout_s_per_frame=med[2],
                    mask_build_s_per_video=med[3], clip_seconds=clip_s, frames_per_s=T / clip_s)

    aff, quota = granted_cpus()
    grant = max(1, int(min(aff, quota) if quota else aff))                 # the share of the host this process was given
    cores = min(grant, 32)                                                 # torch CPU ops stop scaling long before 256 threads here
    res = [measure(cores, runs)]
    if cores >= 32 and grant >= 64:
        res.append(measure(16, 2))                                         # a second thread count, for the scaling of the port
    best = max(res, key=lambda r: r["frames_per_s"])
    return dict(value=best["frames_per_s"], unit="frames/s", cores=best["threads"], kind="port", measurement="measured frame",
                granted_cpus=dict(sched_affinity=aff, cgroup_quota=quota, used_threads=best["threads"]),
                runs=best["runs"],
                sample=f"1 whole frame x{best['runs']} (median): encoder, all {len(chunks)} chunks x {len(ks)} key slots, read-out",
                host_cpu=dict(model=model, physical_cores=phys, logical_cpus=logical),
                thread_counts=res,
                note=(f"oracle/fgvc_oracle.py (plain torch.topk, pre-built mask like the reference); the clip's {T} frames = {T} encoder + "
                      f"read-out passes and {slots} key slots of attention, the measured last frame has {len(ks)}"),
                clip_seconds_est=best["clip_seconds"])


def self_launch(n: int) -> int:
    """Start `n` ranks of this script under torch.distributed.run on 127.0.0.1 (a free port), relay their output, return the launcher's
    exit code (non-zero if any rank failed).  Runs in a parent that has made no GPU call: the ranks are fresh child processes."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")            # dmabuf IPC: RCCL / device-tensor sharing between the ranks
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def granted_cpus():
    """CPUs this process may actually use: its affinity mask, capped by the cgroup's CPU quota where one is set (a GPU box grants a
    share of its host's cores; torch's default thread count = all logical CPUs oversubscribes that share)."""
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        n = os.cpu_count() or 1
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]          # cgroup v2
        if q != "max":
            quota = float(q) / float(per)
    except Exception:
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())    # cgroup v1
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except Exception:
            pass
    return n, quota


class KernelProbe:
    """HIP events around chosen launches, recorded on the launch's own stream (the encoder's lanes run on side streams)."""

    def __init__(self):
        self.on = False
        self.ev = {}

    def wrap(self, fn, tag_of):
        def wrapped(*a, **k):
            tag = tag_of(*a, **k) if self.on else None
            if tag is None:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            self.ev.setdefault(tag, []).append((e0, e1))
            return r
        return wrapped

    def mean_ms(self, tag):
        ev = self.ev.get(tag, [])
        return (sum(a.elapsed_time(b) for a, b in ev) / len(ev), len(ev)) if ev else (None, 0)


def dump_outputs(out_dir: str, **arrays):
    """`--dump-outputs`: every array given as out_dir/<name>.npy in float64 (None = not produced by this mode).  The timed path
    returns trajectories of a few points (T x P x 2): far below the 64 MB a dump may take, so nothing is sampled."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        if t is not None:
            np.save(os.path.join(out_dir, name + ".npy"), t.detach().to("cpu", torch.float64).numpy())


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--workload", default="cfg2_480p_8f", choices=sorted(WORKLOADS))
    ap.add_argument("--mode", default="video", choices=["video", "clips"],
                    help="video = one N x T-frame video per step, sharded by clip over the ranks (broadcast + halo message + "
                         "all_gather in the data path); clips = an independent T-frame clip per rank per step (no collective)")
    ap.add_argument("--halo", default="exchange", choices=["exchange", "recompute", "auto"],
                    help="auto: exchange or recompute from the schedule's byte and pair counts and a 16 MB link ping at start-up (fgvc_amd.dist.choose_halo)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also everything the headline figure does not need: the repeat blocks and one-step latency, "
                         "the pair kernel alone, the clips-mode and precision lines, the dense corr-volume section, the CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned as DIR/<name>.npy (float64; rank 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-corr-volume", action="store_true", help="with --full: skip the dense corr-volume section")
    ap.add_argument("--no-autotune", action="store_true", help="MIOpen immediate mode (clean profiles)")
    ap.add_argument("--pair-precision", default="auto", choices=["auto", "f32", "split"],
                    help="pair top-k kernel: split = the 16-bit matrix pipe (default where it applies), f32 = fgvc_pair_topk_f32")
    ap.add_argument("--pair-fmt", default="auto", choices=["auto", "f16", "f16f6"],
                    help="arithmetic of the split pair kernel: f16 = fgvc_pair_topk_f16x3 (three f16 products, 1e-7-grade), f16f6 = "
                         "fgvc_pair_topk_f16f6 (f16 + FP6 cross terms, ~6e-5 logit); auto = f16f6 with an f16f8 encoder, f16 otherwise")
    ap.add_argument("--no-f16x3-line", action="store_true", help="with --full: skip the extra steps in the highest-precision arithmetic (`value_f16x3`)")
    ap.add_argument("--encoder-lanes", type=int, default=None,
                    help="batch slices of the encoder run on this many HIP streams at once (default: ResNet.split_lanes)")
    ap.add_argument("--sync-tail", action="store_true",
                    help="label sweep + read-out on the main stream (default: on a side stream, so that the next step's encoder "
                         "overlaps this step's chain of small launches; every step is complete before the closing barrier)")
    ap.add_argument("--tail-priority", type=int, default=0, help="HIP priority of the side stream (lower = dispatched first; A/B)")
    ap.add_argument("--lane-priority", type=int, default=0, help="HIP priority of the encoder's lane streams (ResNet.lane_priority; A/B)")
    ap.add_argument("--tail-from", default="pairs", choices=["sweep", "pairs"],
                    help="what runs on the side stream: the label sweep + read-out only, or everything after the encoder (pair top-k, "
                         "merge, exchange steps, sweep): the next step's encoder then runs beside this step's pair kernel")
    ap.add_argument("--merge-on-main", action="store_true", help="the slot merge (+ exact re-scoring) behind the pair kernel on the main stream instead of "
                                                                 "on the side stream with the sweep (HipBackend.merge_on_tail = False; A/B)")
    ap.add_argument("--no-layer1-whole-batch", action="store_true", help="the stem and layer 1 per stream lane instead of once over the whole batch (ResNet.layer1_whole_batch; A/B)")
    ap.add_argument("--no-conv64", action="store_true", help="64-channel layers on the generic fgvc_conv_split_f32 (A/B)")
    ap.add_argument("--conv64-f16f8", action="store_true", help="with --enc-arith f16f8: layer 1 and the stem's output in the f16 + fp8 form too (ResNet.conv64_f16f8; A/B)")
    ap.add_argument("--no-conv64-f16f8", action="store_true", help="layer 1 and the stem's output in the bf16 form also when the trunk computes in f16f8 (A/B)")
    ap.add_argument("--encoder-graph", action="store_true", help="replay the encoder from a HIP graph (ResNet.use_graph: host time per call 0.7 -> 0.1 ms; "
                                                                 "no throughput change where the step is GPU-bound)")
    ap.add_argument("--no-encoder-graph", action="store_true", help="never replay the encoder from a HIP graph (default: ResNet.use_graph = 'auto': small inputs only)")
    ap.add_argument("--no-fuse-bank", action="store_true", help="the two-kernel route to the feature bank (dense f32 output + normalise pass) instead of "
                                                                "the last convolution's own epilogue (ResNet.fuse_bank; A/B)")
    ap.add_argument("--no-fold-projection", action="store_true", help="layer 3's 1 x 1 projection shortcut as its own launch + dense f32 identity instead of "
                                                                      "extra stages of the block's second convolution (ResNet.fold_projection; A/B)")
    ap.add_argument("--res-split", action="store_true", help="layer-1 identities from the split form instead of dense f32 copies (A/B)")
    ap.add_argument("--enc-arith", default=None, choices=["f16f8", "f16f6", "bf16x3", "f16x3"],
                    help="arithmetic of the encoder's wide convolutions (default: ResNet.arith = f16f6; f16f8 = round 3's, bf16x3 = round 2's)")
    ap.add_argument("--no-clips-line", action="store_true", help="with --full: skip the extra `--mode clips` measurement that a `video` run appends")
    ap.add_argument("--repeats", type=int, default=5, help="with --full: extra blocks of 20 steps after the timed region, for the spread")
    ap.add_argument("--set-option", action="append", default=[], metavar="NAME=VALUE",
                    help="fgvc_set_option knobs for A/B runs, e.g. --set-option conv_narrow=1")
    ap.add_argument("--comm-timeout", type=float, default=180.0, help="seconds before a collective that does not complete aborts the job (rc != 0)")
    ap.add_argument("--rehearse-on-one-gpu", action="store_true",
                    help="N > 1 ranks on ONE GPU over gloo (device tensors staged through the host by fgvc_amd.dist): exercises every "
                         "line of the multi-rank path on a one-GPU box; the number it prints is NOT a measurement (RCCL refuses two "
                         "ranks on one device, hence gloo)")
    return ap.parse_args()


def setup_workload(L):
    """model, data, kernel probe, backend of one run: everything the timed loop needs.  `L`: the run's namespace (main() threads one dict through the phases)."""
    a, dev, engine, fdist, ops, rank, world = L.get("a"), L.get("dev"), L.get("engine"), L.get("fdist"), L.get("ops"), L.get("rank"), L.get("world")
    for kv in a.set_option:
        name, _, val = kv.partition("=")
        ops.set_option(name, int(val))
    wl = WORKLOADS[a.workload]
    Tc, h, w, P = wl["frames"], wl["h"], wl["w"], wl["points"]
    T = Tc * world if a.mode == "video" else Tc                    # frames of the video of one step (per rank in `clips` mode)
    torch.backends.cudnn.benchmark = not a.no_autotune
    from fgvc_amd.mmpt_api.backbones import ResNet
    if a.encoder_lanes is not None:
        ResNet.split_lanes = a.encoder_lanes
    if a.no_conv64:
        ResNet.use_conv64 = False
    ResNet.lane_priority = a.lane_priority
    if a.no_layer1_whole_batch:
        ResNet.layer1_whole_batch = False
    if a.encoder_graph:
        ResNet.use_graph = True
    if a.no_fuse_bank:
        ResNet.fuse_bank = False
    if a.no_fold_projection:
        ResNet.fold_projection = False
    if a.no_encoder_graph:
        ResNet.use_graph = False
    if a.res_split:
        ResNet.res_from_split = True
    if a.conv64_f16f8:
        ResNet.conv64_f16f8 = True
    if a.no_conv64_f16f8:
        ResNet.conv64_f16f8 = False
    model = build_tracker(wl, dev)
    if a.enc_arith:
        model.backbone.set_arith(a.enc_arith)
    arith = model.backbone.arith
    if a.pair_fmt != "auto":
        model.test_cfg["pair_split_fmt"] = a.pair_fmt
    cfg = model.engine_config()
    pair_fmt = cfg.pair_split_fmt
    cfg.pair_precision = a.pair_precision
    cfg.regroup = False                                              # all points are given at frame 0 of the video

    halo_why = None
    if a.halo == "auto" and a.mode == "video":                       # resolved once, from numbers every rank holds (the link figure is broadcast)
        halo_why = fdist.choose_halo(T, world, [0], cfg, fdist.halo_cost_model(h, w),
                                     fdist.measure_link_gbps(None, dev) if world > 1 else fdist.LINK_GBPS_ASSUMED)
        a.halo = halo_why["mode"]
    elif a.halo == "auto":
        a.halo = "exchange"
    # the same video on every rank (seeded): a rank only ever touches its own frames of it
    g = torch.Generator(device="cpu").manual_seed(1000 if a.mode == "video" else 1000 + rank)
    lo, hi = (fdist.shard_frames(T, world, first=1)[rank] if a.mode == "video" else (1, T))
    e_lo = 0 if (rank == 0 or a.mode == "clips") else lo
    frames_all = None
    rgbs = torch.empty((T, 3, h, w), dtype=torch.float32, device=dev) if a.mode == "video" else None
    if a.mode == "video":
        for f in range(T):                                           # generate frame by frame: identical stream on every rank
            fr = torch.randn(3, h, w, generator=g)
            if e_lo <= f < hi or (a.halo == "recompute" and lo - cfg.precede_frames <= f < hi):
                rgbs[f] = fr.to(dev)
    else:
        rgbs = torch.randn(T, 3, h, w, generator=g).to(dev)
    qp = torch.cat([torch.zeros(P, 1), torch.rand(P, 2, generator=torch.Generator().manual_seed(7)) * torch.tensor([w - 1.0, h - 1.0])], 1)
    pts = qp[:, 1:].to(dev)

    probe = KernelProbe()
    # launch probes: the 256 -> 256 3x3 convolutions of encoder layer 3 and the pair top-k, timed where they run
    # (tag = (name, frames, channels of a folded projection's input): all three forms of the layer's kernel -- plain, with layer 3's projection
    # shortcut in its sums, and the bank-writing last one)
    ops.conv_split = probe.wrap(ops.conv_split, lambda x, wt, *r, **k: ("conv256", x.shape[0], 0 if k.get("x2_split") is None else k["x2_split"].shape[3] * 32)
                                if (wt.shape[0] == 9 and wt.shape[2] == 256 and x.shape[3] * 32 == 256) else None)
    ops.conv_split_to_bank = probe.wrap(ops.conv_split_to_bank, lambda x, wt, *r, **k: ("conv256", x.shape[0], 0) if x.shape[3] * 32 == 256 else None)
    ops.pair_topk_split = probe.wrap(ops.pair_topk_split, lambda q, k_, prs, *r, **kw: ("pair_split", prs.shape[0]))
    ops.pair_topk = probe.wrap(ops.pair_topk, lambda q, k_, prs, *r, **kw: ("pair_f32", prs.shape[0]))
    ops.merge_refine_topk = probe.wrap(ops.merge_refine_topk, lambda pi, *r, **kw: ("merge_refine", pi.shape[0]))
    ops.merge_topk = probe.wrap(ops.merge_topk, lambda pi, *r, **kw: ("merge", pi.shape[0]))

    tail_stream = None if a.sync_tail else torch.cuda.Stream(dev, priority=a.tail_priority)
    backend = fdist.HipBackend(model, tail_stream=tail_stream, tail_from=a.tail_from)
    backend.merge_on_tail = not a.merge_on_main
    if os.environ.get("FGVC_EARLY_HALO", "1") == "0":               # escape hatch: the halo posted after the whole encoder pass (round 2's order)
        backend.early_halo = False
    timing = fdist.Timing(dev)
    plan1 = engine.plan_clip(Tc, [0], cfg)
    state = {}
    sched_cache = {}
    _out = ('P', 'T', 'Tc', '_', 'arith', 'backend', 'cfg', 'e_lo', 'h', 'halo_why', 'hi', 'lo', 'model', 'name', 'pair_fmt', 'plan1', 'probe', 'pts', 'qp', 'rgbs', 'sched_cache', 'state', 'tail_stream', 'timing', 'w', 'wl')
    L.update({k_: v_ for k_, v_ in locals().items() if k_ in _out})


def timed_steps(L):
    """warm-up, EXACTLY a.steps timed steps between barrier + synchronise (max over ranks), failure flags, `--dump-outputs`, the repeat blocks (--full).  `L`: the run's namespace (main() threads one dict through the phases)."""
    T, _, a, backend, cfg, dev, engine, fdist, h, model, ops, plan1 = L.get("T"), L.get("_"), L.get("a"), L.get("backend"), L.get("cfg"), L.get("dev"), L.get("engine"), L.get("fdist"), L.get("h"), L.get("model"), L.get("ops"), L.get("plan1")
    probe, pts, qp, rgbs, sched_cache, state, tail_stream, timing, w, world = L.get("probe"), L.get("pts"), L.get("qp"), L.get("rgbs"), L.get("sched_cache"), L.get("state"), L.get("tail_stream"), L.get("timing"), L.get("w"), L.get("world")
    rank = L.get("rank")
    def step(timed: bool):
        if a.mode == "video":
            traj, state["order"] = fdist.track_points_sharded(backend, rgbs, qp, cfg, device=dev, halo=a.halo, timing=timing if timed else None,
                                                               cache=sched_cache, check=False)      # (the failure flags are read once after the timed loop)
            return traj
        feats, Hf, Wf = model.get_feats_hwc(rgbs, split=True)          # encoder + normalise (+ split), all T frames
        state["geom"] = (Hf, Wf, feats)
        pl = engine.run_pairs(feats, Hf, Wf, plan1, cfg)
        if tail_stream is None:
            tk = engine.merge_pairs(pl, cfg)
            return engine.run_propagation(tk, 0, pts, Hf, Wf, h, w, cfg)[1]
        return engine.run_propagation_async(pl, 0, pts, Hf, Wf, h, w, cfg, tail_stream)[1]

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    if world > 1:
        assert dist.get_world_size() == a.gpus == world
    for _ in range(a.warmup):
        step(False)
    barrier()
    fdist.reset_comm_bytes()
    probe.on = True
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out_coords = step(True)
    barrier()
    elapsed = time.perf_counter() - t0
    probe.on = False
    if world > 1:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    comm = {k: v / a.steps for k, v in fdist.COMM_BYTES.items()}
    assert bool(torch.isfinite(out_coords).all())
    if ops.pair_f16x3_timed_out():
        raise SystemExit("bench.py: fgvc_pair_topk_f16x3 reported a timed-out wait of its LDS protocol: results invalid")
    if model.backbone.check_overflow():
        raise SystemExit("bench.py: an encoder activation left the f16 range of its calibrated scale: results invalid")
    n_frames_total = T * a.steps if a.mode == "video" else world * T * a.steps
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, traj=out_coords, order=state.get("order") if a.mode == "video" else None)

    # spread: a few more short blocks (not part of `value`)
    rep = []
    for _ in range(max(0, a.repeats) if a.full else 0):
        barrier()
        t1 = time.perf_counter()
        for _ in range(20):
            step(False)
        barrier()
        rep.append((time.perf_counter() - t1) / 20 * 1e3)
    # one step at a time (synchronised on both sides): what a caller with ONE clip waits for -- the timed region above overlaps each
    # step's side-stream work (pair top-k, merge, sweep with --tail-from pairs) with the next step's encoder
    lat = []
    for _ in range(10 if a.full and a.repeats > 0 else 0):
        barrier()
        t1 = time.perf_counter()
        step(False)
        barrier()
        lat.append((time.perf_counter() - t1) * 1e3)
    _out = ('_', 'barrier', 'comm', 'elapsed', 'lat', 'n_frames_total', 'out_coords', 'rep', 't', 't1')
    L.update({k_: v_ for k_, v_ in locals().items() if k_ in _out})


def roofline_objects(L):
    """per-kernel roofline objects from the HIP events of the timed region and the committed PMC passes.  `L`: the run's namespace (main() threads one dict through the phases)."""
    Tc, a, arith, backend, cfg, h, name, ops, pair_fmt, plan1, probe, t = L.get("Tc"), L.get("a"), L.get("arith"), L.get("backend"), L.get("cfg"), L.get("h"), L.get("name"), L.get("ops"), L.get("pair_fmt"), L.get("plan1"), L.get("probe"), L.get("t")
    w, wl, world = L.get("w"), L.get("wl"), L.get("world")
    Hf, Wf = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    for s_ in wl["strides"][:wl["out_indices"][0] + 1]:
        Hf, Wf = (Hf - 1) // s_ + 1, (Wf - 1) // s_ + 1
    HW, C = Hf * Wf, 256
    n_pairs_clip = len(plan1.pairs)

    # ---- roofline objects ---------------------------------------------------------------------------------------------------
    kernels = {}
    conv_tags = [t for t in probe.ev if t[0] == "conv256"]
    if conv_tags:
        # per launch: the lane's batch slice (N frames) of one 256 -> 256 3x3 convolution
        tot_ms = sum(sum(e0.elapsed_time(e1) for e0, e1 in probe.ev[t]) for t in conv_tags)
        tot_fl = sum(len(probe.ev[t]) * 2.0 * t[1] * HW * 256 * (256 * 9 + t[2]) for t in conv_tags)      # (+ the folded 1 x 1 projection's products)
        n_l = sum(len(probe.ev[t]) for t in conv_tags)
        f32_tf = tot_fl / (tot_ms * 1e-3) / 1e12
        pm = pmc("fgvc_conv_split_fmt_f32[%s]" % arith if arith in ("f16f8", "f16f6") else "fgvc_conv_split_f32")   # (no PMC pass of the f16x3 form)
        kernels["encoder_conv"] = {
            "kernel": "fgvc_conv_split_fmt_f32",      # (256 -> 256 3x3; its _proj_ and _bank_ entry points are instances of the same kernel: DESIGN section 6)
            "bound": "mfma", "achieved": f32_tf, "peak": BF16_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": f32_tf / BF16_MFMA_PEAK_TFLOPS,
            "what": "algorithmic f32 FLOPs (2 N H W 256 256 9 + folded projection) / mean launch time vs the 16-bit MFMA peak",
            "arith": arith,
            "executed_tflops": CONV_UNITS[arith] * f32_tf, "frac_executed": CONV_UNITS[arith] * f32_tf / BF16_MFMA_PEAK_TFLOPS,
            "executed_note": {"bf16x3": "3 bf16 partial products per f32-grade product (hi*hi + hi*lo + lo*hi)",
                              "f16x3": "3 f16 partial products per f32-grade product (h*h + h*l + l*h)",
                              "f16f8": "2 pipe units per f32-grade product: the f16 main product + both cross sums in one K-64 fp8 MFMA "
                                       "(twice the f16 rate)",
                              "f16f6": "1.5 pipe units per f32-grade product: the f16 main product + both cross sums in one K-64 FP6 MFMA "
                                       "(block-scaled e2m3 operands: four times the f16 rate)"}[arith],
            "frac_of_f32_mfma_peak": f32_tf / F32_MFMA_PEAK_TFLOPS,
            "sustained_peak": {"bf16x3": SUSTAINED_TFLOPS["bf16"], "f16x3": SUSTAINED_TFLOPS["f16"],
                               "f16f8": SUSTAINED_TFLOPS["f16f8_mix_per_f16_unit"], "f16f6": SUSTAINED_TFLOPS["f16f8_mix_per_f16_unit"]}[arith],
            "frac_executed_of_sustained": CONV_UNITS[arith] * f32_tf / {"bf16x3": SUSTAINED_TFLOPS["bf16"], "f16x3": SUSTAINED_TFLOPS["f16"],
                                                                        "f16f8": SUSTAINED_TFLOPS["f16f8_mix_per_f16_unit"],
                                                                        "f16f6": SUSTAINED_TFLOPS["f16f8_mix_per_f16_unit"]}[arith],
            "sustained_note": "matrix pipe alone at the power cap: profiles/r03_mfma_sustained.log",
            "ms_per_launch": tot_ms / n_l, "launches_timed": n_l,
            "launch_note": "HIP events on the lane's stream in the timed region (lanes overlap: rocprofv3 kernel-only times are 5-8 % shorter)",
            "mfma_util": pm.get("mfma_util"), "traffic": pm.get("hbm_bytes_per_launch"),
            "pmc_note": "rocprofv3 PMC passes of one whole-clip launch alone (profiles/r0N_pmc.json)"}
    pair_tag = next((t for t in probe.ev if t[0] in ("pair_split", "pair_f32")), None)
    if pair_tag:
        pair_ms, n_l = probe.mean_ms(pair_tag)
        n_disc = sum(1 for dy in range(-40, 41) for dx in range(-40, 41) if dy * dy + dx * dx <= cfg.mask.r2max)
        fl = 2.0 * HW * n_disc * C * pair_tag[1]                       # windowed FLOPs of the launch's pairs
        f32_tf = fl / (pair_ms * 1e-3) / 1e12
        split = pair_tag[0] == "pair_split"
        name = ({"f16f6x": "fgvc_pair_topk_f16f6x", "f16f6": "fgvc_pair_topk_f16f6"}.get(cfg.bank_fmt, "fgvc_pair_topk_f16x3")) if split else "fgvc_pair_topk_f32"
        n_prod = PAIR_UNITS[pair_fmt] if split else 1
        pm = pmc(name) or pmc(name.replace("f16f6x", "f16f6"))
        kernels["pair_topk"] = {
            "kernel": name, "bound": "mfma", "achieved": f32_tf, "peak": BF16_MFMA_PEAK_TFLOPS if split else F32_MFMA_PEAK_TFLOPS,
            "unit": "TFLOP/s", "frac": f32_tf / (BF16_MFMA_PEAK_TFLOPS if split else F32_MFMA_PEAK_TFLOPS),
            "what": "ALGORITHMIC windowed f32 FLOPs (2 HW N_disc C per pair, N_disc = 697) / mean launch duration",
            "executed_tflops": n_prod * f32_tf,
            "frac_executed": (n_prod * f32_tf / BF16_MFMA_PEAK_TFLOPS) if split else f32_tf / F32_MFMA_PEAK_TFLOPS,
            "executed_note": f"{n_prod} 16-bit pipe units per f32-grade product (f16x3: h*h + l*h + h*l; f16f6: h*h on the f16 pipe + "
                             "h6*l6 + l6*h6 in FP6 at four times the rate), in-window candidates only (the 4x8-block tiling multiplies "
                             "1312 candidates per query for 697 in the disc)"
                             if split else "exact f32 MFMA",
            "pair_fmt": pair_fmt if split else "f32",
            "frac_of_f32_mfma_peak": f32_tf / F32_MFMA_PEAK_TFLOPS,
            "ms_per_launch": pair_ms, "pairs_per_launch": pair_tag[1], "launches_timed": n_l,
            "mfma_util": pm.get("mfma_util"), "traffic": pm.get("hbm_bytes_per_launch")}
        # In the step the launch runs on the side stream BESIDE the next step's encoder (--tail-from pairs): its in-step duration is
        # stretched by what it shares the CUs with.  The kernel's own figure: the same launch alone on an idle chip, timed right here (--full).
        alone_applies = split and a.mode == "video" and world == 1 and pair_tag[1] == n_pairs_clip and not a.sync_tail and a.tail_from == "pairs"
        if alone_applies and not a.full:      # every key means what it does in a --full run: the alone figures are not measured here
            kernels["pair_topk"].update(ms_per_launch_in_step=pair_ms, ms_per_launch=None, achieved=None, frac=None, executed_tflops=None,
                                        frac_executed=None, frac_of_f32_mfma_peak=None,
                                        launch_note="ms_per_launch and the fractions (the launch ALONE on an idle chip): --full only; "
                                                    "ms_per_launch_in_step: HIP events in the timed region, where it runs beside the next step's encoder")
        if alone_applies and a.full:
            import torch
            model, rgbs, engine = L.get("model"), L.get("rgbs"), L.get("engine")
            torch.cuda.synchronize()
            feats_, Hf_, Wf_ = model.get_feats_hwc(rgbs, split=True)
            probe.on = False
            for _ in range(3):
                engine.run_pairs(feats_, Hf_, Wf_, plan1, cfg)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                engine.run_pairs(feats_, Hf_, Wf_, plan1, cfg)
            e1.record()
            torch.cuda.synchronize()
            alone = e0.elapsed_time(e1) / 10
            k_ = kernels["pair_topk"]
            k_.update(ms_per_launch_in_step=pair_ms, ms_per_launch=alone, achieved=fl / (alone * 1e-3) / 1e12,
                      frac=fl / (alone * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, executed_tflops=n_prod * fl / (alone * 1e-3) / 1e12,
                      frac_executed=n_prod * fl / (alone * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                      frac_of_f32_mfma_peak=fl / (alone * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS,
                      launch_note="ms_per_launch and the fractions: the launch ALONE (10 launches on an idle chip after the timed steps); "
                                  "ms_per_launch_in_step: HIP events in the timed region, where it runs beside the next step's encoder")
            del feats_
    for tag_ in [t for t in probe.ev if t[0] in ("merge_refine", "merge")]:
        ms_, n_ = probe.mean_ms(tag_)
        kernels[tag_[0]] = {"kernel": "fgvc_merge_refine_topk_f32" if tag_[0] == "merge_refine" else "fgvc_merge_topk_f32", "ms_per_launch": ms_,
                            "launches_timed": n_, "pairs": tag_[1],
                            "note": "HIP events on the stream the merge runs on (the tail stream: overlaps the next step's encoder)"}
    rs = getattr(backend, "refine_stats", None)
    if "merge_refine" in kernels and rs is not None:
        worst = ops.refine_max_error(rs)
        smp_err, smp_n = ops.refine_sample_error(rs)
        cnt = ops.refine_counts(rs)
        n_q = (Tc - 1) * HW if a.mode == "video" and world == 1 else None
        kernels["merge_refine"].update(**cnt, queries=n_q, eps=cfg.pair_refine_eps, max_pair_score_error_seen=worst,
                                       max_pair_score_error_unbiased_sample=smp_err, unbiased_sample_entries=smp_n)
        if worst > cfg.pair_refine_eps:
            raise SystemExit(f"bench.py: the pair kernel's score error reached {worst:.2e}, beyond the bound {cfg.pair_refine_eps:.2e} the exact re-scoring assumes")
    head = kernels.get("encoder_conv") or kernels.get("pair_topk")
    roofline = {k: head[k] for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "what", "executed_tflops",
                                     "frac_executed", "frac_of_f32_mfma_peak", "sustained_peak", "frac_executed_of_sustained", "sustained_note", "ms_per_launch", "mfma_util", "launch_note", "pmc_note")
                if k in head} if head else None
    _out = ('C', 'HW', 'Hf', 'Wf', 'kernels', 'n_', 'n_pairs_clip', 'name', 'pm', 'roofline')
    L.update({k_: v_ for k_, v_ in locals().items() if k_ in _out})


def assemble_record(L):
    """the JSON line's fixed part: metric, value, config, distributed, sharding phases.  `L`: the run's namespace (main() threads one dict through the phases)."""
    C, HW, Hf, P, T, Tc, Wf, _, a, arith, backend, backend_name = L.get("C"), L.get("HW"), L.get("Hf"), L.get("P"), L.get("T"), L.get("Tc"), L.get("Wf"), L.get("_"), L.get("a"), L.get("arith"), L.get("backend"), L.get("backend_name")
    cfg, comm, dev, e_lo, elapsed, engine, fdist, h, hi, kernels, lo, local = L.get("cfg"), L.get("comm"), L.get("dev"), L.get("e_lo"), L.get("elapsed"), L.get("engine"), L.get("fdist"), L.get("h"), L.get("hi"), L.get("kernels"), L.get("lo"), L.get("local")
    lat = L.get("lat")
    n_, n_frames_total, n_pairs_clip, pair_fmt, rank, rep, roofline, timing, w, wl, world = L.get("n_"), L.get("n_frames_total"), L.get("n_pairs_clip"), L.get("pair_fmt"), L.get("rank"), L.get("rep"), L.get("roofline"), L.get("timing"), L.get("w"), L.get("wl"), L.get("world")
    out = {
        "metric": "frames/sec + ms/corr-volume, 480p 8-frame clip, 1/2/4/8 MI355X",
        "value": n_frames_total / elapsed, "unit": "frames/s",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": elapsed / a.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f16 + fp6 (e2m3) MFMA operands, f32 accumulate; top-k near-ties re-scored in f64 from f32 features" if cfg.bank_fmt == "f16f6x" else
                 ("MFMA operands: encoder " + arith + ", correlation " + {"f16": "f16 h/l x3", "f16f6": "f16 + FP6 cross terms (no re-scoring)"}[pair_fmt] + "; f32 accumulate"),
        "parity": {"f16f6x": "top-10 lists = the reference's own on every list whose float64 ranks are 3e-5 apart, over all 16 384 queries of two fixtures; on 99.91 % of those 1e-5 apart (the encoder's error decides 14 of 16 285: profiles/r06_precision_ledger_all_queries.json)",
                   "f16f6": "round 4's arithmetic: lists exact only where float64 ranks are 1e-4 apart",
                   "f16": "three f16 products per f32-grade product: lists exact at 1e-5"}[cfg.bank_fmt],
        "data": "synthetic",
        "config": {"workload": (f"{a.workload}: one {T}x{h}x{w} video per step = {world} clip(s) of {Tc} frames, one per rank -> {Hf}x{Wf}x{C} "
                                f"features, top-10, radius 15, tau 0.07, P={P}" if a.mode == "video" else
                                f"{a.workload}: {Tc}x{h}x{w} clip -> {Hf}x{Wf}x{C} features, {n_pairs_clip} unique (query,key) pairs, top-10, "
                                f"radius 15, tau 0.07, P={P}, one independent clip per rank per step"),
                   "parallelism": (f"clip-sharded video over {world} rank(s): RCCL broadcast of first-frame features, point-to-point "
                                   f"{cfg.precede_frames}-frame halo ({a.halo}), all_gather of merged top-k lists, replicated sweep"
                                   if a.mode == "video" else f"dp{world} (independent clips per rank, no data-path collective)")},
        "timed_seconds": elapsed,
        "single_step_latency_ms": (round(sorted(lat)[len(lat) // 2], 4) if lat else None),
        "steps_overlap": (None if a.sync_tail else
                          {"pairs": "each step's pair top-k, merge and sweep run on a side stream under the NEXT step's encoder (HipBackend(tail_from='pairs')); "
                                    "all K steps are complete before the closing barrier; single_step_latency_ms is one step alone",
                           "sweep": "each step's merge and sweep run on a side stream under the next step's encoder"}[a.tail_from]),
        "repeat_ms_per_step": rep,
        "roofline": roofline,
        "kernels": kernels,
        "encoder_arith": arith,
        "pair_arith": pair_fmt,
    }
    if a.mode == "video":
        rr = fdist.shard_frames(T, world, first=1)
        out["config"]["query_frames_per_rank"] = [hi_ - lo_ for lo_, hi_ in rr]
        out["config"]["pairs_per_rank"] = [len(engine.plan_clip(T, [0], cfg, frame_range=r_).pairs) for r_ in rr]
        out["config"]["pairs_note"] = ("unique (query frame, key frame) pairs: frame t of a video has min(t, 6) key frames (frame 0 + the 5 "
                                       "before it), so every rank after the first carries 6 per frame where an 8-frame clip has 27 in all -- "
                                       "per-GPU frames are fixed as N grows (weak scaling), per-GPU pair work grows from 27 to 48")
    if world > 1:
        # what the communication library saw (so that a reader of the line can check it was a real N-rank RCCL job)
        try:
            rccl = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl = None
        devs = [None] * world
        dist.all_gather_object(devs, (rank, local, torch.cuda.get_device_properties(dev).name, str(torch.cuda.get_device_properties(dev).uuid)
                                      if hasattr(torch.cuda.get_device_properties(dev), "uuid") else None))
        out["distributed"] = {"world_size": dist.get_world_size(), "backend": backend_name, "rccl_version": rccl,
                              "ranks": [dict(rank=r_, local_rank=l_, device=n_, uuid=u_) for r_, l_, n_, u_ in devs],
                              "distinct_devices": len({u_ for _, _, _, u_ in devs if u_}) or None,
                              "early_halo": bool(getattr(backend, "early_halo", False)), "comm_timeout_s": a.comm_timeout}
    else:
        try:
            rccl1 = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            rccl1 = None
        out["distributed"] = {"world_size": 1, "backend": None, "rccl_version": rccl1,
                              "note": "one process, no process group: the sharded driver runs without any collective"}
    if a.rehearse_on_one_gpu:
        out["rehearsal"] = (f"{world} ranks on ONE GPU over gloo, device tensors staged through the host: a functional rehearsal of the "
                            "multi-rank path, not a measurement")
    if a.mode == "video":
        torch.cuda.synchronize()
        ph = timing.report()
        out["sharding_ms_per_step"] = {k: v / a.steps for k, v in ph.items()}
        enc_ms = ph.get("encode", 0.0) / a.steps
        if enc_ms > 0:
            n_enc = (hi - e_lo) if a.halo == "exchange" or world == 1 else (hi - max(0, lo - cfg.precede_frames))
            efl = encoder_flops(wl, n_enc)
            kernels["encoder_phase"] = {
                "what": "the whole trunk on rank 0 (stem, 3x3 / 1x1 / stride-2 convolutions on both stream lanes, normalise + split): "
                        "ALGORITHMIC f32 FLOPs of its convolutions / the encode phase's HIP-event time",
                "frames": n_enc, "ms": enc_ms, "bound": "mfma", "achieved": efl / (enc_ms * 1e-3) / 1e12, "peak": BF16_MFMA_PEAK_TFLOPS,
                "unit": "TFLOP/s", "frac": efl / (enc_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                "executed_note": "layers 2-3 (80 % of the FLOPs) in `arith`, stem / layer 1 / stride-2 convolutions in bf16x3: priced at 3 units",
                "executed_tflops": 3.0 * efl / (enc_ms * 1e-3) / 1e12,
                "frac_executed": 3.0 * efl / (enc_ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS,
                "frac_of_f32_mfma_peak": efl / (enc_ms * 1e-3) / 1e12 / F32_MFMA_PEAK_TFLOPS}
        out["sharding_note"] = ("HIP-event time per phase on rank 0's main stream (the sweep runs on a side stream and overlaps the next "
                                "step's encoder; at N = 1 broadcast / halo / all_gather are skipped)")

    if a.mode == "video":
        # what this rank handed to the exchange steps per step, against the schedule's arithmetic (N = 1: nothing moves)
        frame_bytes = HW * C * 4                                           # one frame ON THE WIRE: 1 KiB per pixel (f32 or 2 x 16-bit parts; of split_f16f6x() rows only the f32 half travels)
        list_bytes = HW * cfg.topk * 8                                      # idx int32 + weight f32 of one frame's merged list
        rr = fdist.shard_frames(T, world, first=1)
        exp = {"broadcast": frame_bytes if world > 1 else 0,
               "halo_recv": (min(cfg.precede_frames, lo - 1) * frame_bytes if (world > 1 and a.halo == "exchange" and rank > 0) else 0),
               "all_gather_send": (max(hi_ - lo_ for lo_, hi_ in rr) * list_bytes if world > 1 else 0)}
        out["comm_bytes_per_step_rank0"] = dict(comm, expected=exp, frame_bytes=frame_bytes, list_bytes_per_frame=list_bytes)
        for k_, v_ in exp.items():
            assert abs(comm[k_] - v_) <= 1e-6 * max(v_, 1), (k_, comm[k_], v_)
    _out = ('out',)
    L.update({k_: v_ for k_, v_ in locals().items() if k_ in _out})


def clips_line(L):
    """the same ranks on independent clips (no collective): what the exchange steps cost.  `L`: the run's namespace (main() threads one dict through the phases)."""
    Tc, _, a, barrier, cfg, dev, engine, h, model, n_pairs_clip, out, plan1 = L.get("Tc"), L.get("_"), L.get("a"), L.get("barrier"), L.get("cfg"), L.get("dev"), L.get("engine"), L.get("h"), L.get("model"), L.get("n_pairs_clip"), L.get("out"), L.get("plan1")
    pts, rank, t1, tail_stream, w, world = L.get("pts"), L.get("rank"), L.get("t1"), L.get("tail_stream"), L.get("w"), L.get("world")
    if a.mode == "video" and not a.no_clips_line:
        # the reference's own data parallelism on the same clips (`--mode clips`: independent 8-frame clips per rank, no data-path
        # collective), measured right here: separates "cost of the exchange steps" from "a longer video has more pairs per frame"
        x_c = torch.randn(Tc, 3, h, w, generator=torch.Generator().manual_seed(2000 + rank)).to(dev)      # this rank's own clip

        def step_clips():
            feats, Hf_, Wf_ = model.get_feats_hwc(x_c, split=True)
            pl = engine.run_pairs(feats, Hf_, Wf_, plan1, cfg)
            if tail_stream is None:
                return engine.run_propagation(engine.merge_pairs(pl, cfg), 0, pts, Hf_, Wf_, h, w, cfg)[1]
            return engine.run_propagation_async(pl, 0, pts, Hf_, Wf_, h, w, cfg, tail_stream)[1]
        for _ in range(5):
            step_clips()
        barrier()
        t1 = time.perf_counter()
        n_c = max(20, a.steps // 2)
        for _ in range(n_c):
            step_clips()
        barrier()
        el_c = time.perf_counter() - t1
        if world > 1:
            tc_ = torch.tensor([el_c], device=dev, dtype=torch.float64)
            dist.all_reduce(tc_, op=dist.ReduceOp.MAX)
            el_c = float(tc_.item())
        out["clips_mode"] = {"what": "the same ranks running INDEPENDENT 8-frame clips (the reference's video-level data parallelism: no broadcast, "
                                     "no halo, no all_gather), timed the same way right after the sharded-video steps",
                             "value": world * Tc * n_c / el_c, "unit": "frames/s", "ms_per_step": el_c / n_c * 1e3, "steps": n_c,
                             "pairs_per_rank": n_pairs_clip}
    _out = ('_', 't1')
    L.update({k_: v_ for k_, v_ in locals().items() if k_ in _out})


def precision_lines(L):
    """the same steps in the three-f16-product form and without the refining merge.  `L`: the run's namespace (main() threads one dict through the phases)."""
    T, _, a, arith, backend, barrier, cfg, dev, fdist, model, out, out_coords = L.get("T"), L.get("_"), L.get("a"), L.get("arith"), L.get("backend"), L.get("barrier"), L.get("cfg"), L.get("dev"), L.get("fdist"), L.get("model"), L.get("out"), L.get("out_coords")
    pair_fmt, qp, rgbs, t1, world = L.get("pair_fmt"), L.get("qp"), L.get("rgbs"), L.get("t1"), L.get("world")
    if a.mode == "video" and not a.no_f16x3_line and (arith != "f16x3" or pair_fmt != "f16"):
        # the price of precision, on the driver's record: the same steps with every matrix product in the three-f16-product form
        # (22 significand bits per operand: encoder f16x3 + fgvc_pair_topk_f16x3), timed the same way right here
        model.backbone.set_arith("f16x3")
        model.test_cfg["pair_split_fmt"] = "f16"
        cfg3 = model.engine_config()
        cfg3.pair_precision, cfg3.regroup = cfg.pair_precision, False
        cache3 = {}

        def step3():
            return fdist.track_points_sharded(backend, rgbs, qp, cfg3, device=dev, halo=a.halo, timing=None, cache=cache3, check=False)[0]
        for _ in range(5):
            step3()
        barrier()
        t1 = time.perf_counter()
        n3 = max(20, a.steps // 2)
        for _ in range(n3):
            out3 = step3()
        barrier()
        el3 = time.perf_counter() - t1
        if world > 1:
            t3_ = torch.tensor([el3], device=dev, dtype=torch.float64)
            dist.all_reduce(t3_, op=dist.ReduceOp.MAX)
            el3 = float(t3_.item())
        assert bool(torch.isfinite(out3).all())
        out["value_f16x3"] = {"what": "the same sharded-video steps with the encoder in f16x3 and the pair kernel fgvc_pair_topk_f16x3 (three f16 products "
                                      "per f32-grade product everywhere: the form closest to the reference's fp32)",
                              "value": T * n3 / el3, "unit": "frames/s", "ms_per_step": el3 / n3 * 1e3, "steps": n3,
                              "traj_diff_px_vs_default": (lambda d: {"median": float(d.median()), "within_0.01px": float((d < 0.01).double().mean()),
                                                                     "within_0.5px": float((d < 0.5).double().mean()), "max": float(d.max()),
                                                                     "note": "per (frame, point) read-out on the bench's clip of seeded NOISE frames through a random-"
                                                                             "weight encoder: label maps there are nearly flat, and a near-tie at the top-5 boundary "
                                                                             "of the soft-argmax (discontinuous: vanilla_tracker.py:181) moves a read-out by pixels; on "
                                                                             "the reference's fixtures every arithmetic stays within 3.1e-5 px "
                                                                             "(profiles/r05_precision_ledger.json)"})(
                                  (out3.to(torch.float64) - out_coords.to(torch.float64)).abs().amax(-1).flatten())}
        model.backbone.set_arith(arith)
        if a.pair_fmt != "auto":
            model.test_cfg["pair_split_fmt"] = a.pair_fmt
        else:
            model.test_cfg.pop("pair_split_fmt", None)
    if a.mode == "video" and not a.no_f16x3_line and cfg.bank_fmt == "f16f6x":
        # ... and round 4's arithmetic (the f16 + FP6 pair kernel WITHOUT the refining merge, 1 KiB bank rows): what exactness costs
        model.test_cfg["pair_refine"] = False
        cfg4 = model.engine_config()
        cfg4.pair_precision, cfg4.regroup = cfg.pair_precision, False
        cache4 = {}
        for _ in range(5):
            fdist.track_points_sharded(backend, rgbs, qp, cfg4, device=dev, halo=a.halo, timing=None, cache=cache4, check=False)
        barrier()
        t1 = time.perf_counter()
        n4 = max(20, a.steps // 2)
        for _ in range(n4):
            fdist.track_points_sharded(backend, rgbs, qp, cfg4, device=dev, halo=a.halo, timing=None, cache=cache4, check=False)
        barrier()
        el4 = time.perf_counter() - t1
        if world > 1:
            t4_ = torch.tensor([el4], device=dev, dtype=torch.float64)
            dist.all_reduce(t4_, op=dist.ReduceOp.MAX)
            el4 = float(t4_.item())
        out["value_unrefined"] = {"what": "the same steps without the refining merge (pair_refine = False: round 4's default, lists exact at 1e-4 only)",
                                  "value": T * n4 / el4, "unit": "frames/s", "ms_per_step": el4 / n4 * 1e3, "steps": n4}
        model.test_cfg.pop("pair_refine")
    _out = ('_',)
    L.update({k_: v_ for k_, v_ in locals().items() if k_ in _out})


def corr_volume_section(L):
    """ms/corr-volume: the dense volume kernels round-robin, the store stream by itself.  `L`: the run's namespace (main() threads one dict through the phases)."""
    C, HW, _, _lib, a, dev, name, ops, out, pm, rank = L.get("C"), L.get("HW"), L.get("_"), L.get("_lib"), L.get("a"), L.get("dev"), L.get("name"), L.get("ops"), L.get("out"), L.get("pm"), L.get("rank")
    if rank == 0 and not a.no_corr_volume:
        gq = torch.Generator(device=dev).manual_seed(5)
        feats2 = torch.nn.functional.normalize(torch.randn(2, HW, C, generator=gq, device=dev), dim=2)
        vol = torch.empty((HW, HW), device=dev, dtype=torch.float32)
        gbytes = (HW * HW * 4 + 2 * HW * C * 4) / 1e9                  # volume write + both inputs (f32-sized)
        hl, sp, sp6 = ops.split_bf16(feats2), ops.split_f16f8(feats2), ops.split_f16f6(feats2)
        fns = {"f16f6": lambda: ops.corr_volume(sp6[1], sp6[0], 0.07, "f16f6", out=vol),
               "f16f8": lambda: ops.corr_volume(sp[1], sp[0], 0.07, "f16f8", out=vol),
               "bf16x3": lambda: ops.corr_volume(hl[1], hl[0], 0.07, "bf16x3", out=vol),
               "f32": lambda: ops.corr_volume(feats2[1], feats2[0], 0.07, "f32", out=vol),
               "bf16": lambda: ops.corr_volume(hl[1], hl[0], 0.07, "bf16", out=vol)}
        res = {k: [] for k in fns}
        for rnd in range(7):                                           # round-robin: the first kernel timed in a process runs slow;
            for name, fn in fns.items():                               # round 0 is dropped, the MEDIAN of the other six is reported
                fn()
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(10)]
                for e0, e1 in evs:
                    e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rnd:
                    res[name].append(sum(e0.elapsed_time(e1) for e0, e1 in evs) / len(evs))
        med = lambda v: sorted(v)[len(v) // 2]
        # the write stream by itself, measured HERE: (a) the kernel's own store sequence replayed without its loads
        # and multiplies (same grid, row classes, lane swap, barriers; zeros written), (b) a linear sweep of 16-byte stores over the same bytes
        def timed(fn, n=10, rounds=5):
            out_ms = []
            for _ in range(rounds):
                fn()
                evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
                for e0, e1 in evs:
                    e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                out_ms.append(sum(e0.elapsed_time(e1) for e0, e1 in evs) / n)
            return med(out_ms[1:])
        try:                                   # (a results-wrong switch: only the experiment build of the library takes it)
            with _lib.ablations():
                ops.set_option("corr6_debug", 1024)
                try:
                    replay_ms = timed(fns["f16f6"])
                finally:
                    ops.set_option("corr6_debug", 0)
        except _lib.FgvcHipError:
            replay_ms = None
        nfl = (HW * HW // 4) * 4
        sweep_ms = {nt: timed(lambda nt=nt: _lib.call("fgvc_debug_store_sweep_f32", ops._ptr(vol), nfl, nt, ops._stream(vol))) for nt in (0, 1)}
        vol_bytes = HW * HW * 4 / 1e9
        var = {k: {"ms": med(v), "ms_min": min(v), "ms_max": max(v), "rounds": len(v), "achieved": gbytes / (med(v) * 1e-3),
                   "frac": gbytes / (med(v) * 1e-3) / HBM_PEAK_GBPS} for k, v in res.items()}
        var["f16f6"]["max_abs_err_bound"] = "1e-3 logit (tests); measured 6e-5 on Gaussian rows, 8e-5 against bf16x3 at 720p"
        var["f16f8"]["max_abs_err_bound"] = "1e-3 logit (tests); measured 4e-5 on Gaussian rows, 8e-5 against bf16x3 at 720p"
        var["bf16x3"]["max_abs_err_bound"] = "1e-3 logit (tests); measured 2e-5"
        var["bf16"]["max_abs_err_bound"] = "3e-2 logit (reduced precision: reported, not parity-grade)"
        pm = pmc("fgvc_corr_volume_f16f6")
        out["corr_volume"] = {
            "what": f"dense materialised ({HW}x{HW}) f32 volume for one (query,key) frame pair.  f16f6 / f16f8 (f16 main product + "
                    "block-scaled FP6 / FP8 cross terms) and bf16x3 meet the 1e-3 score bar, f32 is exact, plain bf16 is reduced precision",
            "ms_per_corr_volume": var["f16f6"]["ms"],
            "roofline": {"kernel": "fgvc_corr_volume_f16f6", "bound": "hbm", "achieved": var["f16f6"]["achieved"],
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": var["f16f6"]["frac"],
                         "ceiling_gbps": STORE_CEILING_GBPS, "ceiling_frac": var["f16f6"]["achieved"] / STORE_CEILING_GBPS,
                         "write_rate_ceiling_note": "dword stores over 2.64 GB: profiles/r03_store_footprint.log; measured live: store_replay / store_sweep",
                         "store_replay_ms": replay_ms, "store_replay_gbps": (vol_bytes / (replay_ms * 1e-3)) if replay_ms else None,
                         "store_sweep_ms": sweep_ms[0], "store_sweep_gbps": vol_bytes / (sweep_ms[0] * 1e-3),
                         "store_sweep_nt_gbps": vol_bytes / (sweep_ms[1] * 1e-3),
                         "traffic": pm.get("hbm_bytes_per_launch"), "mfma_util": pm.get("mfma_util"),
                         "bytes_per_launch": gbytes * 1e9,
                         "note": "median of 6 rounds x 10 launches (HIP events), round-robin with the other variants, first round dropped"},
            "variants": var,
        }
        if out.get("roofline") is not None:      # the second half of BASELINE's metric, where the driver's record keeps it
            out["roofline"].update(corr_volume_kernel="fgvc_corr_volume_f16f6", ms_per_corr_volume=var["f16f6"]["ms"],
                                   corr_volume_frac=var["f16f6"]["frac"], corr_volume_gbps=var["f16f6"]["achieved"],
                                   corr_volume_traffic=pm.get("hbm_bytes_per_launch"), corr_volume_peak_gbps=HBM_PEAK_GBPS,
                                   store_ceiling_gbps=vol_bytes / (min(sweep_ms.values()) * 1e-3),
                                   corr_volume_store_replay_gbps=(vol_bytes / (replay_ms * 1e-3)) if replay_ms else None)
        del vol


def main():
    a = parse_args()

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: this process (which has not touched the GPU and never will) starts the N ranks with the
        # reference's launcher shape (tools/dist_test.sh:10-13: torch.distributed.launch --nproc_per_node) and hands on their exit code
        raise SystemExit(self_launch(a.gpus))
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus != world:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: launch one process per GPU "
                         f"(python -m torch.distributed.run --nproc-per-node {a.gpus} ... bench.py --gpus {a.gpus})")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    if a.rehearse_on_one_gpu:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    backend_name = None
    if world > 1:
        import datetime
        # every collective is bounded: a rank that hangs in one makes the job exit non-zero (the process group's watchdog aborts
        # the communicator and raises) instead of sitting at the closing barrier for ever
        tmo = datetime.timedelta(seconds=a.comm_timeout)
        if a.rehearse_on_one_gpu:
            os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
            dist.init_process_group("gloo", timeout=tmo)
        else:
            os.environ.setdefault("TORCH_NCCL_ASYNC_ERROR_HANDLING", "1")
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)      # RCCL over xGMI
        backend_name = dist.get_backend()

    from fgvc_amd import _lib, dist as fdist, engine, ops
    _lib.load()
    L = dict(locals())                                               # the run's namespace: every phase reads what it needs from it and adds what later ones need
    setup_workload(L)
    timed_steps(L)
    roofline_objects(L)
    assemble_record(L)
    if a.full:                                                       # what the headline figure does not need: runs of their own
        clips_line(L)
        precision_lines(L)
        corr_volume_section(L)
    a, halo_why, out, rank, wl, world = L.get("a"), L.get("halo_why"), L.get("out"), L.get("rank"), L.get("wl"), L.get("world")
    if a.full and rank == 0 and world == 1 and not a.no_cpu_baseline:          # reported at N = 1 only (the other ranks would sit at the barrier)
        out["cpu_baseline"] = cpu_baseline(wl)
    if halo_why is not None:
        out["halo_auto"] = {"mode": halo_why["mode"], "link_gbps": halo_why["link_gbps"],
                            "worst_boundary": max(halo_why["boundaries"], key=lambda d: d["exposed_s"]) if halo_why["boundaries"] else None}
    _driver_view(out)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


ROOFLINE_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "executed_tflops", "frac_executed", "sustained_peak",
                 "frac_executed_of_sustained", "ms_per_launch", "mfma_util", "corr_volume_kernel", "ms_per_corr_volume", "corr_volume_frac",
                 "corr_volume_gbps", "corr_volume_traffic", "corr_volume_store_replay_gbps")


def _driver_view(out):
    """The driver's record keeps 24 scalar keys of `roofline`: numbers only (the prose moves to `roofline_notes`), plus what the review
    asked to see there -- the three-f16-product figure, the pair kernel's own time and fraction, the spread of the step over the repeat
    blocks -- and in `config` what tells a real N-rank RCCL job from N ranks on one device."""
    r = out.get("roofline")
    if r is not None:
        new = {k: r[k] for k in ROOFLINE_KEYS if k in r}
        v3 = out.get("value_f16x3")
        new["value_f16x3"] = v3.get("value") if isinstance(v3, dict) else None
        pk = (out.get("kernels") or {}).get("pair_topk") or {}
        new["pair_topk_ms"], new["pair_topk_frac"] = pk.get("ms_per_launch"), pk.get("frac")
        blocks = [m for m in (out.get("repeat_ms_per_step") or []) if m] + [out["ms_per_step"]]
        new["step_ms_min"], new["step_ms_max"] = min(blocks), max(blocks)
        assert len(new) <= 24, len(new)
        out["roofline_notes"] = {k: v for k, v in r.items() if k not in new}
        out["roofline"] = new
    # (what the timed region overlaps, and one step alone, where the driver keeps them)
    out.setdefault("config", {}).update(steps_overlap=("next step's encoder under this step's pair top-k, merge and sweep (side stream); all steps "
                                                       "complete before the closing barrier" if out.get("steps_overlap") and "pair top-k" in out["steps_overlap"]
                                                       else "next step's encoder under this step's merge and sweep" if out.get("steps_overlap") else "none"),
                                        single_step_latency_ms=out.get("single_step_latency_ms"))
    d = out.get("distributed") or {}
    out.setdefault("config", {}).update(world_size=d.get("world_size"), distinct_devices=d.get("distinct_devices", 1 if d.get("world_size") == 1 else None),
                                        rccl_version=d.get("rccl_version"), backend=d.get("backend"))


if __name__ == "__main__":
    main()
