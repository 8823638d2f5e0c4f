"""GPU tests of the soft-map output (test_cfg.return_maps=True: the propagated maps themselves, (T, K, h0, w0), the reference's
coords=False return value, vanilla_tracker.py:770-784, :800-803): the read-out kernel against a float64 torch restatement, its bit
identity with the coordinate read-out, the engine's whole clip (dense and local window) against a restatement driven by the same top-k
lists, the tracker API against the reference's own output (tests/golden/softmap_*.npz, hr_softmap_*.npz,
tests/golden/gen_golden_softmap.py), the chunked host-bound read-out, and tools/test.py --pose-form softmap end to end.

Bounds (derived, none fitted to the kernel's output):
  read-out, frame f >= 1, per (frame, map): a value combines at most 16 bank values with f32 weights that sum to 1; products, weight
    products and the fmaf chain each round once: 64 * 2^-24 * Mb, Mb = max|bank[f, :, k]|.  The source coordinate scale * (o + 0.5) - 0.5
    is evaluated in f32 (PyTorch's own arithmetic for f32 input) and is as large as the input size, so it carries up to 2^-23 * n of
    rounding, which moves a bilinear weight by that and the value by that times the difference of two neighbouring samples; four such
    coordinates enter a value: 4 * 2^-23 * max(hp, wp) * D, D = the largest difference of adjacent bank values of that (frame, map).
  read-out, frame 0: f32 map against F.interpolate in float32: 2 f32 ulps of the value + 2 * 2^-23 * max(hp, wp) * D0 (D0 from the padded
    map); f64 map against F.interpolate in float64: 4 f64 ulps of max|map|, plus one f32 rounding (half an f32 ulp of the value) for an f32
    output.
  model call, frame f >= 1: the project's score bar is delta = 1e-3 logit; a logit error of delta changes a softmax weight by at most
    2 delta relatively and a propagated value is a convex combination of earlier values: atol(f) = 2 * delta * f * M, M = max|ref_seg_map|.
    A top-k list that flips at a near tie exchanges candidates of rank >= topk, whose weight is at most 1 / topk: at most 1 % of a
    fixture's values above atol(f), none above atol(f) + f * M / topk.
  coordinates decoded from the maps against the coordinate read-out, clear maps ((5th - 6th) / max > 1e-5): 1e-9 px for an f64 stack (the
    same five values, five products summed in f64), plus 4 f32 ulps of the largest coordinate for an f32 stack (one rounding of the top-5
    sum moves every weight)."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAR = 1e-5
TOL_DECODE_PX = 1e-9
TOL_F32_ULPS = 4
DELTA = 1e-3
SHARE_CAP = 0.01


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tol_decode(f64: bool, out_shape) -> float:
    return TOL_DECODE_PX if f64 else TOL_DECODE_PX + TOL_F32_ULPS * 2.0 ** -24 * max(out_shape)


def _ulp32(x: torch.Tensor) -> torch.Tensor:
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


# ---- float64 restatement (torch) ---------------------------------------------------------------------------------------------------
def later_restated(bank, Hf, Wf, hw_map, map_pad, out_shape):
    """Frames 1.. of the stack in float64: bilinear(bank[f] -> padded size), unpad, bilinear(-> out_shape) (:770-784).  bank (T, HfWf, K)."""
    hm, wm = hw_map
    lw, uw, lh, uh = map_pad
    hp, wp = hm + lh + uh, wm + lw + uw
    T, _, K = bank.shape
    x = bank[1:].double().reshape(T - 1, Hf, Wf, K).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=(hp, wp), mode="bilinear", align_corners=False)[:, :, lh:hp - uh, lw:wp - uw]
    return F.interpolate(x, size=tuple(out_shape), mode="bilinear", align_corners=False)


def frame0_restated(heat, map_pad, out_shape):
    """Frame 0: bilinear(padded heat -> out_shape) in heat's dtype, NOT unpadded (:712-716)."""
    return F.interpolate(F.pad(heat[None], map_pad), size=tuple(out_shape), mode="bilinear", align_corners=False)[0]


def _adjacent(x: torch.Tensor) -> torch.Tensor:
    """x (..., H, W) -> (...) the largest |difference| of horizontally or vertically adjacent values."""
    dv = (x[..., 1:, :] - x[..., :-1, :]).abs().flatten(-2).amax(-1) if x.shape[-2] > 1 else torch.zeros(x.shape[:-2], device=x.device)
    dh = (x[..., :, 1:] - x[..., :, :-1]).abs().flatten(-2).amax(-1) if x.shape[-1] > 1 else torch.zeros(x.shape[:-2], device=x.device)
    return torch.maximum(dv, dh)


def later_bound(bank, Hf, Wf, hw_map, map_pad):
    """(T - 1, K) float64: the derived bound of frames 1.. per (frame, map), from the bank alone."""
    hm, wm = hw_map
    lw, uw, lh, uh = map_pad
    n = max(hm + lh + uh, wm + lw + uw)
    T, _, K = bank.shape
    g = bank[1:].double().reshape(T - 1, Hf, Wf, K).permute(0, 3, 1, 2)
    return 64 * 2.0 ** -24 * g.abs().flatten(-2).amax(-1) + 4 * 2.0 ** -23 * n * _adjacent(g)


def frame0_check(got0, heat, map_pad, out_shape, out_f32: bool, want=None):
    """got0 (K, h0, w0) against `want` (default: frame0_restated, PyTorch's own interpolation in the map's dtype) under the frame-0 bound;
    returns (largest error, largest bound) for the report."""
    want = (frame0_restated(heat, map_pad, out_shape) if want is None else want).double()
    err = (got0.double() - want).abs()
    if heat.dtype == torch.float32:
        hp, wp = heat.shape[1] + map_pad[2] + map_pad[3], heat.shape[2] + map_pad[0] + map_pad[1]
        d0 = _adjacent(F.pad(heat, map_pad).double())[:, None, None]
        bound = 2 * _ulp32(want) + 2 * 2.0 ** -23 * max(hp, wp) * d0
    else:
        m = float(heat.abs().max())
        bound = torch.full_like(want, 4 * float(np.spacing(np.float64(m))))
        if out_f32:
            bound = bound + 0.5 * _ulp32(want)          # one rounding to f32: half an ulp
    assert bool((err <= bound).all()), (float(err.max()), float(bound.max()))
    return float(err.max()), float(bound.max())


def decode(maps: torch.Tensor):
    """img2coord (:172-191) of (T, K, h0, w0) maps in their own dtype, the kernels' tie rule (a stable ascending sort puts the higher flat
    index last).  Returns (coords (2, K, T), gap (T, K) = (5th - 6th) / max)."""
    T, K, h0, w0 = maps.shape
    flat = maps.reshape(T, K, -1)
    srt, idx = torch.sort(flat, dim=-1, stable=True)
    top_i, top_v = idx[..., -5:].cpu().numpy(), srt[..., -5:].cpu().numpy()
    v = top_v / (np.sum(top_v, axis=-1, keepdims=True) + top_v.dtype.type(1e-9))
    coords = np.zeros((2, K, T))
    coords[0] = np.sum((top_i % w0) * v, axis=-1).T
    coords[1] = np.sum((top_i // w0) * v, axis=-1).T
    coords[:, (flat.double().sum(-1) == 0).cpu().numpy().T] = -1
    s6 = srt[..., -6:].double()
    gap = ((s6[..., 1] - s6[..., 0]) / s6[..., -1].abs().clamp_min(1e-300)).cpu().numpy()
    return coords, gap


def heat_maps(K, hm, wm, sigma, rng, dtype=torch.float64):
    yy, xx = np.mgrid[0:hm, 0:wm]
    out = np.zeros((K, hm, wm))
    for k in range(K):
        cy, cx = rng.uniform(0, hm - 1), rng.uniform(0, wm - 1)
        out[k] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    return torch.from_numpy(out).to(dtype)


def bank_rows(T, Hf, Wf, K, rng):
    """(T, HfWf, K) f32 propagated-like labels: one smooth bump per channel per frame; channel 0 all zero, channel 1 a plateau (a flat
    top wider than 5 pixels), channel 2 with negative values."""
    yy, xx = np.mgrid[0:Hf, 0:Wf]
    b = np.zeros((T, Hf, Wf, K))
    for t in range(T):
        for k in range(K):
            cy, cx = rng.uniform(0, Hf - 1), rng.uniform(0, Wf - 1)
            s = rng.uniform(1.5, 4.0)
            b[t, :, :, k] = rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    b[:, :, :, 0] = 0.0
    b[:, :, :, 1] = np.minimum(b[:, :, :, 1], 0.5 * b[:, :, :, 1].max(axis=(1, 2), keepdims=True))
    b[:, :, :, 2] = b[:, :, :, 2] - 0.3
    return torch.from_numpy(b.reshape(T, Hf * Wf, K)).float()


# ---- the read-out kernel ------------------------------------------------------------------------------------------------------------
READOUT_CASES = [
    # (T, K, (hm, wm), d, (Hf, Wf), (h0, w0), heat dtype): the cases of the coordinate read-out's test
    (8, 16, (480, 854), 2, (240, 427), (480, 854), torch.float32),       # DAVIS size, K = 16
    (8, 16, (480, 854), 2, (240, 427), (480, 854), torch.float64),
    (6, 15, (320, 320), 2, (160, 160), (240, 320), torch.float64),       # JHMDB: network 320 x 320, maps at the video's 240 x 320
    (5, 20, (320, 512), 2, (160, 256), (320, 512), torch.float64),       # BADJA: at the network size
    (4, 6, (41, 47), 2, (21, 24), (45, 52), torch.float32),              # padded map, original_shape != map size
    (4, 6, (41, 47), 2, (21, 24), (45, 52), torch.float64),
]
CASE_ID = lambda c: f"T{c[0]}K{c[1]}_{c[2][0]}x{c[2][1]}_to_{c[5][0]}x{c[5][1]}_{str(c[6])[-7:]}"


def _readout_case(case, seed):
    from fgvc_amd import engine
    T, K, (hm, wm), d, (Hf, Wf), out_shape, dtype = case
    rng = np.random.default_rng(seed)
    heat = heat_maps(K, hm, wm, 4.0, rng, dtype)
    heat[0] = 0                                        # all-zero map
    heat[1] = heat[1].clamp_max(0.6)                   # flat top: a plateau
    heat[2] = heat[2] - 0.25                           # negative values
    _, map_pad = engine.pad_divide_by(hm, wm, d)
    return heat, bank_rows(T, Hf, Wf, K, rng), map_pad, Hf, Wf, out_shape


@pytest.mark.parametrize("case", READOUT_CASES, ids=CASE_ID)
def test_readout_matches_float64_restatement(dev, case):
    from fgvc_amd import ops
    heat, bank, map_pad, Hf, Wf, out_shape = _readout_case(case, 7)
    T, K = bank.shape[0], heat.shape[0]
    heat_d, bank_d = heat.to(dev), bank.to(dev)
    want = later_restated(bank_d, Hf, Wf, heat.shape[1:], map_pad, out_shape)
    bound = later_bound(bank_d, Hf, Wf, heat.shape[1:], map_pad)
    got = {}
    for dt in (torch.float32, torch.float64):
        g = got[dt] = ops.softmap_readout(bank_d, heat_d, Hf, Wf, map_pad, out_shape, out_dtype=dt)
        assert g.shape == (T, K, *out_shape) and g.dtype == dt and g.is_contiguous()
        err = (g[1:].double() - want).abs().flatten(-2).amax(-1)                    # (T - 1, K)
        e0, b0 = frame0_check(g[0], heat_d, map_pad, out_shape, dt == torch.float32)
        print(f"softmap read-out {CASE_ID(case)} out={str(dt)[-7:]}: frames>=1 max err {float(err.max()):.3e} (bound there "
              f"{float(bound.flatten()[err.argmax()]):.3e}, largest err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}); "
              f"frame 0 max err {e0:.3e} (largest bound {b0:.3e})")
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
        assert not bool(g[:, 0].any())                                              # the all-zero map: exactly zero in every frame
    # the two output dtypes hold the same values: frames >= 1 are f32 values widened; frame 0 is rounded once for the f32 output
    assert torch.equal(got[torch.float64][1:], got[torch.float32][1:].double())
    assert torch.equal(got[torch.float64][0].float(), got[torch.float32][0])
    assert ops.softmap_readout(bank_d, heat_d, Hf, Wf, map_pad, out_shape).dtype == heat.dtype     # default: np.stack's dtype
    # a frame range in the middle is the same rows of the full call, bit for bit; so is a range that starts at frame 0
    for dt in (torch.float32, torch.float64):
        mid = ops.softmap_readout(bank_d, heat_d, Hf, Wf, map_pad, out_shape, frames=(1, T - 1), out_dtype=dt)
        assert mid.shape[0] == T - 2 and torch.equal(mid, got[dt][1:T - 1])
        head = ops.softmap_readout(bank_d, heat_d, Hf, Wf, map_pad, out_shape, frames=(0, 2), out_dtype=dt)
        assert torch.equal(head, got[dt][:2])
        one = ops.softmap_readout(None, heat_d, Hf, Wf, map_pad, out_shape, frames=(0, 1), out_dtype=dt)       # frame 0 needs no bank
        assert torch.equal(one, got[dt][:1])


def test_readout_odd_sizes_channel_groups_and_small_outputs(dev):
    """Shapes that leave the common path: K not a multiple of 4 (scalar staging loads), K > 16 (several channel groups, the last one
    partial), an odd w0 (row starts at every alignment), and an output much smaller than the feature grid (the footprint of a tile does
    not fit the staging buffer: the kernel reads the bank directly).  Same bound."""
    from fgvc_amd import engine, ops
    for T, K, (hm, wm), d, (Hf, Wf), out_shape in ((3, 37, (60, 75), 2, (30, 38), (57, 71)), (3, 5, (200, 300), 2, (200, 300), (17, 23)),
                                                    (2, 256, (30, 40), 2, (15, 20), (30, 40)), (3, 8, (64, 64), 2, (64, 64), (9, 130))):
        rng = np.random.default_rng(K)
        heat = heat_maps(K, hm, wm, 3.0, rng, torch.float32).to(dev)
        bank = bank_rows(T, Hf, Wf, K, rng).to(dev)
        _, map_pad = engine.pad_divide_by(hm, wm, d)
        got = ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape)
        err = (got[1:].double() - later_restated(bank, Hf, Wf, (hm, wm), map_pad, out_shape)).abs().flatten(-2).amax(-1)
        bound = later_bound(bank, Hf, Wf, (hm, wm), map_pad)
        print(f"softmap read-out K={K} {Hf}x{Wf} -> {out_shape}: largest err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())
        frame0_check(got[0], heat, map_pad, out_shape, True)
        coords = ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape).cpu().numpy()
        dec, gap = decode(got)
        clear = gap.T > CLEAR
        assert clear.any() and float(np.abs(dec - coords).max(0)[clear].max()) <= _tol_decode(False, out_shape)


@pytest.mark.parametrize("case", READOUT_CASES, ids=CASE_ID)
def test_written_maps_are_the_coordinate_readouts_field(dev, case):
    """img2coord of the written maps is fgvc_heatmap_coords_f32's answer: both evaluate the same field with the same device functions,
    so on clear maps only the last step (five products summed) can differ."""
    from fgvc_amd import ops
    heat, bank, map_pad, Hf, Wf, out_shape = _readout_case(case, 11)
    f64 = heat.dtype == torch.float64
    heat_d, bank_d = heat.to(dev), bank.to(dev)
    maps = ops.softmap_readout(bank_d, heat_d, Hf, Wf, map_pad, out_shape)              # the stack's dtype
    coords = ops.heatmap_coords(bank_d, heat_d, Hf, Wf, map_pad, out_shape).cpu().numpy()
    dec, gap = decode(maps)
    clear = gap.T > CLEAR
    err = np.abs(dec - coords).max(0)
    tol = _tol_decode(f64, out_shape)
    print(f"maps vs coordinate read-out {CASE_ID(case)}: {int((~clear).sum())} unclear of {clear.size}, max err on clear "
          f"{float(err[clear].max()):.3e} px (tol {tol:.1e})")
    assert clear.mean() > 0.5 and float(err[clear].max()) <= tol
    # ... and the unclear maps too (plateaus: ties at rank 5): the decoder above applies the kernel's tie rule, so any map whose written
    # values differed from the scanned ones in a single bit at a tie would pick other pixels
    assert float(err.max()) <= tol, np.argwhere(err > tol)[:8].tolist()
    assert np.array_equal(coords[:, 0], np.full((2, bank.shape[0]), -1.0)) and np.array_equal(dec[:, 0], coords[:, 0])
    assert not bool(maps[:, 0].any())


# ---- the engine's whole clip against the restatement on the same top-k lists ------------------------------------------------------
def _clip(dev, T, C_feat, Hf, Wf, seed):
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, C_feat, Hf, Wf, generator=g)
    feats = torch.cat([torch.roll(base, shifts=(t, t), dims=(2, 3)) + 0.3 * torch.randn(1, C_feat, Hf, Wf, generator=g)
                       for t in range(T)])
    return ops.normalize_to_hwc(feats.to(dev))


def _check_clip(name, got, bank64, heat, Hf, Wf, map_pad, out_shape, topk, dev):
    """got (T, K, h0, w0) from the engine against the restatement on `bank64` (T, HW, K) float64, propagated through the same lists.
    The product's bank is f32: a propagated value is a topk-term f32 sum with weights that sum to 1 (each product, each add and the
    weights' own sum round once: (topk + 2) * 2^-24 * M per frame, M = max|heat| bounds every value), accumulated over f frames, and
    the read-out's own bound on top."""
    T, K = bank64.shape[0], heat.shape[0]
    assert got.shape == (T, K, *out_shape) and got.dtype == heat.dtype and got.device.type == "cuda"
    want = later_restated(bank64.to(dev), Hf, Wf, heat.shape[1:], map_pad, out_shape)
    M = float(heat.abs().max())
    prop = (topk + 2) * 2.0 ** -24 * M * torch.arange(1, T, device=dev, dtype=torch.float64)[:, None]
    bound = later_bound(bank64.to(dev), Hf, Wf, heat.shape[1:], map_pad) + prop
    err = (got[1:].double() - want).abs().flatten(-2).amax(-1)
    e0, b0 = frame0_check(got[0], heat.to(dev), map_pad, out_shape, heat.dtype == torch.float32)
    print(f"{name} {heat.dtype}: frames>=1 max err {float(err.max()):.3e}, largest err/bound {float((err / bound).max()):.3f}; "
          f"frame 0 max err {e0:.3e} (bound {b0:.3e})")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_propagate_softmaps_matches_restatement(dev, dtype):
    from fgvc_amd import engine
    T, h, w, d, K = 7, 62, 70, 2, 9
    (hp, wp), _ = engine.pad_divide_by(h, w, d)
    Hf, Wf = hp // d, wp // d
    hm, wm = 31, 35                                        # a half-size map, padded by its own pad_divide_by
    _, map_pad = engine.pad_divide_by(hm, wm, d)
    heat = heat_maps(K, hm, wm, 3.0, np.random.default_rng(5), dtype)
    feats = _clip(dev, T, 64, Hf, Wf, 11)
    cfg = engine.TrackerConfig(neighbor_range=8, precede_frames=3)
    ev = {k: torch.cuda.Event(enable_timing=True) for k in ("labels", "affinity", "propagation", "readout", "end")}
    out_shape = (h, w)
    got = engine.propagate_softmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg, events=ev)
    torch.cuda.synchronize()
    assert all(ev["labels"].elapsed_time(ev[k]) >= 0 for k in ("affinity", "propagation", "readout", "end"))
    plan = engine.plan_clip(T, [0], cfg)
    tk = engine.run_affinity(feats, Hf, Wf, plan, cfg)
    HW = Hf * Wf
    bank = torch.zeros(T, HW, K, dtype=torch.float64)
    b0 = F.interpolate(F.pad(heat[None], map_pad), size=(Hf, Wf), mode="bilinear", align_corners=False).float()[0]
    bank[0] = b0.permute(1, 2, 0).reshape(HW, K).double()
    for f in range(1, T):
        row = tk.row(plan.out_rows[(0, f)])
        idx, wt, sf = tk.idx[row].cpu().long(), tk.weight[row].cpu().double(), tk.slot_frame[row].cpu().long()
        slot, pix = idx // HW, idx % HW
        bank[f] = (wt[..., None] * bank[sf[slot], pix]).sum(1)
    _check_clip("propagate_softmaps", got, bank, heat, Hf, Wf, map_pad, out_shape, cfg.topk, dev)
    # the range form, and the coordinates of the same clip: one bank, two read-outs
    part = engine.propagate_softmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg, frames=(2, 5))
    assert torch.equal(part, got[2:5])
    coords = engine.propagate_heatmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg).cpu().numpy()
    dec, gap = decode(got)
    clear = gap.T > CLEAR
    assert clear.any() and float(np.abs(dec - coords).max(0)[clear].max()) <= _tol_decode(dtype == torch.float64, out_shape)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_propagate_softmaps_local_matches_restatement(dev, dtype):
    from fgvc_amd import engine
    T, h, w, d, K, R = 6, 62, 70, 2, 7, 4
    (hp, wp), _ = engine.pad_divide_by(h, w, d)
    Hf, Wf = hp // d, wp // d
    hm, wm = 31, 35
    _, map_pad = engine.pad_divide_by(hm, wm, d)
    heat = heat_maps(K, hm, wm, 3.0, np.random.default_rng(6), dtype)
    feats = _clip(dev, T, 64, Hf, Wf, 12)
    cfg = engine.LocalConfig(temperature=0.07, topk=10, precede_frames=3, radius=R)
    out_shape = (h, w)
    stats = {}
    got = engine.propagate_softmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg, affinity_stats=stats)
    assert stats["route"] in ("f16x3", "f32")
    plan = engine.plan_local_clip(T, cfg, Hf * Wf)
    idx_all, _, weight_all = engine.run_local_affinity(feats, Hf, Wf, plan, cfg)
    _, slot_frame = plan.tables(dev)
    HW, L = Hf * Wf, 2 * R + 1
    bank = torch.zeros(T, HW, K, dtype=torch.float64)
    b0 = F.interpolate(F.pad(heat[None], map_pad), size=(Hf, Wf), mode="bilinear", align_corners=False).float()[0]
    bank[0] = b0.permute(1, 2, 0).reshape(HW, K).double()
    qy, qx = torch.arange(HW)[:, None] // Wf, torch.arange(HW)[:, None] % Wf
    for f in range(1, T):
        idx, wt, sf = idx_all[f - 1].cpu().long(), weight_all[f - 1].cpu().double(), slot_frame[f - 1].cpu().long()
        slot, tap = idx // (L * L), idx % (L * L)               # candidate = slot position * L^2 + tap, taps row-major over (dy, dx)
        ky, kx = qy + tap // L - R, qx + tap % L - R
        inside = (ky >= 0) & (ky < Hf) & (kx >= 0) & (kx < Wf)  # a tap outside the frame carries label 0 (zero padding)
        val = bank[sf[slot], (ky.clamp(0, Hf - 1) * Wf + kx.clamp(0, Wf - 1))] * inside[..., None]
        bank[f] = (wt[..., None] * val).sum(1)
    _check_clip("propagate_softmaps_local", got, bank, heat, Hf, Wf, map_pad, out_shape, cfg.topk, dev)
    part = engine.propagate_softmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg, frames=(0, 3))
    assert torch.equal(part, got[:3])
    coords = engine.propagate_heatmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg).cpu().numpy()
    dec, gap = decode(got)
    clear = gap.T > CLEAR
    assert clear.any() and float(np.abs(dec - coords).max(0)[clear].max()) <= _tol_decode(dtype == torch.float64, out_shape)


# ---- tracker API against the reference's own output ------------------------------------------------------------------------------
DENSE_FIXTURES = ["softmap_jhmdb_6x48x64", "softmap_badja_6x56x80", "softmap_pad_5x41x47"]
LOCAL_FIXTURES = ["hr_softmap_jhmdb_6x48x64", "hr_softmap_pad_5x41x47"]


def _model(dev, g, kind, arith, extra):
    from oracle import fgvc_oracle as O
    import fgvc_amd.mmpt_api as api
    cfg = dict(json.loads(str(g["test_cfg"])), **extra)
    if arith == "f16x3" and kind == "VanillaTracker":
        cfg["pair_split_fmt"] = "f16"
    model = api.build_model(dict(type=kind, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                            train_cfg=None, test_cfg=api.ConfigDict(**cfg))
    model.backbone.load_state_dict(O.seeded_resnet_state(int(g["seed"]), (1, 1, 1, 4), "none"), strict=False)
    model = model.to(dev).eval()
    if arith is not None:                                  # None: the arithmetic a freshly built model runs
        model.backbone.set_arith(arith)
    return model


def _call(model, g, dev):
    imgs = torch.from_numpy(g["imgs"].astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous().to(dev)
    heat = torch.from_numpy(g["ref_seg_map"]).unsqueeze(0).to(dev)
    meta = [dict(original_shape=tuple(int(v) for v in g["original_shape"]))]
    return model(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)


@pytest.mark.parametrize("arith", ["f16x3", None], ids=["f16x3", "default"])
@pytest.mark.parametrize("name", DENSE_FIXTURES + LOCAL_FIXTURES)
def test_model_call_matches_reference_fixture(dev, golden, name, arith):
    """model(test_mode=True, imgs=, ref_seg_map=4-D, img_meta=) with return_maps=True against the reference's coords=False output:
    frame 0 under the frame-0 bound, frames f >= 1 at most 1 % of the values above atol(f) = 2 delta f M and none above
    atol(f) + f M / topk (module docstring).  First MI355X run: see docs/LAB_NOTES.md."""
    g = golden(name)
    kind = "HRVanillaTracker" if name in LOCAL_FIXTURES else "VanillaTracker"
    model = _model(dev, g, kind, arith, dict(return_maps=True))
    out = _call(model, g, dev)
    heat = g["ref_seg_map"]
    T, K = g["imgs"].shape[1], heat.shape[0]
    shape = tuple(int(v) for v in g["original_shape"])
    assert isinstance(out, list) and len(out) == 1 and isinstance(out[0], np.ndarray)
    pred = out[0]
    assert pred.shape == (T, K, *shape) and pred.dtype == heat.dtype
    # frame 0 against the reference's own (PyTorch's interpolation in the map's dtype)
    from fgvc_amd import engine
    heat_t = torch.from_numpy(heat)
    _, map_pad = engine.pad_divide_by(heat.shape[1], heat.shape[2], 2)          # both set-ups pad by 2 (the reference tracker's `stride`)
    e0, b0 = frame0_check(torch.from_numpy(pred[0]), heat_t, map_pad, shape, heat.dtype == np.float32, want=torch.from_numpy(g["maps0"]))
    # frames >= 1
    M = float(np.abs(heat).max())
    topk = int(json.loads(str(g["test_cfg"]))["topk"])
    fr = np.arange(1, T, dtype=np.float64)[:, None]
    atol, flip = 2 * DELTA * fr * M, fr * M / topk
    diff = np.abs(pred[1:].astype(np.float64) - g["maps"].astype(np.float64)).reshape(T - 1, -1)
    share = float((diff > atol).mean())
    worst = float((diff / (atol + flip)).max())
    noise = float(g["ref_noise_max"].max()) if "ref_noise_max" in g else float("nan")
    print(f"{name} {'default' if arith is None else arith}: frame 0 max err {e0:.2e} (bound {b0:.2e}); frames>=1 max diff {float(diff.max()):.3e} "
          f"(atol(1) {float(atol[0, 0]):.1e}), share above atol {share:.2e} (cap {SHARE_CAP}), largest diff / (atol + flip bound) {worst:.3f}; "
          f"reference f32-vs-f64 noise max {noise:.2e}")
    assert share <= SHARE_CAP
    assert bool((diff <= atol + flip).all())
    assert np.array_equal(pred[1:], pred[1:].astype(np.float32).astype(pred.dtype))        # frames >= 1 are float32 values
    if "jhmdb" in name:
        assert not pred[:, 4].any()                      # the joint off the frame: zero maps throughout


@pytest.mark.parametrize("name", ["softmap_pad_5x41x47", "hr_softmap_jhmdb_6x48x64"])
def test_model_call_chunked_is_bit_identical(dev, golden, name):
    g = golden(name)
    kind = "HRVanillaTracker" if name in LOCAL_FIXTURES else "VanillaTracker"
    heat = g["ref_seg_map"]
    frame_bytes = heat.shape[0] * int(g["original_shape"][0]) * int(g["original_shape"][1]) * heat.dtype.itemsize
    whole = _call(_model(dev, g, kind, "f16x3", dict(return_maps=True)), g, dev)[0]
    parts = _call(_model(dev, g, kind, "f16x3", dict(return_maps=True, maps_budget=2 * frame_bytes)), g, dev)[0]
    assert np.array_equal(whole, parts)
    with pytest.raises(ValueError, match=str(frame_bytes)):
        _call(_model(dev, g, kind, "f16x3", dict(return_maps=True, maps_budget=frame_bytes - 1)), g, dev)


def test_chunked_readout_bounds_device_memory(dev):
    """engine.softmaps_to_host at the DAVIS case with a budget of two frames: the result equals the unchunked read-out bit for bit, and
    the device memory allocated during the call stays under budget + one chunk -- far below the full stack."""
    from fgvc_amd import engine, ops
    heat, bank, map_pad, Hf, Wf, out_shape = _readout_case(READOUT_CASES[0], 3)
    T, K = bank.shape[0], heat.shape[0]
    heat_d, bank_d = heat.to(dev), bank.to(dev)
    frame_bytes = K * out_shape[0] * out_shape[1] * 4
    budget = 2 * frame_bytes
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    host = engine.softmaps_to_host(bank_d, heat_d, Hf, Wf, map_pad, out_shape, budget=budget)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    full = T * frame_bytes
    print(f"chunked read-out: peak {peak} B during the call, budget {budget} B, full stack {full} B")
    assert peak <= budget + 2 * frame_bytes and peak < full / 2
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host.shape == (T, K, *out_shape)
    assert np.array_equal(host, ops.softmap_readout(bank_d, heat_d, Hf, Wf, map_pad, out_shape).cpu().numpy())
    with pytest.raises(ValueError, match=str(frame_bytes)):
        engine.softmaps_to_host(bank_d, heat_d, Hf, Wf, map_pad, out_shape, budget=frame_bytes - 1)


@pytest.mark.parametrize("name", DENSE_FIXTURES + LOCAL_FIXTURES)
def test_returned_maps_decode_to_the_coords_call(dev, golden, name):
    """return_maps=True decoded on the host against the same model with coords=True, clear maps."""
    from fgvc_amd.datasets import img2coord_maps
    g = golden(name)
    kind = "HRVanillaTracker" if name in LOCAL_FIXTURES else "VanillaTracker"
    maps = _call(_model(dev, g, kind, "f16x3", dict(return_maps=True)), g, dev)[0]
    coords = _call(_model(dev, g, kind, "f16x3", dict(coords=True)), g, dev)[0]
    dec = img2coord_maps(maps)
    _, gap = decode(torch.from_numpy(maps))
    clear = gap.T > CLEAR
    err = np.abs(dec - coords).max(0)
    shape = tuple(int(v) for v in g["original_shape"])
    tol = _tol_decode(maps.dtype == np.float64, shape)
    print(f"{name}: decoded maps vs coords=True, {int(clear.sum())} clear maps of {clear.size}, max err {float(err[clear].max()):.3e} px (tol {tol:.1e})")
    assert clear.any() and float(err[clear].max()) <= tol


# ---- tools/test.py --pose-form softmap end to end ---------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("task", ["jhmdb", "badja"])
def test_tools_test_softmap_form_end_to_end(dev, tmp_path, task):
    """The two forms as two processes on one synthetic set and one set of weights: exit 0, equal PCK, the dumped maps load.  The tool
    initialises a model without a checkpoint from torch's default generator, whose seed differs from process to process, so both runs
    load the same seeded checkpoint (--checkpoint); without it the two forms score different random encoders."""
    import subprocess
    import sys
    from oracle import fgvc_oracle as O
    mk = _tool("make_fake_poses")
    names = getattr(mk, "make_" + task)(str(tmp_path / "data"), videos=2, frames=5, seed=3)
    ckpt = tmp_path / "weights.pth"
    torch.save({"state_dict": {"backbone." + k: v for k, v in O.seeded_resnet_state(17, (1, 1, 1, 4), "none").items()}}, str(ckpt))
    outs = {}
    for form in ("heatmap", "softmap"):
        out = tmp_path / f"{form}.json"
        cmd = [sys.executable, os.path.join(ROOT, "tools", "test.py"), "--task", task, "--data-root", str(tmp_path / "data"),
               "--pose-form", form, "--checkpoint", str(ckpt), "--out", str(out)]
        if form == "softmap":
            cmd += ["--dump-maps", str(tmp_path / "maps")]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[form] = json.loads(out.read_text())
    print(task, outs)
    assert outs["softmap"] == outs["heatmap"]            # the same PCK, not a close one
    shape = (60, 80) if task == "jhmdb" else (320, 512)      # JHMDB: the video's own size; BADJA: the network size
    for n in names:
        m = np.load(tmp_path / "maps" / (n + ".npy"))
        assert m.ndim == 4 and m.shape[0] == 5 and m.shape[2:] == shape and m.dtype == np.float64 and np.isfinite(m).all()
        assert task != "jhmdb" or m.shape[1] == 15
