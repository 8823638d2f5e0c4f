"""GPU tests of the heat-map path (soft first-frame labels read out as joint coordinates, vanilla_tracker.py:663-830 with a 4-D map and
coords=True): the bank-row-0 kernel against F.interpolate in float64, the coordinate read-out against a float64 torch restatement of
steps 3, 5 and 6 of the issue (frame 0 unpadded-not, later frames bilinear / unpad / bilinear, img2coord on the np.stack dtype), the
engine's whole clip against a restatement driven by the same top-k lists, the tracker API against the reference's own output
(tests/golden/heatmap_*.npz, tests/golden/gen_golden_heatmap.py), and tools/test.py --pose-form heatmap end to end.

"Clear" map: (5th - 6th largest value) / max > 1e-5 in float64, so the top 5 is the same set under any rounding of the values.  The
normalisation of an f32 stack rounds the top-5 sum once in f32: a one-ulp change of that sum moves a coordinate by x * 2^-24, so the
f32 flavour's tolerance carries that term (TOL_F32_ULPS ulps of the largest coordinate)."""
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
TOL_PX = 1e-5
TOL_F32_ULPS = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _tol(f64: bool, out_shape, base=TOL_PX) -> float:
    return base if f64 else base + TOL_F32_ULPS * 2.0 ** -24 * max(out_shape)


def _ulp32(x: torch.Tensor) -> torch.Tensor:
    x = x.float().abs()
    return torch.nextafter(x, torch.full_like(x, float("inf"))) - x


# ---- float64 restatement (torch) ---------------------------------------------------------------------------------------------------
def maps_restated(bank, heat, Hf, Wf, map_pad, out_shape):
    """(T, K, h0, w0) float64: frame 0 = bilinear(padded heat -> out_shape) in heat's dtype, NOT unpadded (:712-716); frame f >= 1 =
    bilinear(bank[f] -> padded size), unpad, bilinear(-> out_shape), in float64 (:770-784)."""
    K, hm, wm = heat.shape
    lw, uw, lh, uh = map_pad
    hp, wp = hm + lh + uh, wm + lw + uw
    padded = F.pad(heat[None], map_pad)
    f0 = F.interpolate(padded, size=tuple(out_shape), mode="bilinear", align_corners=False).double()
    T = bank.shape[0]
    x = bank[1:].double().reshape(T - 1, Hf, Wf, K).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=(hp, wp), mode="bilinear", align_corners=False)[:, :, lh:hp - uh, lw:wp - uw]
    x = F.interpolate(x, size=tuple(out_shape), mode="bilinear", align_corners=False)
    return torch.cat([f0, x], 0)


def img2coord_restated(maps: torch.Tensor, f64: bool):
    """img2coord (:172-191) of (T, K, h0, w0) float64 maps on the stack dtype: f64 -> float64 normalisation, else float32.  Ties: a stable
    ascending sort puts the higher flat index last (the kernels' rule).  Returns (coords (2, K, T), gap (T, K) = (5th - 6th) / max)."""
    T, K, h0, w0 = maps.shape
    flat = maps.reshape(T, K, -1)
    work = flat if f64 else flat.float()
    srt, idx = torch.sort(work, dim=-1, stable=True)
    top_i = idx[..., -5:].cpu().numpy()
    top_v = srt[..., -5:].cpu().numpy()
    v = top_v / (np.sum(top_v, axis=-1, keepdims=True) + 1e-9)
    coords = np.zeros((2, K, T))
    coords[0] = np.sum((top_i % w0) * v, axis=-1).T
    coords[1] = np.sum((top_i // w0) * v, axis=-1).T
    zero = (work.sum(-1) == 0).cpu().numpy()
    coords[:, zero.T] = -1
    s6 = torch.sort(flat, dim=-1).values[..., -6:]
    mx = s6[..., -1].abs().clamp_min(1e-300)
    gap = ((s6[..., 1] - s6[..., 0]) / mx).cpu().numpy()
    return coords, gap


def heat_maps(K, hm, wm, sigma, rng, dtype=torch.float64):
    """K Gaussians (peak 1) at random centres, one per joint, as the pose datasets draw them."""
    yy, xx = np.mgrid[0:hm, 0:wm]
    out = np.zeros((K, hm, wm))
    for k in range(K):
        cy, cx = rng.uniform(0, hm - 1), rng.uniform(0, wm - 1)
        out[k] = np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    return torch.from_numpy(out).to(dtype)


def bank_rows(T, Hf, Wf, K, rng, special=True):
    """(T, HfWf, K) f32 propagated-like labels: one smooth bump per channel per frame; with `special`: an all-zero channel (exactly -1),
    a plateau channel (a flat top wider than 5 pixels), a channel with negative values."""
    yy, xx = np.mgrid[0:Hf, 0:Wf]
    b = np.zeros((T, Hf, Wf, K))
    for t in range(T):
        for k in range(K):
            cy, cx = rng.uniform(0, Hf - 1), rng.uniform(0, Wf - 1)
            s = rng.uniform(1.5, 4.0)
            b[t, :, :, k] = rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    if special and K >= 4:
        b[:, :, :, 0] = 0.0
        b[:, :, :, 1] = np.minimum(b[:, :, :, 1], 0.5 * b[:, :, :, 1].max(axis=(1, 2), keepdims=True))
        b[:, :, :, 2] = b[:, :, :, 2] - 0.3
    return torch.from_numpy(b.reshape(T, Hf * Wf, K)).float()


# ---- bank row 0 ------------------------------------------------------------------------------------------------------------------
SOFT_CASES = [
    # (K, hm, wm, d, Hf, Wf) -- the feature grid is the PADDED FRAME's, which need not be the map's padded size / d
    (15, 41, 47, 2, 21, 24),          # padded map, odd sizes
    (20, 160, 256, 2, 160, 256),      # BADJA: a half-size map to the network's feature grid
    (15, 320, 320, 2, 160, 160),      # JHMDB at the network size
    (1, 37, 50, 4, 12, 13),           # K = 1, map != frame size
]


@pytest.mark.parametrize("case", SOFT_CASES, ids=lambda c: f"K{c[0]}_{c[1]}x{c[2]}_to_{c[4]}x{c[5]}")
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_soft_labels_match_interpolate(dev, case, dtype):
    from fgvc_amd import engine, ops
    K, hm, wm, d, Hf, Wf = case
    rng = np.random.default_rng(hm * 3 + K)
    heat = heat_maps(K, hm, wm, 3.0, rng, dtype)
    _, pad = engine.pad_divide_by(hm, wm, d)
    got = ops.seg_soft_labels(heat.to(dev), pad, Hf, Wf).cpu()
    # the reference's arithmetic: F.interpolate in the map's dtype (f64 input: against float64; f32 input: against torch's own f32 result,
    # whose weights are rounded to f32 as the kernel's are)
    want = F.interpolate(F.pad(heat.to(dev)[None], pad), size=(Hf, Wf), mode="bilinear", align_corners=False)[0]
    want = want.permute(1, 2, 0).reshape(Hf * Wf, K).cpu().double()
    err = (got.double() - want).abs()
    ulps = 1 if dtype == torch.float64 else 2
    assert bool((err <= ulps * _ulp32(want).double() + 1e-30).all()), float((err / _ulp32(want).double().clamp_min(1e-45)).max())
    if dtype == torch.float64:         # one rounding of the f64 value: .float() of it, up to a tie of the last bit
        assert float((got.double() - want.float().double()).abs().max()) <= float(_ulp32(want).max())


# ---- read-out ------------------------------------------------------------------------------------------------------------------
READOUT_CASES = [
    # (T, K, (hm, wm), d, (Hf, Wf), (h0, w0), heat dtype)
    (8, 16, (480, 854), 2, (240, 427), (480, 854), torch.float32),       # DAVIS size, K = 16
    (8, 16, (480, 854), 2, (240, 427), (480, 854), torch.float64),
    (6, 15, (320, 320), 2, (160, 160), (240, 320), torch.float64),       # JHMDB: network 320 x 320, scored at the video's 240 x 320
    (5, 20, (320, 512), 2, (160, 256), (320, 512), torch.float64),       # BADJA: at the network size
    (4, 6, (41, 47), 2, (21, 24), (45, 52), torch.float32),              # padded map, original_shape != map size
    (4, 6, (41, 47), 2, (21, 24), (45, 52), torch.float64),
]


def _readout_case(dev, case, seed):
    from fgvc_amd import engine
    T, K, (hm, wm), d, (Hf, Wf), out_shape, dtype = case
    rng = np.random.default_rng(seed)
    heat = heat_maps(K, hm, wm, 4.0, rng, dtype)
    if K >= 4:
        heat[0] = 0                                        # all-zero joint: -1 in every frame
        heat[1] = heat[1].clamp_max(0.6)                   # flat top: ties at rank 5
        heat[2] = heat[2] - 0.25                           # negative values
    _, map_pad = engine.pad_divide_by(hm, wm, d)
    bank = bank_rows(T, Hf, Wf, K, rng)
    return heat, bank, map_pad, Hf, Wf, out_shape


@pytest.mark.parametrize("case", READOUT_CASES, ids=lambda c: f"T{c[0]}K{c[1]}_{c[2][0]}x{c[2][1]}_to_{c[5][0]}x{c[5][1]}_{str(c[6])[-7:]}")
def test_readout_matches_float64_restatement(dev, case):
    from fgvc_amd import ops
    heat, bank, map_pad, Hf, Wf, out_shape = _readout_case(dev, case, 7)
    T, K = bank.shape[0], heat.shape[0]
    f64 = heat.dtype == torch.float64
    heat_d, bank_d = heat.to(dev), bank.to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    got = ops.heatmap_coords(bank_d, heat_d, Hf, Wf, map_pad, out_shape)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    full = T * K * out_shape[0] * out_shape[1] * 4
    assert peak < full / 10, (peak, full)
    got = got.cpu().numpy()
    assert got.shape == (2, K, T) and got.dtype == np.float64
    want, gap = img2coord_restated(maps_restated(bank_d, heat_d, Hf, Wf, map_pad, out_shape), f64)
    clear = gap.T > CLEAR                                  # (K, T)
    err = np.abs(got - want).max(0)
    tol = _tol(f64, out_shape)
    print(f"read-out {case[:6]} f64={f64}: {int((~clear).sum())} unclear maps of {clear.size}, max err on clear "
          f"{float(err[clear].max()) if clear.any() else 0.0:.3e} px (tol {tol:.1e}), peak {peak} B of a map stack's {full} B")
    assert float(err[clear].max()) <= tol
    assert clear.mean() > 0.5                              # (the zero and plateau joints are unclear by construction)
    if K >= 4:
        assert np.array_equal(got[:, 0], np.full((2, T), -1.0))           # all-zero joint: exactly -1 (frame 0 and the bank's zero channel)
    # the arithmetic flag: the other flavour differs from this one's restatement no more than by the f32 rounding terms
    other = ops.heatmap_coords(bank_d, heat_d, Hf, Wf, map_pad, out_shape, f64_arith=not f64).cpu().numpy()
    assert float(np.abs(other - got)[:, clear].max()) <= _tol(False, out_shape)


def test_readout_single_frame_and_zero_maps(dev):
    from fgvc_amd import ops
    heat = torch.zeros(3, 30, 40, dtype=torch.float64)
    heat[1, 10, 20] = 1.0                                  # one pixel: bilinear spreads it over a 2 x 2 neighbourhood at most
    bank = torch.zeros(1, 15 * 20, 3)
    got = ops.heatmap_coords(bank.to(dev), heat.to(dev), 15, 20, (0, 0, 0, 0), (30, 40)).cpu().numpy()
    assert got.shape == (2, 3, 1)
    assert np.array_equal(got[:, 0], [[-1.0], [-1.0]]) and np.array_equal(got[:, 2], [[-1.0], [-1.0]])
    assert got[0, 1, 0] == pytest.approx(20.0, abs=1e-6) and got[1, 1, 0] == pytest.approx(10.0, abs=1e-6)


# ---- the engine's whole clip against the restatement on the same top-k lists ------------------------------------------------------
def _clip(dev, T, C_feat, Hf, Wf, seed):
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, C_feat, Hf, Wf, generator=g)
    feats = torch.cat([torch.roll(base, shifts=(t, t), dims=(2, 3)) + 0.3 * torch.randn(1, C_feat, Hf, Wf, generator=g)
                       for t in range(T)])
    return ops.normalize_to_hwc(feats.to(dev))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_propagate_heatmaps_matches_restatement(dev, dtype):
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
    got = engine.propagate_heatmaps(feats, Hf, Wf, heat.to(dev), map_pad, out_shape, cfg, events=ev)
    torch.cuda.synchronize()
    assert got.shape == (2, K, T) and got.dtype == torch.float64 and got.device.type == "cuda"
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
    f64 = dtype == torch.float64
    want, gap = img2coord_restated(maps_restated(bank.to(dev), heat.to(dev), Hf, Wf, map_pad, out_shape), f64)
    clear = gap.T > CLEAR
    err = np.abs(got.cpu().numpy() - want).max(0)
    print(f"propagate_heatmaps {dtype}: {int((~clear).sum())} unclear of {clear.size}, max err on clear {float(err[clear].max()):.3e} px")
    assert float(err[clear].max()) <= _tol(f64, out_shape)


# ---- tracker API against the reference's own output (tests/golden/heatmap_*.npz) --------------------------------------------------
HEATMAP_FIXTURES = ["heatmap_jhmdb_6x48x64", "heatmap_badja_6x56x80", "heatmap_pad_5x41x47"]
# Largest coordinate difference (px) on the DEFAULT arithmetic (f16 + FP6 encoder, f16 + FP6 pair kernel + refining merge), clear maps
# of frames 1..: the figure of the first MI355X run of this test, per fixture.
DEFAULT_MISMATCH_BOUND = {"heatmap_jhmdb_6x48x64": 1.6e-4, "heatmap_badja_6x56x80": 4.5e-4, "heatmap_pad_5x41x47": 6e-6}
# (first MI355X run: 1.58e-4, 4.40e-4 and 5.10e-6 px.)  The f16x3 arithmetic's bound on clear maps of frames 1..: the first run measured
# 1.5e-7 (JHMDB-like), 1.35e-4 (BADJA-like) and 4.2e-6 px (padded).  The BADJA-like clip's figure is above the 1e-4 px first aimed at;
# the read-out itself agrees with a float64 restatement on the same top-k lists to 1e-7 px (test_propagate_heatmaps_matches_restatement),
# so the difference comes from the lists, i.e. the affinity arithmetic.
F16X3_LATER_BOUND = 2e-4


def _fixture_run(dev, golden, name, arith, pair_split_fmt=None):
    from oracle import fgvc_oracle as O
    import fgvc_amd.mmpt_api as api
    g = golden(name)
    cfg = dict(json.loads(str(g["test_cfg"])), coords=True)
    if pair_split_fmt is not None:
        cfg["pair_split_fmt"] = pair_split_fmt
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")), train_cfg=None, test_cfg=api.ConfigDict(**cfg))
    model.backbone.load_state_dict(O.seeded_resnet_state(int(g["seed"]), (1, 1, 1, 4), "none"), strict=False)
    model = model.to(dev).eval()
    model.backbone.set_arith(arith)
    imgs = torch.from_numpy(g["imgs"].astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous().to(dev)
    heat = torch.from_numpy(g["ref_seg_map"]).unsqueeze(0).to(dev)
    meta = [dict(original_shape=tuple(int(v) for v in g["original_shape"]))]
    out = model(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
    assert isinstance(out, list) and len(out) == 1 and out[0].shape == g["coords"].shape and out[0].dtype == np.float64
    return g, out[0]


def _clear_err(g, pred):
    clear = g["gap"].T > CLEAR                            # gap (T, K) -> (K, T)
    err = np.abs(pred - g["coords"]).max(0)
    return clear, err


@pytest.mark.parametrize("name", HEATMAP_FIXTURES)
def test_heatmap_f16x3_matches_reference_fixture(dev, golden, name):
    """The reference's forward_test_backward_save_mem with coords=True against the tracker API on the f16x3 arithmetic: frame 0 within
    1e-6 px (plus the f32 rounding term for an f32 map) on clear maps, later frames within 1e-4 px on clear maps, undecidable maps (a tie
    at rank 5: np.argsort's quicksort picks among equals in its own order) within 1 px.  BADJA's frame 0 has no clear map: its map is
    drawn at half size around integer-truncated corners and upsampled 2x, so the values around every peak come in equal pairs."""
    g, pred = _fixture_run(dev, golden, name, "f16x3", "f16")
    clear, err = _clear_err(g, pred)
    f64 = g["ref_seg_map"].dtype == np.float64
    shape = tuple(int(v) for v in g["original_shape"])
    e0 = err[:, 0][clear[:, 0]]
    later = err[:, 1:][clear[:, 1:]]
    unclear = err[~clear]
    print(f"{name} f16x3: frame 0 {e0.size} clear maps, max {float(e0.max()) if e0.size else 0.0:.2e} px; later clear max "
          f"{float(later.max()):.2e} px; {unclear.size} undecidable maps, max {float(unclear.max()) if unclear.size else 0.0:.2e} px")
    if name != "heatmap_badja_6x56x80":
        assert e0.size > 0
    assert e0.size == 0 or float(e0.max()) <= _tol(f64, shape, 1e-6)
    assert float(later.max()) <= _tol(f64, shape, F16X3_LATER_BOUND)
    assert unclear.size == 0 or float(unclear.max()) <= 1.0
    if name == "heatmap_jhmdb_6x48x64":
        assert np.array_equal(pred[:, int(g["off_joint"])], np.full((2, pred.shape[2]), -1.0))


@pytest.mark.parametrize("name", HEATMAP_FIXTURES)
def test_heatmap_default_arithmetic_against_reference_fixture(dev, golden, name):
    """The same on the DEFAULT arithmetic; the largest difference on clear maps of frames 1.. is held to DEFAULT_MISMATCH_BOUND."""
    g, pred = _fixture_run(dev, golden, name, "f16f6")
    clear, err = _clear_err(g, pred)
    f64 = g["ref_seg_map"].dtype == np.float64
    shape = tuple(int(v) for v in g["original_shape"])
    e0 = err[:, 0][clear[:, 0]]
    assert e0.size == 0 or float(e0.max()) <= _tol(f64, shape, 1e-6)
    later = err[:, 1:][clear[:, 1:]]
    unclear = err[~clear]
    print(f"{name} default arithmetic: later clear max {float(later.max()):.2e} px; {unclear.size} undecidable maps, "
          f"max {float(unclear.max()) if unclear.size else 0.0:.2e} px")
    assert float(later.max()) <= DEFAULT_MISMATCH_BOUND[name]
    assert unclear.size == 0 or float(unclear.max()) <= 1.0


# ---- tools/test.py --pose-form heatmap end to end ---------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("task", ["jhmdb", "badja"])
def test_tools_test_heatmap_form_end_to_end(dev, tmp_path, task):
    import subprocess
    import sys
    mk = _tool("make_fake_poses")
    getattr(mk, "make_" + task)(str(tmp_path), videos=2, frames=5, seed=3)
    outs = {}
    for form in ("heatmap", "points"):
        out = tmp_path / f"{form}.json"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--task", task, "--data-root", str(tmp_path),
                            "--pose-form", form, "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        outs[form] = json.loads(out.read_text())
    print(task, outs)
    for form, pck in outs.items():
        assert all(0.0 <= v <= 100.0 for k, v in pck.items() if k.startswith("PCK@") and np.isfinite(v)), (form, pck)
