"""GPU tests of HRVanillaTracker's label-map path (vanilla_tracker.py:663-830 with its own affinity, masked_attention_efficient_correlation,
local_attention.py:883-1006): the tracker API against the genuine reference's output (tests/golden/hr_seg_*.npz, hr_heatmap_*.npz,
tests/golden/gen_golden_hr_seg.py) on both pair-kernel routes, the planned merge against the per-frame local-window call bit for bit, a
float64 restatement of the operator and the read-out on the product's own feature rows at 480p, chunking, and tools/test.py --eval-arc.

"Decidable" pixel: the reference's top-two normalised channel values differ by more than 1e-5.  "Clear" heat map: (5th - 6th largest) /
max > 1e-5.
"""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECIDE = 1e-5
CLEAR = 1e-5
LATER_PX = 2e-4            # heat maps, clear maps of frames 1..: the f16x3 route of the dense path measured up to 1.35e-4 px
F32_ULPS = 4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _model(dev, g, extra=None, strides=None):
    from oracle import fgvc_oracle as O
    import fgvc_amd.mmpt_api as api
    cfg = dict(json.loads(str(g["test_cfg"])), **(extra or {}))
    strides = tuple(int(v) for v in (g["strides"] if strides is None else strides))
    model = api.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=strides, out_indices=(2,),
                                                                         pool_type="none")), train_cfg=None, test_cfg=api.ConfigDict(**cfg))
    model.backbone.load_state_dict(O.seeded_resnet_state(int(g["seed"]), strides, "none"), strict=False)
    model = model.to(dev).eval()
    model.backbone.set_arith("f16x3")            # 1e-7-grade features, as the dense path's fixture tests run
    return model


def _imgs(g, dev):
    return torch.from_numpy(g["imgs"].astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous().to(dev)   # (1,1,3,T,h,w)


# ---- against the reference's own output ---------------------------------------------------------------------------------------------
MASK_FIXTURES = ["hr_seg_8x62x70", "hr_seg_hard_8x62x70", "hr_seg_vanish_5x41x47", "hr_seg_nonorm_5x62x70"]


@pytest.mark.parametrize("precision", ["auto", "f32"])
@pytest.mark.parametrize("name", MASK_FIXTURES)
def test_masks_match_reference_fixture(dev, golden, name, precision):
    """Frame 0 exact, every decidable pixel of frames 1.. equal, on the f16x3 route ('auto' where it applies) and the f32 route."""
    g = golden(name)
    model = _model(dev, g, dict(pair_precision=precision))
    meta = [dict(original_shape=tuple(int(v) for v in g["original_shape"]))]
    out = model(test_mode=True, imgs=_imgs(g, dev), ref_seg_map=torch.from_numpy(g["ref_seg_map"]).unsqueeze(0).to(dev), img_meta=meta)
    assert isinstance(out, list) and len(out) == 1
    pred, want = out[0], g["masks"]
    assert pred.dtype == np.float64 and pred.shape == want.shape
    route = model.label_stats["route"]
    assert route == ("f32" if (precision == "f32" or "nonorm" in name) else "f16x3"), route
    assert np.array_equal(pred[0], want[0].astype(np.float64))
    dec = g["gap"] > DECIDE
    bad = int(((pred[1:] != want[1:]) & dec).sum())
    print(f"{name} {route}: {bad} decidable mismatches of {dec.size} pixels ({int((~dec).sum())} undecidable)")
    assert bad == 0
    if "vanish" in name:
        assert int(want[0].max()) == 3 and int(pred[1:].max()) == 2          # the id lost at feature resolution never comes back


HEAT_FIXTURES = ["hr_heatmap_jhmdb_6x48x64", "hr_heatmap_pad_5x41x47"]


@pytest.mark.parametrize("precision", ["auto", "f32"])
@pytest.mark.parametrize("name", HEAT_FIXTURES)
def test_heatmaps_match_reference_fixture(dev, golden, name, precision):
    """coords=True: frame 0 (the padded map, not unpadded) within 1e-6 px plus the f32 rounding term for an f32 map, clear maps of frames
    1.. within 2e-4 px of the reference's coordinates."""
    g = golden(name)
    model = _model(dev, g, dict(coords=True, pair_precision=precision), strides=(1, 1, 1, 4))
    shape = tuple(int(v) for v in g["original_shape"])
    out = model(test_mode=True, imgs=_imgs(g, dev), ref_seg_map=torch.from_numpy(g["ref_seg_map"]).unsqueeze(0).to(dev),
                img_meta=[dict(original_shape=shape)])
    pred = out[0]
    assert pred.shape == g["coords"].shape and pred.dtype == np.float64
    assert model.label_stats["route"] == ("f32" if precision == "f32" else "f16x3")
    clear = g["gap"].T > CLEAR
    err = np.abs(pred - g["coords"]).max(0)
    f32_term = 0.0 if g["ref_seg_map"].dtype == np.float64 else F32_ULPS * 2.0 ** -24 * max(shape)
    e0, later = err[:, 0][clear[:, 0]], err[:, 1:][clear[:, 1:]]
    print(f"{name} {model.label_stats['route']}: frame 0 max {float(e0.max()):.2e} px over {e0.size} clear maps; later max "
          f"{float(later.max()):.2e} px over {later.size}")
    assert e0.size > 0 and float(e0.max()) <= 1e-6 + f32_term
    assert later.size > 0 and float(later.max()) <= LATER_PX + f32_term
    if "jhmdb" in name:
        assert np.array_equal(pred[:, 4], np.full((2, pred.shape[2]), -1.0))     # the joint off the frame: a zero map throughout


# ---- the planned merge against the per-frame call --------------------------------------------------------------------------------------
def _bank(dev, T, H, W, C=256, seed=0, normalise=True):
    from fgvc_amd import ops
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(T, C, H, W, generator=gen)
    x = F.avg_pool2d(x, 3, 1, 1) + 0.3 * x                    # neighbouring pixels alike, as encoder features are
    return ops.normalize_to_hwc(x.to(dev), normalise)


@pytest.mark.parametrize("case", [dict(route="f16x3", topk=10, R=5), dict(route="f32", topk=10, R=5), dict(route="f32", topk=16, R=3, norm=False),
                                  dict(route="f16x3", topk=5, R=15)], ids=lambda c: f"{c['route']}-k{c['topk']}-R{c['R']}")
def test_plan_merge_bit_identical_to_per_frame_call(dev, case):
    """Every row of the planned affinity (one pair launch, one merge launch) equals fgvc_local_corr_topk_{f16x3,f32} of that frame on
    its own slots, bit for bit -- frames 1..3 carry frame 0 in two slots (precede_frames = 3)."""
    from fgvc_amd import engine, ops
    T, H, W = 7, 37, 53
    norm = case.get("norm", True)
    feats = _bank(dev, T, H, W, seed=case["topk"] + case["R"], normalise=norm)
    cfg = engine.LocalConfig(temperature=0.07 if norm else 20.0, topk=case["topk"], precede_frames=3, radius=case["R"], with_norm=norm,
                             pair_precision="auto" if case["route"] == "f16x3" else "f32")
    plan = engine.plan_local_clip(T, cfg, H * W)
    stats = {}
    idx, logit, weight = engine.run_local_affinity(feats, H, W, plan, cfg, stats)
    assert stats["route"] == case["route"] and stats["chunks"] == 1
    assert plan.slot_frame[0][:2] == [0, 0] and plan.slot_frame[2][:2] == [0, 0]
    for f in range(1, T):
        ks = plan.slot_frame[f - 1][:len(engine.key_slots(f, 0, 3, True))]
        i1, l1, w1 = ops.local_corr_topk(feats[f:f + 1], feats[ks], H, W, case["R"], case["topk"], cfg.temperature,
                                         normalized=(case["route"] == "f16x3"))
        assert torch.equal(idx[f - 1], i1) and torch.equal(logit[f - 1], l1) and torch.equal(weight[f - 1], w1), f
    assert not ops.pair_f16x3_timed_out()
    L2 = (2 * case["R"] + 1) ** 2
    assert int(idx[0].max()) < 2 * L2 and int((idx[0] >= L2).sum()) > 0       # frame 1: both copies of frame 0 are candidate sets


def test_chunking_is_invisible(dev):
    """A pair-list budget that forces several chunks gives the bits of one chunk, the workspace stays within the budget, and the whole
    path (masks) is unchanged."""
    from fgvc_amd import engine
    T, H, W = 9, 41, 60
    feats = _bank(dev, T, H, W, seed=5)
    cfg = engine.LocalConfig(temperature=0.07, topk=10, precede_frames=4, radius=6)
    st1 = {}
    one = engine.run_local_affinity(feats, H, W, engine.plan_local_clip(T, cfg, H * W), cfg, st1)
    budget = 7 * H * W * 10 * 8
    cfgs = engine.LocalConfig(temperature=0.07, topk=10, precede_frames=4, radius=6, pair_budget=budget)
    plan = engine.plan_local_clip(T, cfgs, H * W)
    st = {}
    many = engine.run_local_affinity(feats, H, W, plan, cfgs, st)
    assert st1["chunks"] == 1 and st["chunks"] == len(plan.chunks) >= 3
    assert st["workspace_bytes"] <= budget < st1["workspace_bytes"]
    for a, b in zip(one, many):
        assert torch.equal(a, b)
    seg = torch.zeros(H * 2, W * 2, dtype=torch.uint8, device=dev)
    seg[10:40, 20:70], seg[50:80, 60:110] = 1, 2
    m1 = engine.propagate_masks(feats, H, W, seg, (0, 0, 0, 0), (H * 2, W * 2), cfg)
    m2 = engine.propagate_masks(feats, H, W, seg, (0, 0, 0, 0), (H * 2, W * 2), cfgs)
    assert torch.equal(m1, m2)


# ---- float64 restatement of masked_attention_efficient_correlation + the read-out ------------------------------------------------------
def _window_scores(q, k, H, W, R, y0, y1):
    """q, k (HW, C) float64 -> scores (n, L^2) of queries in rows [y0, y1) over their zero-padded (2R+1)^2 windows (slot-major tap order
    (dy, dx)), and the key pixel of each tap (-1 outside)."""
    L = 2 * R + 1
    dev = q.device
    b0, b1 = max(0, y0 - R), min(H, y1 + R)
    s = q[y0 * W:y1 * W] @ k[b0 * W:b1 * W].t()
    ys = torch.arange(y0, y1, device=dev).repeat_interleave(W)
    xs = torch.arange(W, device=dev).repeat(y1 - y0)
    dy = torch.arange(L, device=dev).repeat_interleave(L) - R
    dx = torch.arange(L, device=dev).repeat(L) - R
    ky, kx = ys[:, None] + dy[None], xs[:, None] + dx[None]
    inside = (ky >= 0) & (ky < H) & (kx >= 0) & (kx < W)
    local = ((ky - b0).clamp(0, b1 - b0 - 1) * W + kx.clamp(0, W - 1))
    sc = torch.where(inside, s.gather(1, local), torch.zeros((), dtype=s.dtype, device=dev))
    return sc, torch.where(inside, ky * W + kx, torch.full_like(ky, -1))


def _restate(feats, H, W, R, labels0, T, pre, topk, tau, rows=8):
    """The reference's per-frame loop in float64: labels (T, HW, C), and per frame a bound u (HW,) on how far the product's labels may
    lie from them: a query whose k-th and (k+1)-th scores are within 2e-6 may swap that candidate (weight w_k, labels within [0, 1]),
    and every candidate carries its key's bound forward."""
    HW = H * W
    Cl = labels0.shape[1]
    labels = [labels0]
    bounds = [torch.zeros(HW, dtype=torch.float64, device=feats.device)]
    for f in range(1, T):
        ks = [0] + list(range(max(0, f - pre), f))
        out = torch.empty((HW, Cl), dtype=torch.float64, device=feats.device)
        ub = torch.empty(HW, dtype=torch.float64, device=feats.device)
        for y0 in range(0, H, rows):
            y1 = min(H, y0 + rows)
            scs, vals, ubs = [], [], []
            for s in ks:
                sc, key = _window_scores(feats[f], feats[s], H, W, R, y0, y1)
                scs.append(sc)
                kc = key.clamp_min(0)
                vals.append(torch.where((key >= 0)[..., None], labels[s][kc], torch.zeros((), dtype=torch.float64, device=feats.device)))
                ubs.append(torch.where(key >= 0, bounds[s][kc], torch.zeros((), dtype=torch.float64, device=feats.device)))
            sc, val, ubv = torch.cat(scs, 1), torch.cat(vals, 1), torch.cat(ubs, 1)
            top, ti = sc.topk(topk + 1, dim=1)
            w = torch.softmax(top[:, :topk] / tau, dim=1)
            o = slice(y0 * W, y1 * W)
            out[o] = (w[..., None] * val.gather(1, ti[:, :topk, None].expand(-1, -1, Cl))).sum(1)
            amb = (top[:, topk - 1] - top[:, topk]) < 2e-6
            ub[o] = (w * ubv.gather(1, ti[:, :topk])).sum(1) + torch.where(amb, w[:, -1], torch.zeros_like(w[:, -1])) + 1e-6
        labels.append(out)
        bounds.append(ub)
    return labels, bounds


def _readout(lab, H, W, out_shape):
    """(HW, C) float64 -> (normalised maps (C, h0, w0), 1 / (max - min) per channel where normalised) -- vanilla_tracker.py:773-797 with no
    padding (480 x 854 at stride 2)."""
    x = lab.t().reshape(1, -1, H, W)
    x = F.interpolate(x, size=out_shape, mode="bilinear", align_corners=False)[0]
    mn, mx = x.flatten(1).min(1)[0], x.flatten(1).max(1)[0]
    scale = torch.where(mx > 0, 1.0 / (mx - mn + 1e-12), torch.ones_like(mx))
    x = torch.where(mx[:, None, None] > 0, (x - mn[:, None, None]) * scale[:, None, None], x)
    return x, scale


def _frames480(T, seed):
    """Moving textured discs on a smooth texture, (1, 1, 3, T, 480, 854) in about [-1, 1], and the frame-0 id map (3 objects)."""
    rng = np.random.default_rng(seed)
    h, w = 480, 854
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.kron(rng.random((h // 16 + 1, w // 16 + 1, 3)), np.ones((16, 16, 1)))[:h, :w] * 1.2 - 0.6
    imgs = np.zeros((T, 3, h, w), np.float32)
    seg = np.zeros((h, w), np.uint8)
    objs = [(rng.uniform([100, 150], [380, 700]), rng.uniform(-6, 6, 2), rng.uniform(50, 110), rng.uniform(-0.8, 0.8, 3)) for _ in range(3)]
    for t in range(T):
        img = base + 0.05 * rng.standard_normal((h, w, 3))
        for i, (c, v, r, col) in enumerate(objs):
            inside = (yy - c[0] - t * v[0]) ** 2 + (xx - c[1] - t * v[1]) ** 2 <= r * r
            img[inside] = col + 0.3 * base[inside]
            if t == 0:
                seg[inside] = i + 1
        imgs[t] = img.transpose(2, 0, 1)
    return torch.from_numpy(imgs).permute(1, 0, 2, 3)[None, None].contiguous(), seg


def test_masks_match_float64_restatement_480p(dev):
    """4 frames at 480 x 854 (240 x 427 features), R = 15: every window crosses a border somewhere.  The restatement is fed the
    product's own f32 feature rows; it is held at every pixel whose read-out gap exceeds 1e-5 plus twice the propagated bound of a
    near-tie swap (see _restate)."""
    import fgvc_amd.mmpt_api as api
    from fgvc_amd import engine, ops
    T, R = 4, 15
    torch.manual_seed(0)
    model = api.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                         pool_type="none")),
                            test_cfg=api.ConfigDict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=2 * R))
    model.init_weights()
    model = model.to(dev).eval()
    imgs, seg0 = _frames480(T, 7)
    imgs = imgs.to(dev)
    cfg = model._label_config()
    feats, Hf, Wf = model._label_feats(imgs[0, 0].transpose(0, 1))
    assert (Hf, Wf) == (240, 427) and feats.dtype == torch.float32 and cfg.radius == R
    seg = torch.from_numpy(seg0).to(dev)
    stats = {}
    masks = engine.propagate_masks(feats, Hf, Wf, seg, (0, 0, 0, 0), (480, 854), cfg, affinity_stats=stats)
    assert stats["route"] == "f16x3"
    C = int(ops.seg_max_label(seg, Hf, Wf).item()) + 1
    lab0 = ops.seg_onehot_labels(seg, Hf, Wf, C).double()
    labels, bounds = _restate(feats.double(), Hf, Wf, R, lab0, T, cfg.precede_frames, cfg.topk, cfg.temperature)
    total_bad, total_dec = 0, 0
    for f in range(1, T):
        x, scale = _readout(labels[f], Hf, Wf, (480, 854))
        ub = F.interpolate(bounds[f].reshape(1, 1, Hf, Wf), size=(480, 854), mode="nearest")[0, 0]
        ub = F.max_pool2d(ub[None, None], 3, 1, 1)[0, 0] * float(scale.max())          # any of the bilinear sources, in normalised units
        top2 = x.topk(2, dim=0).values
        dec = (top2[0] - top2[1]) > DECIDE + 2 * ub
        bad = int(((masks[f].long() != x.argmax(0)) & dec).sum())
        total_bad += bad
        total_dec += int(dec.sum())
        print(f"frame {f}: {bad} decidable mismatches, {int((~dec).sum())} undecidable of {dec.numel()}; largest bound {float(bounds[f].max()):.2e}")
    assert total_bad == 0
    assert total_dec > 0.8 * (T - 1) * 480 * 854


# ---- tools/test.py --eval-arc HRVanillaTracker end to end ---------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("task", ["vos", "jhmdb", "badja"])
def test_tools_test_eval_arc_hr_end_to_end(dev, tmp_path, task):
    import subprocess
    import sys
    if task == "vos":
        _tool("make_fake_davis").make(str(tmp_path), sequences=2, frames=5, size=(61, 75), objects=2, seed=1)
        extra = []
    else:
        getattr(_tool("make_fake_poses"), "make_" + task)(str(tmp_path), videos=2, frames=5, seed=3)
        extra = ["--pose-form", "heatmap"]
    out = tmp_path / "out.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--task", task, "--data-root", str(tmp_path),
                        "--eval-arc", "HRVanillaTracker", "--out", str(out), *extra], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(out.read_text())
    print(task, {k: v for k, v in res.items() if k != "sequences"})
    if task == "vos":
        assert 0.0 <= res["J&F-Mean"] <= 1.0
    else:
        assert all(0.0 <= v <= 100.0 for k, v in res.items() if k.startswith("PCK@") and np.isfinite(v))
