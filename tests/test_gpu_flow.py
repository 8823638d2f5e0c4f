"""GPU: dense optical flow (test_cfg.flow).  The read-out kernel against its float64 restatement on synthetic lists,
the forward-backward check and the warp against the fixtures recorded from the reference (tests/golden/gen_golden_flow.py) and against
their restatements at the degenerate shapes, the engine on a synthetic bank with a known shift, both trackers' flow call, and the
reference's names under mmpt.models.common.  Bounds: docs/LAB_NOTES.md."""
import math

import numpy as np
import pytest
import torch

from tests import flow_cases as FC
from tests.golden import clips

pytestmark = pytest.mark.gpu
T = torch.from_numpy

FLOWS = ("flow_2x37x53", "flow_2x64x96")
WARP = "flow_warp_2x3x37x53"
VA = dict(typ="VanillaTracker", strides=(1, 1, 1, 4),
          cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=12, step=512, with_first_neighbor=True, batch_step=2))
HR = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1),
          cfg=dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True, batch_step=2))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- 1. the read-out kernel ---------------------------------------------------------------------------------------------------------------
LIST_SHAPES = [(9, 11, 4, 34, 42), (5, 7, 8, 37, 50), (33, 18, 4, 130, 70)]         # (Hf, Wf, scale, h, w): ragged tiles, pad cropped on every side


@pytest.mark.parametrize("renorm", (True, False), ids=("renorm", "raw"))
@pytest.mark.parametrize("Hf,Wf,scale,h,w", LIST_SHAPES)
def test_flow_from_lists_against_float64(dev, Hf, Wf, scale, h, w, renorm):
    """Per pixel |kernel - float64| <= 32 * 2^-24 * (A + P) (k <= 10 fused multiply-adds, a division, a subtraction, three interpolations
    of f32); `valid` with ==; the output lies between two NaN guard bands that stay NaN.  R in {1, 3}, k in {1, 10}, rows in {1, 3}."""
    from fgvc_amd import ops
    top, left = (Hf * scale - h) // 2, (Wf * scale - w) // 2
    assert top >= 1 and left >= 1 and top + h <= Hf * scale and left + w <= Wf * scale
    worst = 0.0
    for R in (1, 3):
        for k in (1, 10):
            for rows in (1, 3):
                idx, wgt = FC.synthetic_lists(rows, Hf, Wf, R, k, seed=100 * R + 10 * k + rows)
                want, wvalid, bound = FC.flow_from_lists_ref(idx, wgt, Hf, Wf, R, scale, (h, w), (left, top), renorm)
                assert 0 < wvalid.mean() < 1 and (bound > 0).all()
                n, g = rows * 2 * h * w, 256
                fbuf = torch.full((n + 2 * g,), float("nan"), device=dev)
                vbuf = torch.full((rows * h * w + 2 * g,), 0xA5, device=dev, dtype=torch.uint8)
                out = (fbuf[g:g + n].view(rows, 2, h, w), vbuf[g:g + rows * h * w].view(rows, h, w))
                flow, valid = ops.flow_from_lists(T(idx).to(dev), T(wgt).to(dev), Hf, Wf, R, scale, (h, w), (left, top), renorm, out=out)
                torch.cuda.synchronize()
                assert bool(torch.isnan(fbuf[:g]).all()) and bool(torch.isnan(fbuf[g + n:]).all())
                assert bool((vbuf[:g] == 0xA5).all()) and bool((vbuf[g + rows * h * w:] == 0xA5).all())
                assert bool(torch.isfinite(flow).all())
                assert np.array_equal(valid.cpu().numpy(), wvalid)
                err = np.abs(flow.cpu().numpy().astype(np.float64) - want)
                ratio = float((err / bound[:, None]).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (R, k, rows, ratio)
    print(f"[flow 1] {Hf}x{Wf} scale {scale} -> {h}x{w} renorm={renorm}: worst |kernel - float64| / bound = {worst:.3f}")


def test_flow_from_lists_equals_topk_coord_rows_at_the_cells(dev):
    """renorm=False at scale-aligned pixels with no pad is get_coord's field minus the cell's own coordinate: the kernel's sum is
    fgvc_topk_coord_rows_f32's, in its order."""
    from fgvc_amd import ops
    Hf, Wf, R, k, scale = 9, 11, 3, 10, 4
    idx, wgt = FC.synthetic_lists(2, Hf, Wf, R, k, seed=5)
    idx[:, :2] = (2 * R + 1) ** 2 // 2                                  # no invalid cell here
    idx_d, wgt_d = T(idx).to(dev), T(wgt).to(dev)
    flow, valid = ops.flow_from_lists(idx_d, wgt_d, Hf, Wf, R, scale, (Hf * scale, Wf * scale), (0, 0), renorm=False)
    fields = ops.topk_coord_rows(idx_d, wgt_d, Hf, Wf, R, scale).view(2, Hf, Wf, 2)
    ys, xs = torch.meshgrid(torch.arange(Hf, device=dev), torch.arange(Wf, device=dev), indexing="ij")
    own = torch.stack([xs, ys], -1).float() * scale
    at = valid[:, ::scale, ::scale].bool()                               # (a valid pixel: its own cell is valid)
    assert float(at.float().mean()) > 0.5
    assert torch.equal(flow[:, :, ::scale, ::scale].permute(0, 2, 3, 1)[at], (fields - own)[at])


# ---- 2. the forward-backward check and the warp -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ("consistency", "fb_abs"))
@pytest.mark.parametrize("name", FLOWS)
def test_flow_consistency_reproduces_reference_masks(dev, golden, name, mode):
    """Both masks == the reference's on every decided pixel; the undecided share is the recorded one and at most 1 %."""
    from fgvc_amd import ops
    g = golden(name)
    _, _, df, db = FC.consistency_both_ref(g["flow_fw"], g["flow_bw"], mode, float(g["diff"]))
    occ_fw, occ_bw = ops.flow_consistency(T(g["flow_fw"]).to(dev), T(g["flow_bw"]).to(dev), mode, float(g["diff"]))
    for key, got, decided in (("occ_fw", occ_fw, df), ("occ_bw", occ_bw, db)):
        want = g[f"{mode}_{key}"]
        got = got.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape and set(np.unique(got)) <= {0.0, 1.0}
        share = 1.0 - decided.mean()
        assert share == float(g[f"{mode}_{key}_undecided"]) and share <= 0.01
        wrong = int(((got != want) & decided).sum())
        print(f"[flow 2] {name} {mode} {key}: {wrong} decided pixels differ, {int((got != want).sum())} in all; undecided share {share:.2e}")
        assert wrong == 0


def _held_to_warp_ref(dev, feat, flow, ac, um, recorded=None):
    from fgvc_amd import ops
    want, ones, mag = FC.warp_ref(feat, flow, ac, um)
    got = ops.warp(T(feat).to(dev), T(flow).to(dev), ac, um).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == feat.shape
    decided = np.broadcast_to((np.abs(ones - 0.9999) >= FC.MASK_MARGIN)[:, None], got.shape) if um else np.ones(got.shape, bool)
    assert 1.0 - decided.mean() <= 0.01
    err, bound = np.abs(got.astype(np.float64) - want), 7 * FC.EPS * mag          # a weight product, a tap product, three sums
    assert (err <= bound)[decided].all(), float((err - bound)[decided].max())
    if recorded is not None:
        assert float(np.abs(got - recorded)[decided].max()) <= 1e-5               # the reference's own f32 run: the bound its restatement is held to
    return float(err[decided].max())


@pytest.mark.parametrize("um", (False, True), ids=("nomask", "mask"))
@pytest.mark.parametrize("ac", (False, True), ids=("ac0", "ac1"))
def test_warp_reproduces_reference(dev, golden, ac, um):
    g = golden(WARP)
    worst = _held_to_warp_ref(dev, g["feat"], g["flow"], ac, um, g[f"out_ac{int(ac)}_m{int(um)}"])
    print(f"[flow 2] warp align_corners={ac} use_mask={um}: max |kernel - float64| = {worst:.2e}")


@pytest.mark.parametrize("N,H,W", [(1, 9, 13), (2, 1, 40), (2, 33, 1)], ids=("n1", "row", "column"))
def test_degenerate_shapes_against_restatements(dev, N, H, W):
    """N = 1, a 1 x W row and an H x 1 column (where the grid is normalised by max(size - 1, 1) = 1): the check against its restatement on
    decided pixels, the warp within its bound."""
    from fgvc_amd import ops
    fw = FC.smooth_field((N, 2, H, W), 31, 2.0)
    bw = -fw + FC.smooth_field((N, 2, H, W), 32, 0.6)
    if H == 1:
        fw[:, 1], bw[:, 1] = fw[:, 1] * 0.1, bw[:, 1] * 0.1                      # stay near the only row
    if W == 1:
        fw[:, 0], bw[:, 0] = fw[:, 0] * 0.1, bw[:, 0] * 0.1
    for mode in ("consistency", "fb_abs"):
        of, ob, df, db = FC.consistency_both_ref(fw, bw, mode, 1.5)
        got_fw, got_bw = ops.flow_consistency(T(fw).to(dev), T(bw).to(dev), mode, 1.5)
        for got, want, decided in ((got_fw, of, df), (got_bw, ob, db)):
            assert decided.mean() >= 0.9
            assert int(((got.cpu().numpy() != want) & decided).sum()) == 0
    feat = FC.smooth_field((N, 3, H, W), 33, 1.0)
    for ac in (False, True):
        for um in (False, True):
            _held_to_warp_ref(dev, feat, fw, ac, um)


# ---- 3. the engine on a synthetic bank ------------------------------------------------------------------------------------------------------------
BANK = dict(T=3, Hf=12, Wf=16, R=3, scale=4, temperature=0.07, topk=10, shift=(2, -1), seed=0)


@pytest.fixture(scope="module")
def banks():
    out = {}
    for C in (64, 256):
        b = FC.shifted_bank(BANK["T"], BANK["Hf"], BANK["Wf"], C, BANK["seed"], BANK["shift"])
        out[C] = (b, {s: FC.largest_off_match_cosine(b, BANK["Hf"], BANK["Wf"], _radius(s), s, BANK["shift"]) for s in (1, 2)})
    return out


def _radius(step):
    """R = 3 reaches the shift of one frame, (2, -1) cells; two frames apart the match is (4, -2) cells away: the smallest window that holds it."""
    return BANK["R"] if step == 1 else 4


@pytest.mark.parametrize("step", (1, 2))
@pytest.mark.parametrize("C,route", [(64, "f32"), (256, "f16x3")])
def test_engine_recovers_a_known_shift(dev, banks, C, route, step):
    """Frame t is frame 0 moved by t * (2, -1) cells: away from the R + shift border flow_fw is (8, -4) * step px and flow_bw its negative,
    within 9 exp(-(1 - c) / 0.07) * 2 R scale sqrt(2) -- nine other list entries, each at most the window's diagonal away and weighted at
    most exp(-(1 - c) / tau) of the match, c the largest off-match cosine of any window (computed here in float64, c < 0.5) -- plus the
    read-out kernel's own bound; occ_fw (fb_abs, 1.5 px) is 1 there."""
    from fgvc_amd import engine
    Hf, Wf, scale, tau, k = (BANK[n] for n in ("Hf", "Wf", "scale", "temperature", "topk"))
    R = _radius(step)
    bank, cs = banks[C]
    c = max(cs[step], 0.0)                                              # (a zero-padded tap scores 0)
    assert c < 0.5
    h, w = Hf * scale, Wf * scale
    cfg = engine.LocalConfig(temperature=tau, topk=k, precede_frames=1, radius=R, with_first=False, with_norm=True)
    stats = {}
    fw, bw, vfw, vbw = engine.flow_fields(T(bank).to(dev), Hf, Wf, cfg, scale, (h, w), (0, 0), step, True, stats)
    assert stats["route"] == route and stats["chunks"] == 1
    n = BANK["T"] - step
    assert fw.shape == bw.shape == (n, 2, h, w) and vfw.shape == vbw.shape == (n, h, w) and vfw.dtype == torch.uint8
    dx, dy = BANK["shift"][0] * step, BANK["shift"][1] * step
    # the interior: R + shift cells from every border (R = 3 and one frame's shift, for either step).  Frame t shows frame 0 moved by at
    # most (T - 1) * shift = (4, -2) cells, so a cell that far inside has its match in every paired frame, in both directions
    mx, my = BANK["R"] + abs(BANK["shift"][0]), BANK["R"] + abs(BANK["shift"][1])
    ys, xs = slice(my * scale, (Hf - 1 - my) * scale + 1), slice(mx * scale, (Wf - 1 - mx) * scale + 1)
    assert ys.stop > ys.start and xs.stop > xs.start
    # the read-out's bound at these pixels: A <= the largest coordinate of the grid (the weights sum to S), P the pixel's own
    tol = 9 * math.exp(-(1 - c) / tau) * 2 * R * scale * math.sqrt(2) + 32 * FC.EPS * 2 * math.hypot(h, w)
    want = torch.tensor([dx * scale, dy * scale], dtype=torch.float32, device=dev).view(1, 2, 1, 1)
    efw = float((fw[:, :, ys, xs] - want).abs().max())
    ebw = float((bw[:, :, ys, xs] + want).abs().max())
    print(f"[flow 3] C={C} {route} step={step}: c = {c:.3f}, tolerance {tol:.3e} px; |flow_fw - shift| = {efw:.3e}, |flow_bw + shift| = {ebw:.3e}")
    assert efw <= tol and ebw <= tol
    assert bool(vfw[:, ys, xs].all()) and bool(vbw[:, ys, xs].all())
    occ_fw, occ_bw = engine.flow_occlusion(fw, bw, "fb_abs", 1.5)
    # a pixel of the interior lands (8, -4) * step px away, at most (4, 2) cells outside the interior on its right and upper side: cells
    # 4 and more from the left border and 2 and more from the lower one, where the backward flow has its match too (frame g + step shows
    # what frame g shows (4, -2) cells or less to the left and below)
    inner = occ_fw[:, :, ys, xs]
    assert occ_fw.shape == (n, 1, h, w) and bool((inner == 1).all()), float(inner.mean())
    assert bool(((occ_bw == 0) | (occ_bw == 1)).all())


def test_engine_chunks_within_the_pair_budget(dev, banks):
    """Two chunks of the affinity run give the bits of one."""
    from fgvc_amd import engine
    Hf, Wf, R, scale = (BANK[n] for n in ("Hf", "Wf", "R", "scale"))
    bank = T(banks[64][0]).to(dev)
    kw = dict(temperature=0.07, topk=10, precede_frames=1, radius=R, with_first=False, with_norm=True)
    one, two = {}, {}
    a = engine.flow_fields(bank, Hf, Wf, engine.LocalConfig(**kw), scale, (46, 61), (1, 2), 1, True, one)
    b = engine.flow_fields(bank, Hf, Wf, engine.LocalConfig(pair_budget=3 * Hf * Wf * 10 * 8, **kw), scale, (46, 61), (1, 2), 1, True, two)
    assert one["chunks"] == 1 and two["chunks"] == 2
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    e = engine.flow_fields(bank[:1], Hf, Wf, engine.LocalConfig(**kw), scale, (46, 61), (1, 2), 1, True)
    assert e[0].shape == (0, 2, 46, 61) and e[2].shape == (0, 46, 61)


# ---- 4. the trackers --------------------------------------------------------------------------------------------------------------------------
def _tracker(dev, spec, **extra):
    import fgvc_amd.mmpt_api as api
    model = api.build_model(dict(type=spec["typ"], backbone=dict(type="ResNet", depth=18, strides=spec["strides"], out_indices=(2,),
                                                                 pool_type="none")),
                            train_cfg=None, test_cfg=api.ConfigDict(**{**spec["cfg"], **extra}))
    torch.manual_seed(4)
    model.init_weights()                                                # Kaiming
    return model.to(dev).eval()


def _clip(dev, seed=6):
    tex = clips.moving_texture(3, 64, 96, seed)                         # (T, 3, h, w) int8, drifting by (3, -2) px a frame
    floats = (T(tex).float() / 32).to(dev)
    u8 = T((tex.astype(np.int16) + 128).astype(np.uint8)).permute(0, 2, 3, 1).contiguous().to(dev)      # (T, h, w, 3)
    return floats, u8


def _by_hand(model, imgs, fc):
    from fgvc_amd import engine
    frames, (h, w), pad = model._label_frames(imgs)
    feats, Hf, Wf = model._label_feats(frames)
    rows, lc = model._window_rows(feats, Hf, Wf, fc.radius, "flow")
    return engine.flow_fields(rows, Hf, Wf, lc, frames.shape[-1] // Wf, (h, w), (pad[0], pad[2]), fc.step, fc.renorm)


@pytest.mark.parametrize("spec", [VA, HR], ids=["vanilla", "hr"])
def test_model_flow_call(dev, spec):
    from fgvc_amd import metrics
    floats, u8 = _clip(dev)
    n, h, w = 2, 64, 96
    model = _tracker(dev, spec, flow=dict(type="window", occlusion="fb_abs"), input=dict(type="rgb8"))
    imgs = floats.transpose(0, 1)[None, None]                           # (1, 1, 3, T, h, w)
    out = model(test_mode=True, imgs=imgs)
    assert sorted(out) == ["flow_bw", "flow_fw", "occ_bw", "occ_fw", "valid_bw", "valid_fw"]
    for key, shape, dt in (("flow_fw", (n, 2, h, w), torch.float32), ("flow_bw", (n, 2, h, w), torch.float32),
                           ("valid_fw", (n, h, w), torch.uint8), ("valid_bw", (n, h, w), torch.uint8),
                           ("occ_fw", (n, 1, h, w), torch.float32), ("occ_bw", (n, 1, h, w), torch.float32)):
        t = out[key]
        assert t.is_cuda and tuple(t.shape) == shape and t.dtype == dt and bool(torch.isfinite(t.float()).all()), key
    assert model.flow_stats["route"] in ("f32", "f16x3") and model.flow_stats["chunks"] == 1
    # ... the engine called by hand on the same bank, bit for bit
    fc = model._flow()
    hand = _by_hand(model, imgs, fc)
    for key, t in zip(("flow_fw", "flow_bw", "valid_fw", "valid_bw"), hand):
        assert torch.equal(out[key], t), key
    # ... the clip reversed in time: the same pairs in the other role
    rev = model(test_mode=True, imgs=torch.flip(imgs, (3,)))
    assert torch.equal(rev["flow_fw"], torch.flip(out["flow_bw"], (0,))) and torch.equal(rev["flow_bw"], torch.flip(out["flow_fw"], (0,)))
    assert torch.equal(rev["occ_fw"], torch.flip(out["occ_bw"], (0,)))
    # ... step = 2: one pair
    two = _tracker(dev, spec, flow=dict(type="window", step=2))(test_mode=True, imgs=imgs)
    assert sorted(two) == ["flow_bw", "flow_fw", "valid_bw", "valid_fw"] and two["flow_fw"].shape == (1, 2, h, w)
    # ... raw uint8 frames through test_cfg.input: the call on ops.frames_to_lab of them
    from fgvc_amd import ops
    raw = model(test_mode=True, imgs=u8[None, None])
    lab = ops.frames_to_lab(u8)                                          # (T, 3, h, w)
    same = model(test_mode=True, imgs=lab.transpose(0, 1)[None, None])
    for key in out:
        assert torch.equal(raw[key], same[key]), key
    drift = torch.tensor([3.0, -2.0], device=dev).view(1, 2, 1, 1).expand(n, 2, h, w)
    r = metrics.flow_epe(out["flow_fw"], drift, out["valid_fw"])
    med = float((out["flow_fw"] - drift).pow(2).sum(1).sqrt().median())
    print(f"[flow 4] {spec['typ']} Kaiming weights, 3 x 64 x 96 moving texture: median end-point error {med:.3f} px, mean {r['epe']:.3f} px, "
          f"<1px {r['1px']:.3f}, <3px {r['3px']:.3f}; occ_fw mean {float(out['occ_fw'].mean()):.3f} (measured, not asserted)")


@pytest.mark.parametrize("spec", [VA, HR], ids=["vanilla", "hr"])
def test_model_flow_routing_and_refusals(dev, spec):
    floats, _ = _clip(dev)
    imgs = floats.transpose(0, 1)[None, None]
    plain = _tracker(dev, spec)
    with pytest.raises(TypeError):                                      # without the key, imgs= alone is today's mask call without its labels
        plain(test_mode=True, imgs=imgs)
    with pytest.raises(ValueError, match="test_cfg.flow"):
        plain.forward_test_flow(imgs)
    both = _tracker(dev, spec, flow=dict(type="window"), occlusion=dict(type="cycle"))
    with pytest.raises(ValueError, match="occlusion"):
        both(test_mode=True, imgs=imgs)
    rm = _tracker(dev, spec, flow=dict(type="window", occlusion="range_map"))
    with pytest.raises(NotImplementedError, match="range_map"):
        rm(test_mode=True, imgs=imgs)
    if spec is HR:                                                      # its pad unit is its own `stride` (2), the encoder's pitch is 4:
        odd = torch.zeros(1, 1, 3, 3, 64, 98, device=dev)               # 98 columns over 25 features is no whole pitch
        with pytest.raises(NotImplementedError, match="pitch"):
            _tracker(dev, spec, flow=dict(type="window"))(test_mode=True, imgs=odd)
    # with the key set, the mask call is still the mask call
    model = _tracker(dev, spec, flow=dict(type="window"))
    seg = torch.zeros(1, 64, 96, dtype=torch.uint8)
    seg[0, 10:30, 20:50] = 1
    masks = model(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(64, 96))])
    want = plain(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(64, 96))])
    assert isinstance(masks, list) and np.array_equal(masks[0], want[0])


# ---- 5. the reference's names ---------------------------------------------------------------------------------------------------------------------
def test_mmpt_names_reproduce_fixtures(dev, golden):
    import fgvc_amd
    fgvc_amd.install_as_mmpt()
    import mmpt.models.common as C
    from mmpt.models import build_operators
    assert getattr(C, "_fgvc_amd", False)
    g = golden(FLOWS[0])
    fw, bw = T(g["flow_fw"]).to(dev), T(g["flow_bw"]).to(dev)
    for mode, kw in (("consistency", {}), ("fb_abs", dict(diff=1.5)), ("fb_abs", dict(diff=1.5, warp_cfg=dict(type="Warp", align_corners=True)))):
        out = C.occlusion_estimation(fw, bw, mode, **kw)
        _, _, df, db = FC.consistency_both_ref(g["flow_fw"], g["flow_bw"], mode, 1.5)
        assert sorted(out) == ["occ_bw", "occ_fw"]
        for key, decided in (("occ_fw", df), ("occ_bw", db)):
            assert int(((out[key].cpu().numpy() != g[f"{mode}_{key}"]) & decided).sum()) == 0
    assert torch.equal(C.forward_backward_consistency(fw, bw), C.occlusion_estimation(fw, bw)["occ_fw"])
    assert torch.equal(C.forward_backward_absdiff(bw, fw, diff=1.5), C.occlusion_estimation(fw, bw, "fb_abs")["occ_bw"])
    w = golden(WARP)
    op = build_operators(dict(type="Warp"))
    got = op(T(w["feat"]).to(dev), T(w["flow"]).to(dev)).cpu().numpy()
    _, ones, _ = FC.warp_ref(w["feat"], w["flow"], False, True)
    decided = np.broadcast_to((np.abs(ones - 0.9999) >= FC.MASK_MARGIN)[:, None], got.shape)
    assert float(np.abs(got - w["out_ac0_m1"])[decided].max()) <= 1e-5
    grid = C.coords_grid_warp(fw)
    assert grid.shape == (2, 37, 53, 2) and grid.is_cuda
    for bad in (lambda: C.occlusion_estimation(fw.double(), bw.double()), lambda: op(T(w["feat"]).to(dev).double(), T(w["flow"]).to(dev).double())):
        with pytest.raises(TypeError, match="float32"):
            bad()
    with pytest.raises(NotImplementedError, match="range_map"):
        C.occlusion_estimation(fw, bw, "range_map")
