"""CPU: the forward-backward visibility read-out (test_cfg.occlusion) -- the oracle's chain against the goldens
recorded from the genuine reference (tests/golden/gen_golden_occlusion.py), the configuration's parsing and refusals, and the occluder of
the synthetic dataset.  No compute calls: there is no GPU here."""
import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O

T = torch.from_numpy

HR_CFG = dict(radius=4, topk=6, temperature=0.07)
FIXTURES = [("occlusion_hr_5x48x64", (1, 2, 1, 1), HR_CFG), ("occlusion_hr_mixed_5x48x64", (1, 2, 1, 1), HR_CFG),
            ("occlusion_vanilla_5x64x64", (1, 1, 1, 4), dict(radius=6, topk=10, temperature=0.07))]


def _groups(g):
    """[(s, columns)] of a fixture, in the order of its predicted trajectories."""
    qp = T(g["out_query_points"] if "out_query_points" in g else g["query_points"])[0]
    return qp, [(s, (qp[:, 0] == s).nonzero().flatten()) for s in sorted(set(int(t) for t in qp[:, 0]))]


@pytest.mark.parametrize("name,strides,kw", FIXTURES)
def test_oracle_chain_reproduces_reference_backtracked_points(golden, name, strides, kw):
    """O.hr_forward_test_forward(precede_frames=1) on the reversed sub-clips [f, ..., s], started at the reference's own x_f, lands where the
    reference's forward_test_forward landed: the bound tests/test_oracle.py holds `forward_coords` to (2e-3 px)."""
    g = golden(name)
    rgbs = T(g["rgbs"])
    h, w = rgbs.shape[-2:]
    net = O.ResNet18(strides, 2, "none")
    net.load_state_dict(O.seeded_resnet_state(int(g["seed"]), strides, "none"))
    with torch.no_grad():
        feats = net.eval()(rgbs[0])
    assert w // feats.shape[-1] == int(g["scale"])
    x, back, scored = T(g["out_traj_pred"])[0], T(g["back"]), T(g["scored"])
    qp, groups = _groups(g)
    n = 0
    for s, cols in groups:
        for f in range(s + 1, rgbs.shape[1]):
            out = O.hr_forward_test_forward(feats[list(range(f, s - 1, -1))], torch.flip(x[f, cols].float().t(), (0,)), h, w,
                                            precede_frames=1, **kw)
            assert bool(scored[f, cols].all())
            assert float((out[:, :, -1].t() - back[f, cols].double()).abs().max()) < 2e-3, (name, s, f)
            n += cols.numel()
    assert n == int(scored.sum())
    # what the fixture promises the GPU test: both classes hold a quarter of the scored entries, under a tenth lie in the excluded band
    err, flags = T(g["err"]), T(g["flags"]).bool()
    thresh_px = float(g["cycle_thresh"]) * int(g["scale"])
    assert torch.equal(flags[scored], err[scored] <= thresh_px)
    assert min(int(flags[scored].sum()), int((~flags[scored]).sum())) >= n / 4
    assert int(((err[scored] - thresh_px).abs() <= float(g["band_px"])).sum()) < 0.1 * n
    for s, cols in groups:                                          # the query frame: visible, err 0; before it: not scored
        assert bool(flags[s, cols].all()) and float(err[s, cols].abs().max()) == 0 and bool(torch.isinf(err[:s, cols]).all())


def test_occlusion_config_parsing():
    from fgvc_amd import engine
    assert engine.parse_occlusion(None, 12) is None
    assert engine.parse_occlusion(dict(type="cycle"), 12) == engine.OcclusionConfig(1.0, 12)
    assert engine.parse_occlusion(dict(type="cycle", cycle_thresh=2.5, radius=None), 7) == engine.OcclusionConfig(2.5, 7)
    assert engine.parse_occlusion(dict(type="cycle", radius=3), 7) == engine.OcclusionConfig(1.0, 3)
    for bad in (dict(type="flow"), dict(cycle_thresh=1.0), dict(type="cycle", thresh=1.0), dict(type="cycle", cycle_thresh=-1),
                dict(type="cycle", cycle_thresh=float("nan")), dict(type="cycle", radius=-1)):
        with pytest.raises(ValueError):
            engine.parse_occlusion(bad, 12)
    with pytest.raises(TypeError):
        engine.parse_occlusion("cycle", 12)
    # backward_fields takes the one-slot plan only: (g, g - 1) for every g
    lc = engine.LocalConfig(temperature=0.07, topk=6, precede_frames=1, radius=4, with_first=False)
    assert engine.plan_local_clip(5, lc, 24 * 32).pairs == [(1, 0), (2, 1), (3, 2), (4, 3)]
    with pytest.raises(ValueError):
        engine.backward_fields(torch.zeros(3, 4, 32), 2, 2, engine.LocalConfig(temperature=0.07, topk=6, precede_frames=2, with_first=False), 2)


def _model(typ, **test_cfg):
    import fgvc_amd.mmpt_api as api
    return api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,), pool_type="none")),
                           train_cfg=None, test_cfg=api.ConfigDict(**test_cfg)).eval()


def test_trackers_read_the_key_and_refuse_what_is_out_of_scope():
    from fgvc_amd import dist, engine
    base = dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True)
    hr = _model("HRVanillaTracker", **base, occlusion=dict(type="cycle"))
    assert hr._occlusion() == engine.OcclusionConfig(1.0, 4) and hr.last_cycle_error is None          # radius: infer_radius
    assert _model("HRVanillaTracker", occlusion=dict(type="cycle"))._occlusion().radius == 12            # neighbor_range's default 24
    va = _model("VanillaTracker", **base, occlusion=dict(type="cycle", cycle_thresh=0.5))
    assert va._occlusion() == engine.OcclusionConfig(0.5, 4)                                             # radius: neighbor_range // 2
    assert _model("VanillaTracker", **base)._occlusion() is None and _model("HRVanillaTracker", **base, occlusion=None)._occlusion() is None
    with pytest.raises(ValueError):
        _model("VanillaTracker", **base, occlusion=dict(type="flow"))._occlusion()
    with pytest.raises(ValueError):                                    # no neighbor_range to derive the window from
        _model("VanillaTracker", topk=6, occlusion=dict(type="cycle"))._occlusion()
    assert _model("VanillaTracker", topk=6, occlusion=dict(type="cycle", radius=5))._occlusion().radius == 5
    # the calls that have no visibility output say so instead of returning zeros
    imgs, seg, meta = torch.zeros(1, 1, 3, 2, 16, 16), torch.zeros(1, 16, 16, dtype=torch.uint8), [dict(original_shape=(16, 16))]
    for m in (hr, va):
        with pytest.raises(NotImplementedError, match="occlusion"):
            m(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
        with pytest.raises(NotImplementedError, match="occlusion"):
            m(test_mode=True, imgs=imgs, ref_seg_map=torch.zeros(1, 2, 16, 16), img_meta=meta)
    with pytest.raises(NotImplementedError, match="occlusion"):
        hr.forward_test_forward(imgs, None, None, torch.zeros(1, 2, 3))

    class Backend:
        model = va
    with pytest.raises(NotImplementedError, match="occlusion"):
        dist.track_points_sharded(Backend(), torch.zeros(2, 3, 16, 16), torch.zeros(1, 3), va.engine_config())


def _sample_as_before(n, frames, size, points, query_mode, seed, i):
    """SyntheticTapVid.__getitem__ as it was before the `occluder` argument existed, restated."""
    g = torch.Generator().manual_seed(seed * 1000 + i)
    T_, h, w, P = frames, size[0], size[1], points
    pad = 2 * T_
    base = torch.nn.functional.interpolate(torch.randn(1, 3, (h + 2 * pad) // 8 + 1, (w + 2 * pad) // 8 + 1, generator=g),
                                           size=(h + 2 * pad, w + 2 * pad), mode="bilinear", align_corners=False)[0]
    base = base + 0.25 * torch.randn(base.shape, generator=g)
    vx, vy = int(torch.randint(-2, 3, (1,), generator=g)), int(torch.randint(-2, 3, (1,), generator=g))
    rgbs = torch.stack([base[:, pad - vy * t: pad - vy * t + h, pad - vx * t: pad - vx * t + w] for t in range(T_)], 0)
    t0 = torch.zeros(P) if query_mode == "first" else torch.randint(0, max(1, T_ // 2), (P,), generator=g).float()
    margin = 2 * T_ + 8
    x0 = torch.rand(P, generator=g) * (w - 2 * margin) + margin
    y0 = torch.rand(P, generator=g) * (h - 2 * margin) + margin
    ts = torch.arange(T_).view(T_, 1).float()
    traj = torch.stack([x0.view(1, P) + vx * (ts - t0.view(1, P)) + 0 * ts, y0.view(1, P) + vy * (ts - t0.view(1, P))], -1)
    qp = torch.stack([t0, x0, y0], -1)
    vis = (ts >= t0.view(1, P)).float()
    return dict(rgbs=rgbs.unsqueeze(0), query_points=qp.unsqueeze(0), trajectories=traj.unsqueeze(0), visibilities=vis.unsqueeze(0))


@pytest.mark.parametrize("query_mode", ["first", "random"])
def test_synthetic_tapvid_occluder(query_mode):
    from fgvc_amd.datasets import SyntheticTapVid
    kw = dict(n_videos=3, frames=8, size=(64, 96), points=24, query_mode=query_mode, seed=3)
    plain, default, occ = SyntheticTapVid(occluder=False, **kw), SyntheticTapVid(**kw), SyntheticTapVid(occluder=True, **kw)
    assert plain.occluder_box(0) is None
    hidden = 0
    for i in range(3):
        a, d, b = plain[i], default[i], occ[i]
        want = _sample_as_before(kw["n_videos"], kw["frames"], kw["size"], kw["points"], query_mode, kw["seed"], i)
        for k in ("rgbs", "query_points", "trajectories", "visibilities"):
            assert torch.equal(a[k], want[k]) and torch.equal(d[k], want[k]), k         # occluder=False (the default): today's sample
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        for k in ("query_points", "trajectories"):
            assert torch.equal(a[k], b[k])
        t_on, y0, y1, x0, x1 = occ.occluder_box(i)
        assert t_on == 4 and 0 <= y0 < y1 <= 64 and 0 <= x0 < x1 <= 96
        ra, rb = a["rgbs"][0], b["rgbs"][0]
        assert torch.equal(ra[:t_on], rb[:t_on])                                         # the early frames are untouched
        outside = torch.ones(64, 96, dtype=torch.bool)
        outside[y0:y1, x0:x1] = False
        assert torch.equal(ra[t_on:][..., outside], rb[t_on:][..., outside])
        assert not torch.equal(ra[t_on:, :, y0:y1, x0:x1], rb[t_on:, :, y0:y1, x0:x1])
        assert all(torch.equal(rb[t, :, y0:y1, x0:x1], rb[t_on, :, y0:y1, x0:x1]) for t in range(t_on, 8))      # static
        tr, va, vb = b["trajectories"][0], a["visibilities"][0], b["visibilities"][0]
        under = (tr[..., 0] >= x0) & (tr[..., 0] <= x1 - 1) & (tr[..., 1] >= y0) & (tr[..., 1] <= y1 - 1)
        under[:t_on] = False
        assert torch.equal(vb, va * (~under).float())
        qt = b["query_points"][0, :, 0].long()
        assert bool((vb[qt, torch.arange(24)] == 1).all())                               # query points stay visible
        hidden += int(under.sum())
    assert hidden > 0
