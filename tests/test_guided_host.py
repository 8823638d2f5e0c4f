"""CPU tests of the edge-aware read-out's rule (engine.guided_readout_host, float64 torch) and of the test_cfg.readout parser: the rule
against an independently written spatial Gaussian filter, its invariances, its refusals, the disc prototype, and the condition the GPU
cases put on their own inputs (at most 0.5 % of the pixels undecided by the f32 error bound)."""
import math

import numpy as np
import pytest
import torch

from tests import guided_cases as G


def _engine():
    from fgvc_amd import engine
    return engine


def _spatial_gaussian(lab, Hf, Wf, pad_shape, pad, out_shape, radius, sigma):
    """Written without looking at the rule's code: per output pixel, loops in numpy over the window around the nearest cell centre."""
    (hp, wp), (lw, uw, lh, uh), (h0, w0) = pad_shape, pad, out_shape
    hu, wu = hp - lh - uh, wp - lw - uw
    L = lab.double().numpy().reshape(Hf, Wf, -1)
    out = np.zeros((h0, w0, L.shape[-1]))
    for y in range(h0):
        py = min(max((y + 0.5) * hu / h0 - 0.5, 0.0), hu - 1.0) + lh
        fy = (py + 0.5) * Hf / hp - 0.5
        ci = math.floor(fy + 0.5)
        for x in range(w0):
            px = min(max((x + 0.5) * wu / w0 - 0.5, 0.0), wu - 1.0) + lw
            fx = (px + 0.5) * Wf / wp - 0.5
            cj = math.floor(fx + 0.5)
            num, den = 0.0, 0.0
            for i in range(max(ci - radius, 0), min(ci + radius, Hf - 1) + 1):
                for j in range(max(cj - radius, 0), min(cj + radius, Wf - 1) + 1):
                    w = math.exp(-((i - fy) ** 2 + (j - fx) ** 2) / (2 * sigma ** 2))
                    num = num + w * L[i, j]
                    den += w
            out[y, x] = num / den
    return out


@pytest.mark.parametrize("pad, out_shape, radius", [((0, 0, 0, 0), (20, 28), 2), ((3, 0, 1, 0), (23, 17), 1), ((0, 2, 0, 3), (11, 31), 3)])
def test_wide_range_sigma_and_constant_guide_are_a_spatial_gaussian(pad, out_shape, radius):
    engine = _engine()
    Hf, Wf, hp, wp = 5, 7, 20, 28
    g = torch.Generator().manual_seed(radius)
    lab = torch.rand(1, Hf * Wf, 3, generator=g)
    guide = torch.rand(1, 3, hp, wp, generator=g)
    want = _spatial_gaussian(lab[0], Hf, Wf, (hp, wp), pad, out_shape, radius, 1.3)
    wide = engine.guided_readout_host(lab, guide, Hf, Wf, (hp, wp), pad, out_shape, False, radius, 1.3, 1e6)
    assert np.abs(wide.values[0].numpy() - want).max() < 1e-10             # |I - Gc|^2 / 2e12 <= 2e-12 in the exponent
    flat = engine.guided_readout_host(lab, torch.full_like(guide, 0.37), Hf, Wf, (hp, wp), pad, out_shape, False, radius, 1.3, 0.1)
    assert np.abs(flat.values[0].numpy() - want).max() < 1e-12
    assert np.array_equal(flat.ids[0].numpy(), want.argmax(-1))
    top = np.sort(want, -1)
    assert np.array_equal(flat.conf[0].numpy(), np.rint(255 * np.clip(top[..., -1] - top[..., -2], 0, 1)).astype(np.uint8))


def test_a_constant_added_to_every_exponent_changes_nothing():
    engine = _engine()
    case = G.CASES[1]
    lab, guide = G.make_inputs(case)
    Hf, Wf, pad_shape, pad, out = G.geometry(case)
    a = engine.guided_readout_host(lab, guide, Hf, Wf, pad_shape, pad, out, True, 2, 1.0, 0.1)
    b = engine.guided_readout_host(lab, guide, Hf, Wf, pad_shape, pad, out, True, 2, 1.0, 0.1, shift=37.5)
    assert float((a.values - b.values).abs().max()) < 1e-12 and torch.equal(a.ids, b.ids)
    assert float((b.e_min - a.e_min - 37.5).abs().max()) < 1e-9
    # the normalised weights never lose a pixel: with a tiny sigma_range every value is still a convex combination of the labels
    c = engine.guided_readout_host(lab, guide, Hf, Wf, pad_shape, pad, out, False, 2, 1.0, 1e-4)
    assert bool(torch.isfinite(c.values).all()) and float(c.values.min()) >= 0.0 and float(c.values.max()) <= 1.0 + 1e-12


def test_normalisation_uses_the_grid_extremes_and_skips_non_positive_channels():
    engine = _engine()
    Hf, Wf, hp, wp = 5, 7, 20, 28
    g = torch.Generator().manual_seed(3)
    lab = torch.rand(1, Hf * Wf, 3, generator=g) * 0.5 + 0.2
    lab[..., 1] = -lab[..., 1]                                              # maximum <= 0: left alone
    guide = torch.rand(1, 3, hp, wp, generator=g)
    got = engine.guided_readout_host(lab, guide, Hf, Wf, (hp, wp), (0, 0, 0, 0), (20, 28), True, 1, 1.0, 0.2)
    L = lab.double()
    mn, mx = L.amin(1, keepdim=True), L.amax(1, keepdim=True)
    pre = torch.where(mx > 0, (L - mn) / (mx - mn + 1e-12), L)
    want = engine.guided_readout_host(pre.float().double(), guide, Hf, Wf, (hp, wp), (0, 0, 0, 0), (20, 28), False, 1, 1.0, 0.2)
    assert float((got.values - want.values).abs().max()) < 1e-6             # (pre went through f32 once)
    assert float(got.values[..., 1].max()) <= 0.0 and float(got.values[..., 0].max()) <= 1.0 + 1e-12
    one = engine.guided_readout_host(lab[..., :1], guide, Hf, Wf, (hp, wp), (0, 0, 0, 0), (20, 28), True, 1, 1.0, 0.2)
    assert bool((one.conf == 255).all()) and bool((one.ids == 0).all()) and bool(torch.isinf(one.margin).all())


def test_refusals_raise_by_name():
    engine = _engine()
    lab, guide = torch.rand(1, 35, 2), torch.rand(1, 3, 20, 28)
    args = (5, 7, (20, 28), (0, 0, 0, 0), (20, 28), True)
    for radius in (0, 4, 2.0, True):
        with pytest.raises(ValueError, match="radius"):
            engine.guided_readout_host(lab, guide, *args, radius, 1.0, 0.1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="sigma_space"):
            engine.guided_readout_host(lab, guide, *args, 2, bad, 0.1)
        with pytest.raises(ValueError, match="sigma_range"):
            engine.guided_readout_host(lab, guide, *args, 2, 1.0, bad)
    with pytest.raises(ValueError, match="does not divide"):
        engine.guided_readout_host(torch.rand(1, 6 * 7, 2), guide, 6, 7, (20, 28), (0, 0, 0, 0), (20, 28), True, 2, 1.0, 0.1)
    with pytest.raises(ValueError, match="does not divide"):
        engine.guided_readout_host(torch.rand(1, 5 * 8, 2), guide, 5, 8, (20, 28), (0, 0, 0, 0), (20, 28), True, 2, 1.0, 0.1)


def test_parse_readout():
    engine = _engine()
    assert engine.parse_readout(None) is None and engine.parse_readout(dict(type="bilinear")) is None
    rc = engine.parse_readout(dict(type="guided"))
    assert (rc.type, rc.radius, rc.sigma_space, rc.sigma_range) == ("guided", 2, 1.0, 0.1)
    rc = engine.parse_readout(dict(type="guided", radius=3, sigma_space=2, sigma_range=0.05))
    assert (rc.radius, rc.sigma_space, rc.sigma_range) == (3, 2.0, 0.05)
    with pytest.raises(ValueError, match="type='box'"):
        engine.parse_readout(dict(type="box"))
    with pytest.raises(ValueError, match="type=None"):
        engine.parse_readout(dict(radius=2))
    with pytest.raises(ValueError, match="sigma"):
        engine.parse_readout(dict(type="guided", sigma=1.0))
    with pytest.raises(ValueError, match="radius"):
        engine.parse_readout(dict(type="bilinear", radius=2))
    with pytest.raises(ValueError, match="radius=4"):
        engine.parse_readout(dict(type="guided", radius=4))
    with pytest.raises(ValueError, match="sigma_range"):
        engine.parse_readout(dict(type="guided", sigma_range=0))
    with pytest.raises(TypeError, match="test_cfg.readout"):
        engine.parse_readout("guided")


@pytest.mark.parametrize("stride", [4, 8])
@pytest.mark.parametrize("blur", [0, 1, 2])
def test_disc_prototype_beats_the_bilinear_readout(stride, blur):
    """The disc of the issue: guided J strictly above the plain read-out's J, recomputed here; 1.0 at stride 4."""
    engine = _engine()
    truth, lab, guide = G.disc_inputs(stride, blur, noise=0.02)
    H, W = G.DISC_H, G.DISC_W
    Hf, Wf = H // stride, W // stride
    plain = G.jaccard(G.bilinear_readout(lab[0], Hf, Wf, H, W).numpy() == 1, truth)
    got = engine.guided_readout_host(lab, guide, Hf, Wf, (H, W), (0, 0, 0, 0), (H, W), True, 2, 1.0, 0.1)
    guided = G.jaccard(got.ids[0].numpy() == 1, truth)
    print(f"disc stride {stride} blur {blur}: bilinear J = {plain:.4f}, guided J = {guided:.4f}, smallest margin {float(got.margin.min()):.2e}")
    assert guided > plain
    if stride == 4:
        assert guided == 1.0


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c["name"])
def test_gpu_cases_satisfy_their_own_input_condition(case):
    """What the GPU comparison asks of its inputs, checked on the float64 rule alone: labels in [0, 1], extremes either apart or equal,
    and at most 0.5 % of the pixels with a margin the f32 bound cannot decide."""
    lab, guide, ref, B = G.reference(case)
    assert float(lab.min()) >= 0.0 and float(lab.max()) <= 1.0 and bool(torch.isfinite(guide).all())
    spread = lab.amax(1) - lab.amin(1)
    assert bool(((spread >= 1e-30) | (spread == 0)).all())
    if case["C"] >= 3 and case["labels"] == "blobs":
        assert float(lab[..., 1].max()) <= 0.0                              # the channel whose maximum is <= 0
    dec = G.decided(case, ref, B)
    excluded = 1.0 - float(dec.double().mean())
    print(f"{case['name']}: B = {B:.3e}, E = {float(ref.e_min.max()):.3f}, excluded share {excluded:.5f}")
    assert B < 0.25 and excluded <= G.EXCLUDED_MAX
    if case["labels"] == "ties":
        v = ref.values
        lead = (v[..., 1] > v[..., [0, 3]].max(-1).values) & dec
        assert int(lead.sum()) > 100 and bool((ref.ids[lead] == 1).all())   # the tied pair leads somewhere, and the first of it wins
