"""CPU: the YUV 4:2:0 output contract (datasets.rgb8_to_yuv420, ops.rgb_to_yuv_coefficients, datasets.pack_yuv420).

datasets.rgb8_to_yuv420 equals the numpy float32 chain of tests/yuv_out_cases.py byte for byte; against the same formulas in float64 it is off
by at most 1 and only within 1e-3 of a rounding boundary; known answers, the legal range, the round trip through the project's decoder,
packing and Y4M files -- and a table of deliberate mutations, each of which a named case must catch."""
import math

import numpy as np
import pytest
import torch

from fgvc_amd import datasets, ops
from tests import yuv_out_cases as OC

SETS = OC.frame_sets()
CASES = OC.cases()


@pytest.fixture(scope="module")
def restated():
    """case id -> datasets.rgb8_to_yuv420's (y, u, v) as numpy arrays, computed once and never written to."""
    memo = {}

    def get(cid):
        if cid not in memo:
            name, m, r, s = CASES[cid]
            memo[cid] = tuple(p.numpy() for p in datasets.rgb8_to_yuv420(SETS[name], m, r, s))
        return memo[cid]

    return get


def test_coefficients_invert_the_decoders():
    for m in OC.MATRICES:
        for r in OC.RANGES:
            got = ops.rgb_to_yuv_coefficients(m, r)
            assert got == OC.coefficients_f64(m, r)
            kr, kg, kb, y_off, sy, cu, cv = got
            d_off, cy, crv, cgu, cgv, cbu = ops.yuv_coefficients(m, r)
            assert y_off == d_off and abs(kr + kg + kb - 1.0) < 1e-15
            assert abs(sy * cy - 1.0) < 1e-15 and abs(cu * cbu - 1.0) < 1e-15 and abs(cv * crv - 1.0) < 1e-15
    with pytest.raises(ValueError, match="matrix"):
        ops.rgb_to_yuv_coefficients("bt2020")
    with pytest.raises(ValueError, match="range"):
        ops.rgb_to_yuv_coefficients("bt601", "tv")


@pytest.mark.parametrize("cid", list(CASES))
def test_restatement_equals_the_float32_chain(restated, cid):
    name, m, r, s = CASES[cid]
    T, h, w, _ = SETS[name].shape
    got = restated(cid)
    want = OC.encode(SETS[name].numpy(), m, r, s, np.float32)
    for g, x, shape in zip(got, want, ((T, h, w), (T, (h + 1) // 2, (w + 1) // 2), (T, (h + 1) // 2, (w + 1) // 2))):
        assert g.dtype == np.uint8 and g.shape == shape
        assert np.array_equal(g, x), (cid, int((g != x).sum()))


@pytest.mark.parametrize("kind", ["texture", "random"])
@pytest.mark.parametrize("m,r,s", OC.COMBOS, ids=["-".join(c) for c in OC.COMBOS])
def test_float64_guard(restated, kind, m, r, s):
    """Against the float64 chain: at most 1 apart everywhere, equal wherever the float64 value is further than NEAR = 1e-3 from a rounding
    boundary (the float32 chain's error: about 8 rounded operations below 256, 1.2e-4).  A case is one source and one setting over all the
    sizes of the list -- on a 1 x 1 frame a single byte is a third of the frame -- and at most 1 % of its bytes may be excused, so the guard
    cannot hide a failure (the float64 chain alone leaves about 0.2 % that close)."""
    total = excused = 0
    for name in SETS:
        if not name.startswith(kind + "_"):
            continue
        values = OC.encode_values(SETS[name].numpy(), m, r, s, np.float64)
        for g, x in zip(restated(f"{name}-{m}-{r}-{s}"), values):
            d = np.abs(g.astype(np.int64) - OC.to_bytes(x).astype(np.int64))
            near = np.abs(x - np.floor(x) - 0.5) <= OC.NEAR
            assert int(d.max()) <= 1, (name, int(d.max()))
            assert not (d[~near] > 0).any(), (name, int((d[~near] > 0).sum()))
            total += d.size
            excused += int(near.sum())
    print(f"[yuv-out] {kind}-{m}-{r}-{s}: {excused} of {total} bytes within {OC.NEAR} of a rounding boundary")
    assert total > 20000 and excused <= 0.01 * total, (excused, total)


def test_float32_chain_stays_within_its_margin():
    """What NEAR rests on: the float32 values are within 1.2e-4 of the float64 ones."""
    worst = 0.0
    for cid, (name, m, r, s) in CASES.items():
        if OC.is_natural(name):
            a = OC.encode_values(SETS[name].numpy(), m, r, s, np.float32)
            b = OC.encode_values(SETS[name].numpy(), m, r, s, np.float64)
            worst = max(worst, max(float(np.abs(x.astype(np.float64) - z).max()) for x, z in zip(a, b)))
    print(f"[yuv-out] largest |float32 - float64| value: {worst:.3e}")
    assert worst <= 8 * 2.0 ** -24 * 256


@pytest.mark.parametrize("m,r,s", OC.COMBOS, ids=["-".join(c) for c in OC.COMBOS])
def test_grey_has_neutral_chroma(m, r, s):
    grey = torch.arange(256, dtype=torch.uint8)[:, None].expand(256, 3)
    y, u, v = datasets.rgb8_to_yuv420(OC.constant_frames(grey.numpy(), 3, 5), m, r, s)
    assert bool((u == 128).all()) and bool((v == 128).all())
    y_off, cy, _ = OC.RANGES[r]
    want = np.rint(y_off + np.arange(256, dtype=np.float64) / cy).astype(np.uint8)
    assert np.array_equal(y.numpy(), np.broadcast_to(want[:, None, None], (256, 3, 5)))


@pytest.mark.parametrize("s", OC.SITINGS)
@pytest.mark.parametrize("m", list(OC.BARS))
def test_limited_range_colour_bars(m, s):
    rgb = list(OC.BARS[m])
    y, u, v = datasets.rgb8_to_yuv420(OC.constant_frames(rgb, 4, 6), m, "limited", s)
    for i, c in enumerate(rgb):
        got = (set(y[i].flatten().tolist()), set(u[i].flatten().tolist()), set(v[i].flatten().tolist()))
        assert got == tuple({x} for x in OC.BARS[m][c]), (m, s, c, got)


@pytest.mark.parametrize("cid", [c for c in CASES if "-limited-" in c])
def test_limited_range_stays_legal(restated, cid):
    y, u, v = restated(cid)
    assert 16 <= int(y.min()) and int(y.max()) <= 235
    for c in (u, v):
        assert 16 <= int(c.min()) and int(c.max()) <= 240


@pytest.mark.parametrize("m,r,s", OC.COMBOS, ids=["-".join(c) for c in OC.COMBOS])
def test_round_trip_on_constant_colours(m, r, s):
    """Encode, then datasets.yuv420_to_rgb8.  Y, U, V are each off by at most half a level after rounding, and the decoder multiplies them by
    cy and the channel's chroma coefficients; its own rounding adds half a level: |error| <= 0.5 cy + 0.5 sum |chroma coefficients| + 0.5,
    an integer error, so the floor of that."""
    y_off, cy, crv, cgu, cgv, cbu = ops.yuv_coefficients(m, r)
    bound = [math.floor(0.5 * cy + 0.5 * c + 0.5) for c in (abs(crv), abs(cgu) + abs(cgv), abs(cbu))]
    assert all(b in (1, 2) for b in bound)
    cols = np.concatenate([np.random.RandomState(7).randint(0, 256, (4000, 3)), np.array(OC.CORNERS)]).astype(np.uint8)
    frames = OC.constant_frames(cols, 2, 2)
    back = datasets.yuv420_to_rgb8(*datasets.rgb8_to_yuv420(frames, m, r, s), m, r, s)
    err = (back.to(torch.int64) - frames.to(torch.int64)).abs().reshape(-1, 3).max(0).values.tolist()
    print(f"[yuv-out] round trip {m}-{r}-{s}: max error {err}, bound {bound}")
    assert all(e <= b for e, b in zip(err, bound)), (err, bound)


def test_pack_and_planes_are_inverses():
    y, u, v = datasets.rgb8_to_yuv420(OC.texture(3, 6, 10, 3))
    for fmt in OC.FORMATS:
        packed = datasets.pack_yuv420(y, u, v, fmt)
        assert packed.shape == (3, 9, 10) and packed.dtype == torch.uint8 and packed.is_contiguous()
        for a, b in zip(ops.yuv420_planes(packed, fmt), (y, u, v)):
            assert torch.equal(a, b)
        assert torch.equal(datasets.pack_yuv420(*ops.yuv420_planes(packed, fmt), fmt), packed)
    assert not torch.equal(datasets.pack_yuv420(y, u, v, "i420"), datasets.pack_yuv420(y, u, v, "nv12"))
    assert datasets.pack_yuv420(y[:0], u[:0], v[:0], "nv12").shape == (0, 9, 10)


def test_y4m_round_trip(tmp_path):
    frames = OC.texture(3, 6, 10, 4)
    for siting, rng in (("left", "limited"), ("center", "full")):
        packed = datasets.pack_yuv420(*datasets.rgb8_to_yuv420(frames, "bt601", rng, siting), "i420")
        path = str(tmp_path / f"{siting}.y4m")
        datasets.write_y4m(path, packed, fps=(25, 1), siting=siting, range=rng)
        back, info = datasets.read_y4m(path)
        assert torch.equal(back, packed)
        assert info == dict(width=10, height=6, fps=(25, 1), siting=siting, range=rng)


def test_odd_sizes_and_bad_arguments_are_refused():
    y, u, v = datasets.rgb8_to_yuv420(OC.texture(2, 3, 5, 5))
    assert y.shape == (2, 3, 5) and u.shape == (2, 2, 3) and v.shape == (2, 2, 3)
    with pytest.raises(ValueError, match="odd"):
        datasets.pack_yuv420(y, u, v, "i420")
    with pytest.raises(ValueError, match="odd"):
        datasets.pack_yuv420(y[:, :2], u[:, :1], v[:, :1], "nv12")
    ye, ue, ve = datasets.rgb8_to_yuv420(OC.texture(2, 4, 6, 5))
    with pytest.raises(ValueError, match="chroma planes"):
        datasets.pack_yuv420(ye, ue[:, :1], ve, "i420")
    with pytest.raises(ValueError, match="fmt"):
        datasets.pack_yuv420(ye, ue, ve, "yv12")
    with pytest.raises(TypeError, match="uint8"):
        datasets.pack_yuv420(ye.float(), ue, ve)
    with pytest.raises(TypeError, match="uint8"):
        datasets.rgb8_to_yuv420(OC.texture(1, 4, 6, 5).float())
    with pytest.raises(ValueError, match="T, h0, w0, 3"):
        datasets.rgb8_to_yuv420(OC.texture(1, 4, 6, 5)[0])
    for bad in (dict(matrix="bt2020"), dict(range="tv"), dict(siting="top")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            datasets.rgb8_to_yuv420(OC.texture(1, 4, 6, 5), **bad)


def test_viz_host_backend():
    from fgvc_amd import viz
    frames = OC.texture(2, 6, 10, 6)
    want = datasets.pack_yuv420(*datasets.rgb8_to_yuv420(frames, "bt709", "full", "center"), "nv12")
    got = viz.frames_to_yuv420(frames.numpy(), "nv12", "bt709", "full", "center")
    assert isinstance(got, np.ndarray) and np.array_equal(got, want.numpy())
    assert torch.equal(viz.frames_to_yuv420(frames, "nv12", "bt709", "full", "center"), want)
    assert np.array_equal(viz.frames_to_yuv420(frames.numpy()), datasets.pack_yuv420(*datasets.rgb8_to_yuv420(frames), "i420").numpy())
    with pytest.raises(ValueError, match="odd"):
        viz.frames_to_yuv420(OC.texture(1, 3, 5, 6).numpy())
    with pytest.raises(ValueError, match="backend"):
        viz.frames_to_yuv420(frames.numpy(), backend="cuda")
    with pytest.raises(ValueError, match="fmt"):
        viz.frames_to_yuv420(frames.numpy(), "yv12")
    with pytest.raises(TypeError, match="uint8"):
        viz.frames_to_yuv420(frames.numpy().astype(np.float32))


@pytest.mark.parametrize("mutation", list(OC.MUTATIONS))
def test_each_mutation_is_caught_by_its_case(restated, mutation):
    """The float32 chain with one thing wrong: the named case's bytes must differ from the restatement's (which equal the unmutated chain:
    test_restatement_equals_the_float32_chain)."""
    cid = OC.MUTATIONS[mutation]
    name, m, r, s = CASES[cid]
    wrong = OC.encode(SETS[name].numpy(), m, r, s, np.float32, mutation)
    n = sum(int((a != b).sum()) for a, b in zip(restated(cid), wrong))
    print(f"[yuv-out] mutation {mutation}: {n} bytes differ on {cid}")
    assert n > 0, (mutation, cid)
