"""GPU: the YUV 4:2:0 input stage (fgvc_frames_yuv420_to_lab_f32, fgvc_frames_yuv420_to_rgb8, ops.yuv_frames_to_lab / _to_rgb8, test_cfg.input
type='nv12' | 'i420').

The Lab kernel against the float64 restatement of the contract (tests/yuv_cases.py), with the torch f32 chain on the same GPU as the yardstick:
E_kernel <= max(2 E_chain, 2^-22) per case, section 14's rule and floor, no pixel left out.  Everything else has no tolerance: the bytes kernel
equals the numpy float32 restatement, neutral chroma ties the new kernel to fgvc_frames_rgb8_to_lab_f32 bit for bit, and formats, views,
`out=`, streams and every call form of both trackers give identical bits."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import input_cases as IC
from tests import yuv_cases as YC

pytestmark = pytest.mark.gpu
CASES = YC.kernel_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def references():
    """(planes, size, matrix, range, siting) -> the float64 restatement (T, 3, h, w) on the CPU, computed once per setting (the formats
    share it) and never written to."""
    memo = {}

    def get(name):
        planes, size, _, matrix, rng, siting, _ = CASES[name]
        key = (name.rsplit("-", 1)[0])
        if key not in memo:
            memo[key] = YC.preprocess_f64(*YC.np_planes(planes), size, matrix, rng, siting)
        return memo[key]

    return get


def _planes(dev, planes, fmt):
    y, u, v = planes
    u, v = YC.in_format(u.to(dev), v.to(dev), fmt)
    return y.to(dev), u, v


def _interior(out, pad, h, w):
    left, right, top, bottom = pad
    return out[:, :, top:top + h, left:left + w]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ---- the Lab kernel against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_lab_kernel_within_twice_the_chains_error(dev, references, name):
    from fgvc_amd import ops
    from fgvc_amd.datasets import preprocess_yuv420_frames
    planes, size, pad, matrix, rng, siting, fmt = CASES[name]
    want = references(name)
    h, w = want.shape[-2:]
    y, u, v = _planes(dev, planes, fmt)
    chain = preprocess_yuv420_frames(y, u, v, (h, w), matrix, rng, siting)[0]
    got = ops.yuv_frames_to_lab(y, u, v, size, pad, matrix, rng, siting)
    assert got.dtype == torch.float32 and got.shape == (y.shape[0], 3, pad[2] + h + pad[3], pad[0] + w + pad[1])
    e_chain = float((chain.cpu().double() - want).abs().max())
    e_kernel = float((_interior(got, pad, h, w).cpu().double() - want).abs().max())
    bound = max(2 * e_chain, YC.ERROR_FLOOR)
    print(f"[yuv] {name}: E_chain = {e_chain:.3e}, E_kernel = {e_kernel:.3e}, bound = {bound:.3e}")
    assert e_kernel <= bound, (name, e_kernel, e_chain)
    border = got.clone()
    _interior(border, pad, h, w).zero_()
    assert int(border.view(torch.int32).abs().max()) == 0, name              # +0.0 bit for bit


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_bytes_kernel_equals_the_float32_restatement(dev, name):
    from fgvc_amd import ops
    planes, _, _, matrix, rng, siting, fmt = CASES[name]
    y, u, v = _planes(dev, planes, fmt)
    got = ops.yuv_frames_to_rgb8(y, u, v, matrix, rng, siting)
    want = YC.rgb8_f32(*YC.np_planes(planes), matrix, rng, siting)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), (name, int((got.cpu().numpy() != want).sum()))


def test_known_answers(dev):
    from fgvc_amd import ops
    triples = [((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255)), ((235, 128, 128), (255, 255, 255)),
               ((16, 128, 128), (0, 0, 0))]
    # one triple per frame, 2 x 2 luma over one chroma sample
    y = torch.tensor([t[0][0] for t in triples], dtype=torch.uint8).view(-1, 1, 1).expand(-1, 2, 2).contiguous().to(dev)
    u = torch.tensor([t[0][1] for t in triples], dtype=torch.uint8).view(-1, 1, 1).to(dev)
    v = torch.tensor([t[0][2] for t in triples], dtype=torch.uint8).view(-1, 1, 1).to(dev)
    for siting in YC.SITINGS:
        got = ops.yuv_frames_to_rgb8(y, u, v, "bt601", "limited", siting).cpu()
        for i, (_, rgb) in enumerate(triples):
            assert got[i].reshape(4, 3).tolist() == [list(rgb)] * 4, (siting, triples[i])
    lab = ops.yuv_frames_to_lab(y[3:], u[3:], v[3:]).cpu()                   # white and black: L = 100 and 0, no chroma
    assert torch.equal(lab[1], torch.tensor([-1.0, 0.0, 0.0]).view(3, 1, 1).expand(3, 2, 2))
    assert abs(float(lab[0, 0, 0, 0]) - 1.0) < 1e-5 and float(lab[0, 1:].abs().max()) < 1e-4


@pytest.mark.parametrize("size", [None, (24, 40)], ids=["same", "resized"])
@pytest.mark.parametrize("siting", YC.SITINGS)
def test_neutral_chroma_in_full_range_is_the_rgb_kernel_on_grey(dev, size, siting):
    """U = V = 128 in full range decodes to R = G = B = Y exactly: the bytes are Y, and the Lab planes are ops.frames_to_lab of the grey RGB
    frames bit for bit -- at the same size (there through the RGB kernel's table) and resized, 19 x 23 -> 24 x 40."""
    from fgvc_amd import ops
    y = IC.texture_u8(2, 19, 23, 8)[..., 0].contiguous().to(dev)
    c = torch.full((2, 10, 12), 128, dtype=torch.uint8, device=dev)
    grey = y[..., None].expand(2, 19, 23, 3).contiguous()
    for matrix in YC.MATRICES:
        assert torch.equal(ops.yuv_frames_to_rgb8(y, c, c.clone(), matrix, "full", siting), grey)
        got = ops.yuv_frames_to_lab(y, c, c.clone(), size, matrix=matrix, range="full", siting=siting)
        want = ops.frames_to_lab(grey, size)
        assert torch.equal(_bits(got), _bits(want)), (matrix, int((_bits(got) != _bits(want)).sum()))


@pytest.mark.parametrize("size,pad", [(None, (1, 2, 0, 1)), ((9, 13), (0, 3, 1, 0)), (None, (5, 3, 2, 2))])
def test_padded_interior_equals_unpadded_call(dev, size, pad):
    from fgvc_amd import ops
    y, u, v = _planes(dev, YC.texture_planes(2, 16, 20, 4), "nv12")
    for siting in YC.SITINGS:
        plain = ops.yuv_frames_to_lab(y, u, v, size, siting=siting)
        padded = ops.yuv_frames_to_lab(y, u, v, size, pad, siting=siting)
        h, w = plain.shape[-2:]
        assert torch.equal(_bits(_interior(padded, pad, h, w)), _bits(plain))
        _interior(padded, pad, h, w).zero_()
        assert int(padded.view(torch.int32).abs().max()) == 0                  # the border: +0.0 bit for bit


@pytest.mark.parametrize("size", [None, (24, 40)], ids=["same", "resized"])
def test_formats_views_and_streams_give_identical_bits(dev, size):
    """NV12 and I420 of the same samples; crops of larger planes at every byte alignment of the luma row (row stride above the width), a
    [::2] time slice, `out=` and a second stream; u and v swapped against their contents swapped: the same bits from both kernels."""
    from fgvc_amd import ops
    Y, U, V = (p.to(dev) for p in YC.texture_planes(4, 48, 64, 6))          # 24 x 32 chroma
    for siting in YC.SITINGS:
        kw = dict(siting=siting, matrix="bt709")
        for x0 in (4, 6, 8, 10):                                             # luma columns 4 .. 10: dword aligned or not; chroma columns 2 .. 5
            y = Y[:, 6:6 + 37, x0:x0 + 53]
            u, v = U[:, 3:3 + 19, x0 // 2:x0 // 2 + 27], V[:, 3:3 + 19, x0 // 2:x0 // 2 + 27]
            assert not y.is_contiguous() and not u.is_contiguous()
            want = ops.yuv_frames_to_lab(y.contiguous(), u.contiguous(), v.contiguous(), size, **kw)
            want8 = ops.yuv_frames_to_rgb8(y.contiguous(), u.contiguous(), v.contiguous(), **kw)
            assert torch.equal(_bits(ops.yuv_frames_to_lab(y, u, v, size, **kw)), _bits(want)), (siting, x0)
            assert torch.equal(ops.yuv_frames_to_rgb8(y, u, v, **kw), want8), (siting, x0)
            for fmt in YC.FORMATS:
                fu, fv = YC.in_format(u, v, fmt)
                assert torch.equal(_bits(ops.yuv_frames_to_lab(y, fu, fv, size, **kw)), _bits(want)), (siting, x0, fmt)
                assert torch.equal(ops.yuv_frames_to_rgb8(y, fu, fv, **kw), want8), (siting, x0, fmt)
        for x0 in (5, 7):                                                    # an odd first column: bytes, and an odd frame (37 x 53)
            y = Y[:, 6:6 + 37, x0:x0 + 53]
            assert torch.equal(_bits(ops.yuv_frames_to_lab(y, u, v, size, **kw)),
                               _bits(ops.yuv_frames_to_lab(y.contiguous(), u.contiguous(), v.contiguous(), size, **kw))), (siting, x0)
            assert torch.equal(ops.yuv_frames_to_rgb8(y, u, v, **kw), ops.yuv_frames_to_rgb8(y.contiguous(), u.contiguous(), v.contiguous(), **kw))
        y = Y[:, 6:6 + 37, 10:10 + 53]
        assert torch.equal(_bits(ops.yuv_frames_to_lab(y[::2], u[::2], v[::2], size, **kw)), _bits(want[::2]))        # a time slice
        assert torch.equal(ops.yuv_frames_to_rgb8(y[::2], u[::2], v[::2], **kw), want8[::2])
        out, out8 = torch.full_like(want, float("nan")), torch.full_like(want8, 0xA5)
        assert ops.yuv_frames_to_lab(y, u, v, size, out=out, **kw) is out and torch.equal(_bits(out), _bits(want))
        assert ops.yuv_frames_to_rgb8(y, u, v, out=out8, **kw) is out8 and torch.equal(out8, want8)
        s = torch.cuda.Stream(device=dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            again, again8 = ops.yuv_frames_to_lab(y, u, v, size, **kw), ops.yuv_frames_to_rgb8(y, u, v, **kw)
        s.synchronize()
        assert torch.equal(_bits(again), _bits(want)) and torch.equal(again8, want8)
        # NV21 / YV12: the planes swapped in the call == the planes' contents swapped
        assert torch.equal(_bits(ops.yuv_frames_to_lab(y, v, u, size, **kw)),
                           _bits(ops.yuv_frames_to_lab(y, v.contiguous(), u.contiguous(), size, **kw)))
        swapped = ops.yuv_frames_to_rgb8(y, v, u, **kw)
        assert torch.equal(swapped, ops.yuv_frames_to_rgb8(y, v.contiguous(), u.contiguous(), **kw)) and not torch.equal(swapped, want8)


@pytest.mark.parametrize("size,pad", [(None, (0, 0, 0, 0)), (None, (1, 2, 0, 1)), ((24, 40), (0, 3, 1, 0))])
def test_outputs_stay_between_their_guard_bands(dev, size, pad):
    """Both kernels write into the middle of a larger buffer whose two ends (NaN for the planes, 0xA5 for the bytes) stay intact: odd
    19 x 23 frames, whose rows end inside a lane's 4 columns and inside a dword of the packed bytes."""
    from fgvc_amd import ops
    y, u, v = _planes(dev, YC.texture_planes(2, 19, 23, 9), "nv12")
    h, w = size or (19, 23)
    n = 2 * 3 * (pad[2] + h + pad[3]) * (pad[0] + w + pad[1])
    buf = torch.full((n + 512,), float("nan"), device=dev)
    out = buf[256:256 + n].view(2, 3, pad[2] + h + pad[3], pad[0] + w + pad[1])
    ops.yuv_frames_to_lab(y, u, v, size, pad, out=out)
    assert bool(torch.isnan(buf[:256]).all()) and bool(torch.isnan(buf[256 + n:]).all()) and bool(torch.isfinite(out).all())
    assert torch.equal(_bits(out), _bits(ops.yuv_frames_to_lab(y, u, v, size, pad)))
    n8 = 2 * 19 * 23 * 3
    for lead in (256, 257, 258, 259):                                        # every byte alignment of the packed output
        buf8 = torch.full((n8 + 515,), 0xA5, dtype=torch.uint8, device=dev)
        out8 = buf8[lead:lead + n8].view(2, 19, 23, 3)
        ops.yuv_frames_to_rgb8(y, u, v, out=out8)
        assert bool((buf8[:lead] == 0xA5).all()) and bool((buf8[lead + n8:] == 0xA5).all()), lead
        assert torch.equal(out8, ops.yuv_frames_to_rgb8(y, u, v)), lead


def test_wrapper_refusals(dev):
    from fgvc_amd import _lib, ops
    y, u, v = _planes(dev, YC.texture_planes(2, 6, 8, 1), "i420")
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.yuv_frames_to_lab(y.cpu(), u, v)
    with pytest.raises(TypeError, match="uint8"):
        ops.yuv_frames_to_lab(y.float(), u, v)
    with pytest.raises(TypeError, match="uint8"):
        ops.yuv_frames_to_rgb8(y, u, v.float())
    with pytest.raises(ValueError, match="3 dimensions"):
        ops.yuv_frames_to_lab(y[0], u, v)
    with pytest.raises(ValueError, match="chroma planes"):
        ops.yuv_frames_to_lab(y, u[:, :2], v)
    with pytest.raises(ValueError, match="chroma planes"):
        ops.yuv_frames_to_rgb8(y, u, v[:1])
    with pytest.raises(ValueError, match="same strides"):
        ops.yuv_frames_to_lab(y, u, YC.in_format(u, v, "nv12")[1])
    with pytest.raises(ValueError, match="adjacent"):
        ops.yuv_frames_to_lab(torch.zeros(2, 6, 16, dtype=torch.uint8, device=dev)[:, :, ::2], u, v)
    for bad in (dict(matrix="bt2020"), dict(range="tv"), dict(siting="top")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ops.yuv_frames_to_lab(y, u, v, **bad)
    with pytest.raises(ValueError, match="out"):
        ops.yuv_frames_to_lab(y, u, v, out=torch.empty(2, 3, 6, 9, device=dev))
    with pytest.raises(ValueError, match="out"):
        ops.yuv_frames_to_rgb8(y, u, v, out=torch.empty(2, 6, 8, 3, device=dev))
    with pytest.raises(ValueError, match="out"):
        ops.yuv_frames_to_rgb8(y, u, v, out=torch.empty(2, 8, 6, 3, dtype=torch.uint8, device=dev).transpose(1, 2))
    with pytest.raises(_lib.FgvcHipError, match="negative pad"):
        ops.yuv_frames_to_lab(y, u, v, out=torch.empty(2, 3, 6, 7, device=dev), pad=(-1, 0, 0, 0))
    assert ops.yuv_frames_to_lab(y[:0], u[:0], v[:0]).shape == (0, 3, 6, 8)
    assert ops.yuv_frames_to_rgb8(y[:0], u[:0], v[:0]).shape == (0, 6, 8, 3)


# ---- the trackers: packed frames with the key == the same model on ops.yuv_frames_to_lab of those frames, bit for bit -------------------------
# Every label-map and flow form runs on encoders of output stride 4 (the pad unit), so that 42 x 46 is padded to 44 x 48 -- by the kernel in
# the packed call, by F.pad of the unpadded conversion in the float call; the points forms never pad.
CFG_VA = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=12, step=512, with_first_neighbor=True, batch_step=2)
CFG_HR = dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True, batch_step=2)
VA = dict(typ="VanillaTracker", strides=(1, 1, 1, 4), kw=dict(), cfg=CFG_VA)
VA4 = dict(typ="VanillaTracker", strides=(1, 2, 1, 4), kw=dict(), cfg=CFG_VA)
HR = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1), kw=dict(), cfg=CFG_HR)
HR4 = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1), kw=dict(stride=4), cfg=CFG_HR)
YUV = dict(matrix="bt709", range="limited", siting="center")
T, H0, W0 = 5, 42, 46


def _tracker(dev, spec, **extra):
    from oracle import fgvc_oracle as O
    import fgvc_amd.mmpt_api as api
    model = api.build_model(dict(type=spec["typ"], **spec["kw"], backbone=dict(type="ResNet", depth=18, strides=spec["strides"],
                                                                                out_indices=(2,), pool_type="none")),
                            train_cfg=None, test_cfg=api.ConfigDict(**{**spec["cfg"], **extra}))
    model.backbone.load_state_dict(O.seeded_resnet_state(3, spec["strides"], "none"), strict=False)
    return model.to(dev).eval()


def _points(T, h, w, P, spread, seed=0):
    g = torch.Generator().manual_seed(seed)
    t0 = torch.randint(0, max(1, T // 2), (P,), generator=g).float() if spread else torch.zeros(P)
    qp = torch.stack([t0, torch.rand(P, generator=g) * (w - 16) + 8, torch.rand(P, generator=g) * (h - 16) + 8], -1)[None]
    return dict(query_points=qp, trajectories=torch.zeros(1, T, P, 2), visibilities=torch.ones(1, T, P))


def _same(a, b):
    assert type(a) is type(b)
    if isinstance(a, dict):
        assert sorted(a) == sorted(b)
        for k in a:
            _same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b)
    else:
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


def _lab(dev, planes, size=None):
    from fgvc_amd import ops
    return ops.yuv_frames_to_lab(*(p.to(dev) for p in planes), size, **YUV)


POINT_CASES = [
    ("vanilla", VA, dict(), (H0, W0), None, False),
    ("vanilla_regrouped", VA, dict(with_first=True), (H0, W0), None, True),
    ("vanilla_occlusion", VA, dict(with_first=True, occlusion=dict(type="cycle")), (H0, W0), None, True),
    ("vanilla_chain", VA, dict(chain=dict(type="flow")), (H0, W0), None, True),
    ("vanilla_resized", VA, dict(with_first=True), (96, 128), (64, 64), True),
    ("hr", HR, dict(with_first=False), (H0, W0), None, False),
    ("hr_regrouped_occlusion", HR, dict(occlusion=dict(type="cycle")), (H0, W0), None, True),
    ("hr_chain", HR4, dict(chain=dict(type="flow", visibility="consistency")), (H0, W0), None, True),
]


@pytest.mark.parametrize("name,spec,extra,src,size,spread", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_points_call_takes_packed_frames(dev, name, spec, extra, src, size, spread):
    planes = YC.texture_planes(T, src[0], src[1], 11)
    h, w = size or src
    data = {k: v.to(dev) for k, v in _points(T, h, w, 6, spread).items()}
    want = None
    for fmt in YC.FORMATS:
        model = _tracker(dev, spec, input=dict(type=fmt, size=size, **YUV), **extra)
        got = model(test_mode=True, rgbs=YC.pack(*planes, fmt).to(dev)[None], **data)
        if want is None:
            want = model(test_mode=True, rgbs=_lab(dev, planes, size)[None], **data)       # float frames with the key set: as ever
        _same(got, want)
        assert got[2].shape == (1, T, 6, 2) and bool(torch.isfinite(got[2]).all())
    plain = _tracker(dev, spec, **extra)
    with pytest.raises(TypeError, match="test_cfg.input"):
        plain(test_mode=True, rgbs=YC.pack(*planes, "nv12").to(dev)[None], **data)


LABEL_CASES = [("masks", dict()), ("coords", dict(coords=True)), ("maps", dict(return_maps=True))]


@pytest.mark.parametrize("spec", [VA4, HR4], ids=["vanilla", "hr"])
@pytest.mark.parametrize("form,extra", LABEL_CASES, ids=[c[0] for c in LABEL_CASES])
def test_label_calls_take_packed_frames(dev, spec, form, extra):
    planes = YC.texture_planes(T, H0, W0, 13)
    h, w = H0, W0
    if form == "masks":
        seg = torch.zeros(1, h, w, dtype=torch.uint8)
        seg[0, 8:24, 10:30], seg[0, 20:36, 25:44] = 1, 2
    else:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        seg = torch.stack([torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 18.0) for cx, cy in ((12.0, 10.0), (30.5, 25.0), (40.0, 33.0))])[None]
    seg, meta = seg.to(dev), [dict(original_shape=(h, w))]
    lab = _lab(dev, planes)                                                  # (T, 3, h, w), unpadded
    want = None
    for fmt in YC.FORMATS:
        model = _tracker(dev, spec, input=dict(type=fmt, **YUV), **extra)
        frames, _, pad = model._label_frames(YC.pack(*planes, fmt).to(dev)[None, None])
        assert tuple(frames.shape) == (T, 3, 44, 48) and pad == (1, 1, 1, 1)               # padded, by the kernel
        got = model(test_mode=True, imgs=YC.pack(*planes, fmt).to(dev)[None, None], ref_seg_map=seg, img_meta=meta)
        if want is None:
            want = model(test_mode=True, imgs=lab.transpose(0, 1)[None, None].contiguous(), ref_seg_map=seg, img_meta=meta)
        _same(got, want)
        assert got[0].shape == {"masks": (T, h, w), "coords": (2, 3, T), "maps": (T, 3, h, w)}[form]
    plain = _tracker(dev, spec, **extra)
    with pytest.raises(TypeError, match="test_cfg.input"):
        plain(test_mode=True, imgs=YC.pack(*planes, "i420").to(dev)[None, None], ref_seg_map=seg, img_meta=meta)


@pytest.mark.parametrize("spec", [VA4, HR4], ids=["vanilla", "hr"])
def test_flow_call_takes_packed_frames(dev, spec):
    planes = YC.texture_planes(T, H0, W0, 14)
    lab = _lab(dev, planes)
    want = None
    for fmt in YC.FORMATS:
        model = _tracker(dev, spec, input=dict(type=fmt, **YUV), flow=dict(type="window", occlusion="fb_abs"))
        got = model(test_mode=True, imgs=YC.pack(*planes, fmt).to(dev)[None, None])
        if want is None:
            want = model(test_mode=True, imgs=lab.transpose(0, 1)[None, None].contiguous())
        _same(got, want)
        assert got["flow_fw"].shape == (T - 1, 2, H0, W0)


def test_forward_warping_takes_packed_frames(dev):
    planes = YC.texture_planes(T, H0, W0, 12)
    ref = torch.tensor([[[20.0, 31.5, 12.0], [18.0, 40.25, 30.0]]], device=dev)       # (1, 2, P) rows (y, x)
    lab = _lab(dev, planes)
    want = None
    for fmt in YC.FORMATS:
        model = _tracker(dev, HR, input=dict(type=fmt, **YUV))
        got = model.forward_test_forward(YC.pack(*planes, fmt).to(dev)[None, None], ref=ref)
        if want is None:
            want = model.forward_test_forward(lab.transpose(0, 1)[None, None], ref=ref)
        _same(got, want)
        assert got[0].shape == (2, 3, T)


# ---- the demo on a .y4m clip ----------------------------------------------------------------------------------------------------------------------
def test_demo_runs_on_a_y4m_clip(dev, tmp_path):
    from PIL import Image
    from fgvc_amd import ops, viz
    from fgvc_amd.datasets import write_y4m
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(ROOT, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    packed = YC.packed_texture(4, 48, 64, 15, "i420")
    clip = str(tmp_path / "clip.y4m")
    write_y4m(clip, packed, siting="center", range="full")
    r = demo.main([clip, "--task", "points", "--query-points", "0", "20", "16", "1", "40", "30", "--out", str(tmp_path / "o"), "--radius", "2",
                   "--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--precede-frames", "3", "--batch-step", "2"])
    names = sorted(n for n in os.listdir(tmp_path / "o") if n.endswith(".png"))
    assert names == [f"frame_{t:05d}.png" for t in range(4)]
    rgb = ops.yuv_frames_to_rgb8(*ops.yuv420_planes(packed.to(dev), "i420"), matrix="bt601", range="full", siting="center")      # 48 rows: bt601
    assert np.array_equal(r["frames"], rgb.cpu().numpy())
    assert r["tracks"].shape == (2, 4, 2) and np.isfinite(r["tracks"]).all()
    want = viz.render(rgb.cpu().numpy(), tracks=r["tracks"], visibles=r["visibles"], radius=2)
    assert (want != r["frames"]).any()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o" / "frame_00000.png").convert("RGB")), want[0])
    assert np.array_equal(r["rendered"], want)
