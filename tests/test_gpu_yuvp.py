"""GPU: the input stage for Y'CbCr at 8 to 16 bits, 4:2:0 / 4:2:2 / 4:4:4 (fgvc_frames_yuvp_to_lab_f32, fgvc_frames_yuvp_to_rgb8,
ops.yuv_planes_to_lab / _to_rgb8, test_cfg.input type = an ops.YUV_PIXEL_FORMATS name).

The Lab kernel against the float64 restatement of the contract (tests/yuvp_cases.py), with the torch f32 chain on the same GPU as the
yardstick: E_kernel <= max(2 E_chain, 2^-22) per case, the project's rule for input kernels, no pixel left out, the border +0.0.  Everything
else has no tolerance: the bytes kernel equals the numpy float32 restatement; depth 8 / (2, 2) is the 8-bit entries, 4 x the samples at 10
bits under limited range is the 8-bit kernel, P010 is yuv420p10, garbage in the unused bits changes nothing, neutral 4:4:4 chroma is the RGB
kernel on grey; views, `out=`, streams and every call form of both trackers give identical bits."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import input_cases as IC
from tests import yuv_cases as YC
from tests import yuvp_cases as PC

pytestmark = pytest.mark.gpu
CASES = PC.kernel_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _interior(out, pad, h, w):
    left, right, top, bottom = pad
    return out[:, :, top:top + h, left:left + w]


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _eq(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _kw(fmt, **more):
    return dict(PC.fmt_args(fmt), **more)


# ---- the Lab kernel against float64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_lab_kernel_within_twice_the_chains_error(dev, name):
    from fgvc_amd import ops
    from fgvc_amd.datasets import preprocess_yuv_frames
    fmt, _, _, size, pad, matrix, rng, siting = CASES[name]
    planes = PC.case_planes(CASES[name])
    want = PC.preprocess_f64(*planes, fmt, size, matrix, rng, siting)
    h, w = want.shape[-2:]
    y, u, v = PC.to_torch(planes, fmt, dev)
    chain = preprocess_yuv_frames(y, u, v, **_kw(fmt, matrix=matrix, range=rng, siting=siting, size=size))[0]
    got = ops.yuv_planes_to_lab(y, u, v, **_kw(fmt, size=size, pad=pad, matrix=matrix, range=rng, siting=siting))
    assert got.dtype == torch.float32 and got.shape == (y.shape[0], 3, pad[2] + h + pad[3], pad[0] + w + pad[1])
    e_chain = float((chain.cpu().double() - want).abs().max())
    e_kernel = float((_interior(got, pad, h, w).cpu().double() - want).abs().max())
    bound = max(2 * e_chain, YC.ERROR_FLOOR)
    print(f"[yuvp] {name}: E_chain = {e_chain:.3e}, E_kernel = {e_kernel:.3e}, bound = {bound:.3e}")
    assert e_kernel <= bound, (name, e_kernel, e_chain)
    border = got.clone()
    _interior(border, pad, h, w).zero_()
    assert int(border.view(torch.int32).abs().max()) == 0, name              # +0.0 bit for bit


# ---- exact ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_bytes_kernel_equals_the_float32_restatement(dev, name):
    from fgvc_amd import ops
    fmt, _, _, _, _, matrix, rng, siting = CASES[name]
    planes = PC.case_planes(CASES[name])
    got = ops.yuv_planes_to_rgb8(*PC.to_torch(planes, fmt, dev), **_kw(fmt, matrix=matrix, range=rng, siting=siting))
    want = PC.rgb8_f32(*planes, fmt, matrix, rng, siting)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), (name, int((got.cpu().numpy() != want).sum()))


@pytest.mark.parametrize("size", [None, (24, 40)], ids=["same", "resized"])
@pytest.mark.parametrize("fmt", YC.FORMATS)
def test_depth_8_420_is_the_8_bit_entries(dev, fmt, size):
    """Tie 1: depth 8, shift 0, subsampling (2, 2) on tests/yuv_cases textures, through NV12's and I420's strides."""
    from fgvc_amd import ops
    for planes in (YC.texture_planes(3, 37, 53, 2), YC.lattice_planes(), YC.tie_planes()):
        y = planes[0].to(dev)
        u, v = YC.in_format(planes[1].to(dev), planes[2].to(dev), fmt)
        for matrix, rng, siting in PC.SETTINGS:
            kw = dict(matrix=matrix, range=rng, siting=siting)
            assert _eq(ops.yuv_planes_to_lab(y, u, v, 8, 0, (2, 2), size, **kw), ops.yuv_frames_to_lab(y, u, v, size, **kw)), (matrix, rng, siting)
            assert _eq(ops.yuv_planes_to_rgb8(y, u, v, 8, 0, (2, 2), **kw), ops.yuv_frames_to_rgb8(y, u, v, **kw)), (matrix, rng, siting)


@pytest.mark.parametrize("size", [None, (24, 40)], ids=["same", "resized"])
def test_four_times_the_samples_at_10_bits_is_the_8_bit_kernel(dev, size):
    """Tie 2: under limited range the 10-bit constants are the 8-bit ones times exact powers of two, so a frame whose every sample is 4 x an
    8-bit frame's decodes to the same bits -- low-aligned and as P010 (x 4 x 64)."""
    from fgvc_amd import ops
    y8, u8, v8 = (p.to(dev) for p in YC.texture_planes(2, 19, 23, 5))
    for matrix in PC.MATRICES:
        for siting in PC.SITINGS:
            kw = dict(matrix=matrix, range="limited", siting=siting)
            want, want8 = ops.yuv_frames_to_lab(y8, u8, v8, size, **kw), ops.yuv_frames_to_rgb8(y8, u8, v8, **kw)
            for shift in (0, 6):
                y, u, v = ((p.cpu().to(torch.int32) * (4 << shift)).to(torch.uint16).to(dev) for p in (y8, u8, v8))     # (made on the host)
                assert _eq(ops.yuv_planes_to_lab(y, u, v, 10, shift, (2, 2), size, **kw), want), (matrix, siting, shift)
                assert _eq(ops.yuv_planes_to_rgb8(y, u, v, 10, shift, (2, 2), **kw), want8), (matrix, siting, shift)


@pytest.mark.parametrize("size", [None, (9, 13)], ids=["same", "resized"])
def test_unused_bits_never_reach_the_arithmetic(dev, size):
    """Tie 3: P010 == yuv420p10 on the same samples; P010 with garbage in the low six bits == with zeros; yuv420p10 with garbage above bit 9
    == the clean one."""
    from fgvc_amd import ops
    s = PC.texture_samples(2, 17, 22, 4, "p010")
    rs = np.random.RandomState(9)
    out = {}
    for fmt in ("p010", "yuv420p10"):
        for label, planes in (("clean", tuple(PC.clean_words(p, fmt) for p in s)), ("garbage", tuple(PC.words(p, fmt, rs) for p in s))):
            assert label == "clean" or any((a != b).any() for a, b in zip(planes, (PC.clean_words(p, fmt) for p in s)))
            t = PC.to_torch(planes, fmt, dev)
            out[fmt, label] = (ops.yuv_planes_to_lab(*t, **_kw(fmt, size=size, range="full", siting="center")),
                               ops.yuv_planes_to_rgb8(*t, **_kw(fmt, range="full", siting="center")))
    first = out["p010", "clean"]
    for key, (lab, rgb) in out.items():
        assert _eq(lab, first[0]) and _eq(rgb, first[1]), key


@pytest.mark.parametrize("size", [None, (24, 40)], ids=["same", "resized"])
def test_neutral_444_chroma_in_full_range_is_the_rgb_kernel_on_grey(dev, size):
    """Tie 4: 8-bit 4:4:4, U = V = 128 in full range decodes to R = G = B = Y exactly."""
    from fgvc_amd import ops
    y = IC.texture_u8(2, 19, 23, 8)[..., 0].contiguous().to(dev)
    c = torch.full((2, 19, 23), 128, dtype=torch.uint8, device=dev)
    grey = y[..., None].expand(2, 19, 23, 3).contiguous()
    for matrix in PC.MATRICES:
        kw = dict(matrix=matrix, range="full")
        assert torch.equal(ops.yuv_planes_to_rgb8(y, c, c.clone(), 8, 0, (1, 1), **kw), grey)
        assert _eq(ops.yuv_planes_to_lab(y, c, c.clone(), 8, 0, (1, 1), size, **kw), ops.frames_to_lab(grey, size)), matrix


@pytest.mark.parametrize("fmt", ["yuv444p", "yuv444p10"])
def test_444_does_not_depend_on_the_siting(dev, fmt):
    """Tie 5."""
    from fgvc_amd import ops
    t = PC.to_torch(PC.texture_planes(2, 17, 22, 6, fmt), fmt, dev)
    for size in (None, (9, 13)):
        assert _eq(ops.yuv_planes_to_lab(*t, **_kw(fmt, size=size, siting="left")), ops.yuv_planes_to_lab(*t, **_kw(fmt, size=size, siting="center")))
    assert _eq(ops.yuv_planes_to_rgb8(*t, **_kw(fmt, siting="left")), ops.yuv_planes_to_rgb8(*t, **_kw(fmt, siting="center")))


def test_known_answers(dev):
    from fgvc_amd import ops

    def planes(triples, sub):
        return tuple(torch.tensor([t[i] for t in triples], dtype=torch.int32).to(torch.uint16).view(-1, 1, 1)
                     .expand(-1, 2 if i == 0 else 2 // sub[1], 2 if i == 0 else 2 // sub[0]).contiguous().to(dev) for i in range(3))
    for sub in ((2, 2), (2, 1), (1, 1)):
        y, u, v = planes([(940, 512, 512), (64, 512, 512)], sub)             # 10-bit limited: white and black
        for matrix in PC.MATRICES:
            for siting in PC.SITINGS:
                kw = dict(matrix=matrix, range="limited", siting=siting)
                got = ops.yuv_planes_to_rgb8(y, u, v, 10, 0, sub, **kw).cpu()
                assert got[0].reshape(-1).tolist() == [255] * 12 and got[1].reshape(-1).tolist() == [0] * 12, (sub, matrix, siting)
                lab = ops.yuv_planes_to_lab(y, u, v, 10, 0, sub, **kw).cpu()
                assert torch.equal(lab[1], torch.tensor([-1.0, 0.0, 0.0]).view(3, 1, 1).expand(3, 2, 2))                 # exactly (-1, 0, 0)
                assert abs(float(lab[0, 0, 0, 0]) - 1.0) < 1e-5 and float(lab[0, 1:].abs().max()) < 1e-4                # L = 100, no chroma
                p = tuple((t.cpu().to(torch.int32) << 6).to(torch.uint16).to(dev) for t in (y, u, v))                                  # the same as P010 words
                assert torch.equal(ops.yuv_planes_to_rgb8(*p, 10, 6, sub, **kw).cpu(), got)
        y, u, v = planes([(65535, 32768, 32768), (0, 32768, 32768)], sub)    # 16-bit full range
        got = ops.yuv_planes_to_rgb8(y, u, v, 16, 0, sub, range="full").cpu()
        assert got[0].reshape(-1).tolist() == [255] * 12 and got[1].reshape(-1).tolist() == [0] * 12
        lab = ops.yuv_planes_to_lab(y, u, v, 16, 0, sub, range="full").cpu()
        assert abs(float(lab[0, 0, 0, 0]) - 1.0) < 1e-5 and float(lab[0, 1:].abs().max()) < 1e-4
        assert torch.equal(lab[1], torch.tensor([-1.0, 0.0, 0.0]).view(3, 1, 1).expand(3, 2, 2))


# ---- views ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [None, (24, 40)], ids=["same", "resized"])
@pytest.mark.parametrize("fmt", ["p010", "yuv422p10", "nv16", "yuv444p"])
def test_views_layouts_and_streams_give_identical_bits(dev, fmt, size):
    """Crops of larger planes at every alignment of the luma row (even and odd column offsets: the vector load of 4 samples, 4 or 8 bytes,
    and the sample-by-sample path, for both sample types), a [::2] time slice, pixel stride 2 against planar copies, `out=` and a second
    stream: the same bits from both kernels."""
    from fgvc_amd import ops
    _, sx, sy = PC.FORMATS[fmt][:3]
    host = PC.texture_planes(4, 48, 64, 6, fmt)
    Y, U, V = (torch.from_numpy(p).to(dev) for p in host)
    kw = _kw(fmt, matrix="bt709", siting="center")
    want = want8 = None
    for x0 in (4, 6, 8, 10, 5, 7):
        h, w = 37, 53
        cx0, cy0 = (x0 // sx, 6 // sy)                                       # (an odd x0 shifts luma against chroma: another picture, the same check)
        crop = (slice(None), slice(6, 6 + h), slice(x0, x0 + w))
        ccrop = (slice(None), slice(cy0, cy0 + (h + sy - 1) // sy), slice(cx0, cx0 + (w + sx - 1) // sx))
        y, u, v = Y[crop], U[ccrop], V[ccrop]                                # views of the larger planes
        assert not y.is_contiguous() and not u.is_contiguous()
        cont = tuple(torch.from_numpy(np.ascontiguousarray(p[c])).to(dev) for p, c in zip(host, (crop, ccrop, ccrop)))   # copies, made on the host
        want, want8 = ops.yuv_planes_to_lab(*cont, size=size, **kw), ops.yuv_planes_to_rgb8(*cont, **kw)
        assert _eq(ops.yuv_planes_to_lab(y, u, v, size=size, **kw), want), x0
        assert _eq(ops.yuv_planes_to_rgb8(y, u, v, **kw), want8), x0
        su, sv = PC.in_layout(host[1][ccrop], host[2][ccrop], "nv16", dev)  # the same samples as interleaved pairs: pixel stride 2
        assert su.stride(2) == 2
        assert _eq(ops.yuv_planes_to_lab(y, su, sv, size=size, **kw), want) and _eq(ops.yuv_planes_to_rgb8(y, su, sv, **kw), want8), x0
    assert _eq(ops.yuv_planes_to_lab(y[::2], u[::2], v[::2], size=size, **kw), want[::2])                     # a time slice
    assert _eq(ops.yuv_planes_to_rgb8(y[::2], u[::2], v[::2], **kw), want8[::2])
    out, out8 = torch.full_like(want, float("nan")), torch.full_like(want8, 0xA5)
    assert ops.yuv_planes_to_lab(y, u, v, size=size, out=out, **kw) is out and _eq(out, want)
    assert ops.yuv_planes_to_rgb8(y, u, v, out=out8, **kw) is out8 and _eq(out8, want8)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        again, again8 = ops.yuv_planes_to_lab(y, u, v, size=size, **kw), ops.yuv_planes_to_rgb8(y, u, v, **kw)
    s.synchronize()
    assert _eq(again, want) and _eq(again8, want8)
    swapped = ops.yuv_planes_to_rgb8(y, v, u, **kw)                          # NV21-style: the planes swapped in the call
    assert _eq(swapped, ops.yuv_planes_to_rgb8(cont[0], cont[2], cont[1], **kw)) and not torch.equal(swapped, want8)


@pytest.mark.parametrize("fmt", ["p010", "yuv444p"])
def test_outputs_stay_between_their_guard_bands(dev, fmt):
    """Both kernels write into the middle of a larger buffer whose two ends stay intact: odd 19 x 23 frames."""
    from fgvc_amd import ops
    t = PC.to_torch(PC.texture_planes(2, 19, 23, 9, fmt), fmt, dev)
    for size, pad in ((None, (0, 0, 0, 0)), (None, (1, 2, 3, 1)), ((24, 40), (2, 3, 1, 1))):
        h, w = size or (19, 23)
        shape = (2, 3, pad[2] + h + pad[3], pad[0] + w + pad[1])
        n = int(np.prod(shape))
        buf = torch.full((n + 512,), float("nan"), device=dev)
        out = buf[256:256 + n].view(shape)
        ops.yuv_planes_to_lab(*t, **_kw(fmt, size=size, pad=pad, out=out))
        assert bool(torch.isnan(buf[:256]).all()) and bool(torch.isnan(buf[256 + n:]).all()) and bool(torch.isfinite(out).all())
    n8 = 2 * 19 * 23 * 3
    for lead in (256, 257, 258, 259):                                        # every byte alignment of the packed output
        buf8 = torch.full((n8 + 515,), 0xA5, dtype=torch.uint8, device=dev)
        out8 = buf8[lead:lead + n8].view(2, 19, 23, 3)
        ops.yuv_planes_to_rgb8(*t, **_kw(fmt, out=out8))
        assert bool((buf8[:lead] == 0xA5).all()) and bool((buf8[lead + n8:] == 0xA5).all()), lead
        assert torch.equal(out8, ops.yuv_planes_to_rgb8(*t, **_kw(fmt))), lead


def test_wrapper_refusals(dev):
    from fgvc_amd import _lib, ops
    y, u, v = PC.to_torch(PC.texture_planes(2, 6, 8, 1, "yuv420p10"), "yuv420p10", dev)
    kw = dict(depth=10)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.yuv_planes_to_lab(y.cpu(), u, v, **kw)
    with pytest.raises(TypeError, match="uint16"):
        ops.yuv_planes_to_lab(y.float(), u, v, **kw)
    with pytest.raises(TypeError, match="one dtype"):
        ops.yuv_planes_to_rgb8(y, u, torch.zeros(2, 3, 4, dtype=torch.uint8, device=dev), **kw)
    with pytest.raises(ValueError, match="3 dimensions"):
        ops.yuv_planes_to_lab(y[0], u, v, **kw)
    with pytest.raises(ValueError, match="chroma planes"):
        ops.yuv_planes_to_lab(y, u, v, 10, 0, (2, 1))
    with pytest.raises(ValueError, match="chroma planes"):
        ops.yuv_planes_to_rgb8(y, u, v[:1], **kw)
    for sub in ((4, 1), (0, 2), (2,), "420"):
        with pytest.raises(ValueError, match="subsampling"):
            ops.yuv_planes_to_lab(y, u, v, 10, 0, sub)
    for depth, shift in ((7, 0), (17, 0), (10, 7), (16, 1), (10, -1)):
        with pytest.raises(ValueError, match="depth"):
            ops.yuv_planes_to_lab(y, u, v, depth, shift)
    with pytest.raises(ValueError, match="depth"):
        ops.yuv_planes_to_rgb8(*(torch.zeros(p.shape, dtype=torch.uint8, device=dev) for p in (y, u, v)), depth=10)
    with pytest.raises(ValueError, match="same strides"):
        ops.yuv_planes_to_lab(y, u, PC.in_layout(np.zeros((2, 3, 4), np.uint16), np.zeros((2, 3, 4), np.uint16), "p010", dev)[1], **kw)
    with pytest.raises(ValueError, match="adjacent"):
        ops.yuv_planes_to_lab(torch.zeros(2, 6, 16, dtype=torch.uint16).to(dev)[:, :, ::2], u, v, **kw)
    for bad in (dict(matrix="bt2020"), dict(range="tv"), dict(siting="top")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ops.yuv_planes_to_lab(y, u, v, **kw, **bad)
    with pytest.raises(ValueError, match="out"):
        ops.yuv_planes_to_lab(y, u, v, out=torch.empty(2, 3, 6, 9, device=dev), **kw)
    with pytest.raises(ValueError, match="out"):
        ops.yuv_planes_to_rgb8(y, u, v, out=torch.empty(2, 6, 8, 3, device=dev), **kw)
    with pytest.raises(_lib.FgvcHipError, match="negative pad"):
        ops.yuv_planes_to_lab(y, u, v, out=torch.empty(2, 3, 6, 7, device=dev), pad=(-1, 0, 0, 0), **kw)
    assert ops.yuv_planes_to_lab(y[:0], u[:0], v[:0], **kw).shape == (0, 3, 6, 8)
    assert ops.yuv_planes_to_rgb8(y[:0], u[:0], v[:0], **kw).shape == (0, 6, 8, 3)


# ---- the trackers: packed frames with the key == the same model on ops.yuv_planes_to_lab of those frames, bit for bit --------------------------
# (the models, sizes and call forms of tests/test_gpu_yuv.py; one 16-bit format and one that is not 4:2:0)
CFG_VA = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=12, step=512, with_first_neighbor=True, batch_step=2)
CFG_HR = dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True, batch_step=2)
VA = dict(typ="VanillaTracker", strides=(1, 1, 1, 4), kw=dict(), cfg=CFG_VA)
VA4 = dict(typ="VanillaTracker", strides=(1, 2, 1, 4), kw=dict(), cfg=CFG_VA)
HR = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1), kw=dict(), cfg=CFG_HR)
HR4 = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1), kw=dict(stride=4), cfg=CFG_HR)
T, H0, W0 = 5, 42, 46
TRACKER_FORMATS = ("p010", "yuv444p")                                        # 16-bit semi-planar 4:2:0; 8-bit planar 4:4:4


def _yuv(fmt):
    kw = dict(matrix="bt709", range="limited")
    return kw if PC.FORMATS[fmt][1] == 1 else dict(kw, siting="center")


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


def _clip(dev, fmt, h0, w0, seed):
    """-> (packed frames on the device, their planes on the device)."""
    planes = PC.texture_planes(T, h0, w0, seed, fmt)
    return PC.pack(*planes, fmt).to(dev), PC.to_torch(planes, fmt, dev)


def _lab(planes, fmt, size=None):
    from fgvc_amd import ops
    return ops.yuv_planes_to_lab(*planes, **_kw(fmt, size=size, **_yuv(fmt)))


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
    h, w = size or src
    data = {k: v.to(dev) for k, v in _points(T, h, w, 6, spread).items()}
    for fmt in TRACKER_FORMATS:
        packed, planes = _clip(dev, fmt, src[0], src[1], 11)
        model = _tracker(dev, spec, input=dict(type=fmt, size=size, **_yuv(fmt)), **extra)
        got = model(test_mode=True, rgbs=packed[None], **data)
        want = model(test_mode=True, rgbs=_lab(planes, fmt, size)[None], **data)           # float frames with the key set: as ever
        _same(got, want)
        assert got[2].shape == (1, T, 6, 2) and bool(torch.isfinite(got[2]).all())
    packed16 = _clip(dev, "p010", src[0], src[1], 11)[0]
    with pytest.raises(TypeError, match="uint16.*test_cfg.input"):           # the key absent
        _tracker(dev, spec, **extra)(test_mode=True, rgbs=packed16[None], **data)
    with pytest.raises(TypeError, match="uint16.*'nv12'.*uint8"):            # the wrong dtype for the key
        _tracker(dev, spec, input=dict(type="nv12"), **extra)(test_mode=True, rgbs=packed16[None], **data)


LABEL_FORMS = dict(masks=dict(), masks_device=dict(masks="device"), guided=dict(readout=dict(type="guided", radius=2, sigma_space=1.0, sigma_range=0.1)),
                   refs=dict(refs=dict(direction="both")), coords=dict(coords=True), maps=dict(return_maps=True))
# (test_cfg.refs belongs to VanillaTracker alone)
LABEL_CASES = [(f"{n}-{form}", spec, form) for n, spec in (("vanilla", VA4), ("hr", HR4)) for form in LABEL_FORMS if (n, form) != ("hr", "refs")]


@pytest.mark.parametrize("name,spec,form", LABEL_CASES, ids=[c[0] for c in LABEL_CASES])
def test_label_calls_take_packed_frames(dev, name, spec, form):
    extra = LABEL_FORMS[form]
    h, w = H0, W0
    if form in ("coords", "maps"):
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        seg = torch.stack([torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 18.0) for cx, cy in ((12.0, 10.0), (30.5, 25.0), (40.0, 33.0))])[None].to(dev)
    else:
        a, b = torch.zeros(h, w, dtype=torch.long), torch.zeros(h, w, dtype=torch.long)
        a[8:24, 10:30], a[20:36, 25:44], b[4:16, 30:44] = 1, 2, 3
        seg = {0: a, 2: b} if form == "refs" else a[None].to(torch.uint8).to(dev)
    meta = [dict(original_shape=(h, w))]
    for fmt in TRACKER_FORMATS:
        packed, planes = _clip(dev, fmt, H0, W0, 13)
        lab = _lab(planes, fmt)                                              # (T, 3, h, w), unpadded
        model = _tracker(dev, spec, input=dict(type=fmt, **_yuv(fmt)), **extra)
        frames, _, pad = model._label_frames(packed[None, None])
        assert tuple(frames.shape) == (T, 3, 44, 48) and pad == (1, 1, 1, 1)               # padded, by the kernel
        got = model(test_mode=True, imgs=packed[None, None], ref_seg_map=seg, img_meta=meta)
        want = model(test_mode=True, imgs=lab.transpose(0, 1)[None, None].contiguous(), ref_seg_map=seg, img_meta=meta)
        _same(got, want)
    plain = _tracker(dev, spec, **extra)
    with pytest.raises(TypeError, match="uint16.*test_cfg.input"):
        plain(test_mode=True, imgs=_clip(dev, "p010", H0, W0, 13)[0][None, None], ref_seg_map=seg, img_meta=meta)


@pytest.mark.parametrize("spec", [VA4, HR4], ids=["vanilla", "hr"])
def test_flow_call_takes_packed_frames(dev, spec):
    for fmt in TRACKER_FORMATS:
        packed, planes = _clip(dev, fmt, H0, W0, 14)
        lab = _lab(planes, fmt)
        model = _tracker(dev, spec, input=dict(type=fmt, **_yuv(fmt)), flow=dict(type="window", occlusion="fb_abs"))
        got = model(test_mode=True, imgs=packed[None, None])
        want = model(test_mode=True, imgs=lab.transpose(0, 1)[None, None].contiguous())
        _same(got, want)
        assert got["flow_fw"].shape == (T - 1, 2, H0, W0)


def test_forward_warping_takes_packed_frames(dev):
    ref = torch.tensor([[[20.0, 31.5, 12.0], [18.0, 40.25, 30.0]]], device=dev)       # (1, 2, P) rows (y, x)
    for fmt in TRACKER_FORMATS:
        packed, planes = _clip(dev, fmt, H0, W0, 12)
        lab = _lab(planes, fmt)
        model = _tracker(dev, HR, input=dict(type=fmt, **_yuv(fmt)))
        got = model.forward_test_forward(packed[None, None], ref=ref)
        want = model.forward_test_forward(lab.transpose(0, 1)[None, None], ref=ref)
        _same(got, want)
        assert got[0].shape == (2, 3, T)


# ---- the demo on a C422p10 clip --------------------------------------------------------------------------------------------------------------------
def test_demo_runs_on_a_422p10_clip(dev, tmp_path):
    from PIL import Image
    from fgvc_amd import ops, viz
    from fgvc_amd.datasets import write_y4m_planes
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(ROOT, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    fmt = "yuv422p10"
    packed = PC.pack(*PC.texture_planes(4, 32, 48, 15, fmt), fmt)
    clip = str(tmp_path / "clip.y4m")
    write_y4m_planes(clip, packed, fmt, range="full")
    r = demo.main([clip, "--task", "points", "--query-points", "0", "20", "16", "1", "30", "20", "--out", str(tmp_path / "o"), "--radius", "2",
                   "--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--precede-frames", "3", "--batch-step", "2"])
    names = sorted(n for n in os.listdir(tmp_path / "o") if n.endswith(".png"))
    assert names == [f"frame_{t:05d}.png" for t in range(4)]
    rgb = ops.yuv_planes_to_rgb8(*ops.yuv_planes(packed.to(dev), fmt), **_kw(fmt, matrix="bt601", range="full", siting="left"))    # 32 rows: bt601
    assert np.array_equal(r["frames"], rgb.cpu().numpy())
    assert r["tracks"].shape == (2, 4, 2) and np.isfinite(r["tracks"]).all()
    want = viz.render(rgb.cpu().numpy(), tracks=r["tracks"], visibles=r["visibles"], radius=2)
    assert (want != r["frames"]).any()
    assert np.array_equal(np.asarray(Image.open(tmp_path / "o" / "frame_00000.png").convert("RGB")), want[0])
    assert np.array_equal(r["rendered"], want)
