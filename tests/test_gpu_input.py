"""GPU: the input stage (fgvc_frames_rgb8_to_lab_f32, ops.frames_to_lab, test_cfg.input).

The kernel against the float64 restatement of the input contract (tests/input_cases.py), with the torch f32 chain on the same GPU as the
yardstick of the error: E_kernel <= max(2 E_chain, 2^-22) per case (two f32 math libraries, each good to an ulp or two in pow and cbrt,
legitimately differ by a factor of two; the floor guards a case on which the chain happens to be exact).  Exact checks without a tolerance
for everything that is plumbing: the zero border, the layouts, views, `out=`, streams, and every call form of both trackers."""
import numpy as np
import pytest
import torch

from tests import input_cases as IC

pytestmark = pytest.mark.gpu
CASES = IC.kernel_cases()


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def references():
    """name -> the float64 restatement (T, 3, h, w) on the CPU, computed once and never written to."""
    return {name: IC.preprocess_f64(frames, size) for name, (frames, size, _) in CASES.items()}


def _interior(out, pad, h, w):
    left, right, top, bottom = pad
    return out[:, :, top:top + h, left:left + w]


@pytest.mark.parametrize("name", list(CASES))
def test_kernel_within_twice_the_chains_error(dev, references, name):
    from fgvc_amd import ops
    from fgvc_amd.datasets import preprocess_tapvid_frames
    frames, size, pad = CASES[name]
    want = references[name]
    h, w = want.shape[-2:]
    chain = preprocess_tapvid_frames(frames.to(dev), (h, w))[0]
    got = ops.frames_to_lab(frames.to(dev), size, pad)
    assert got.dtype == torch.float32 and got.shape == (frames.shape[0], 3, pad[2] + h + pad[3], pad[0] + w + pad[1])
    e_chain = float((chain.cpu().double() - want).abs().max())
    e_kernel = float((_interior(got, pad, h, w).cpu().double() - want).abs().max())
    bound = max(2 * e_chain, IC.ERROR_FLOOR)
    print(f"[input] {name}: E_chain = {e_chain:.3e}, E_kernel = {e_kernel:.3e}, bound = {bound:.3e}")
    assert e_kernel <= bound, (name, e_kernel, e_chain)
    border = got.clone()
    _interior(border, pad, h, w).zero_()
    assert torch.equal(border.view(torch.int32), torch.zeros_like(border, dtype=torch.int32)), name     # +0.0 bit for bit


def test_black_is_exact_and_greys_have_no_chroma(dev):
    from fgvc_amd import ops
    g = ops.frames_to_lab(IC.greys().to(dev)).cpu()
    assert torch.equal(g[0, :, 0, 0], torch.tensor([-1.0, 0.0, 0.0]))
    assert float(g[0, 1:].abs().max()) < 1e-4
    black = ops.frames_to_lab(torch.zeros(2, 5, 7, 3, dtype=torch.uint8, device=dev), (9, 11), (1, 0, 0, 2)).cpu()
    want = torch.zeros(2, 3, 11, 12)
    want[:, 0, :9, 1:] = -1.0
    assert torch.equal(black, want)


@pytest.mark.parametrize("size,pad", [(None, (1, 2, 0, 1)), ((9, 13), (0, 3, 1, 0)), (None, (5, 3, 2, 2))])
def test_padded_interior_equals_unpadded_call(dev, size, pad):
    from fgvc_amd import ops
    frames = IC.texture_u8(2, 16, 20, 4).to(dev)
    plain = ops.frames_to_lab(frames, size)
    padded = ops.frames_to_lab(frames, size, pad)
    h, w = plain.shape[-2:]
    assert torch.equal(_interior(padded, pad, h, w), plain)
    _interior(padded, pad, h, w).zero_()
    assert int(padded.view(torch.int32).abs().max()) == 0                      # the border: +0.0 bit for bit


@pytest.mark.parametrize("size", [None, (24, 40)])
def test_layouts_and_views_give_identical_bits(dev, size):
    """thwc, tchw, a non-contiguous crop of a larger tensor in either layout, every byte alignment of the crop's first column, `out=` and a
    second stream: the same bits."""
    from fgvc_amd import ops
    big = IC.texture_u8(3, 45, 61, 6).to(dev)                                 # (3, 45, 61, 3)
    for x0 in (4, 5, 6, 7):                                                    # the packed route's dword / halfword / byte loads
        crop = big[:, 3:40, x0:x0 + 53]
        assert not crop.is_contiguous()
        want = ops.frames_to_lab(crop.contiguous(), size)
        assert torch.equal(ops.frames_to_lab(crop, size), want), x0
        planar = big.permute(0, 3, 1, 2).contiguous()                         # (3, 3, 45, 61)
        assert torch.equal(ops.frames_to_lab(planar[:, :, 3:40, x0:x0 + 53], size, layout="tchw"), want), x0
        assert torch.equal(ops.frames_to_lab(crop.permute(0, 3, 1, 2), size, layout="tchw"), want), x0
    out = torch.full_like(want, float("nan"))
    assert ops.frames_to_lab(crop, size, out=out) is out and torch.equal(out, want)
    assert torch.equal(ops.frames_to_lab(big[1:, 3:40, 7:60], size), want[1:])             # a time slice
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        again = ops.frames_to_lab(crop, size)
    s.synchronize()
    assert torch.equal(again, want)


def test_wrapper_refusals(dev):
    from fgvc_amd import _lib, ops
    u8 = torch.zeros(2, 6, 8, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.frames_to_lab(u8.cpu())
    with pytest.raises(TypeError, match="uint8"):
        ops.frames_to_lab(u8.float())
    with pytest.raises(ValueError, match="3 channels"):
        ops.frames_to_lab(torch.zeros(2, 6, 8, 4, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="3 channels"):
        ops.frames_to_lab(u8, layout="tchw")                                  # (2, 6, 8, 3) read as (T, C, h, w): 6 channels
    with pytest.raises(ValueError, match="out"):
        ops.frames_to_lab(u8, out=torch.empty(2, 3, 6, 9, device=dev))
    with pytest.raises(ValueError, match="out"):
        ops.frames_to_lab(u8, out=torch.empty(2, 3, 6, 8, device=dev, dtype=torch.float64))
    with pytest.raises(_lib.FgvcHipError, match="negative pad"):
        ops.frames_to_lab(u8, out=torch.empty(2, 3, 6, 7, device=dev), pad=(-1, 0, 0, 0))
    assert ops.frames_to_lab(u8[:0]).shape == (0, 3, 6, 8)


# ---- the trackers: uint8 frames with the key == the same model on ops.frames_to_lab of those frames, bit for bit --------------------------
VA = dict(typ="VanillaTracker", strides=(1, 1, 1, 4),
          cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=12, step=512, with_first_neighbor=True, batch_step=2))
HR = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1),
          cfg=dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True, batch_step=2))


def _tracker(dev, spec, **extra):
    from oracle import fgvc_oracle as O
    import fgvc_amd.mmpt_api as api
    model = api.build_model(dict(type=spec["typ"], backbone=dict(type="ResNet", depth=18, strides=spec["strides"], out_indices=(2,),
                                                                 pool_type="none")),
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
    if isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            _same(x, y)
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and torch.equal(a, b)
    else:
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


POINT_CASES = [
    ("vanilla", VA, dict(), (64, 64), None, "thwc", False),
    ("vanilla_regrouped", VA, dict(with_first=True), (64, 64), None, "tchw", True),
    ("vanilla_occlusion", VA, dict(with_first=True, occlusion=dict(type="cycle")), (64, 64), None, "thwc", True),
    ("vanilla_resized", VA, dict(with_first=True), (96, 128), (64, 64), "thwc", True),
    ("hr", HR, dict(with_first=False), (48, 64), None, "thwc", False),
    ("hr_regrouped_occlusion", HR, dict(occlusion=dict(type="cycle")), (48, 64), None, "tchw", True),
]


@pytest.mark.parametrize("name,spec,extra,src,size,layout,spread", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_points_call_takes_uint8_frames(dev, name, spec, extra, src, size, layout, spread):
    from fgvc_amd import ops
    T = 4 if spec is VA else 5
    u8 = IC.texture_u8(T, src[0], src[1], 11).to(dev)                         # (T, h0, w0, 3)
    model = _tracker(dev, spec, input=dict(type="rgb8", size=size, layout=layout), **extra)
    h, w = size or src
    data = {k: v.to(dev) for k, v in _points(T, h, w, 6, spread).items()}
    raw = (u8 if layout == "thwc" else u8.permute(0, 3, 1, 2).contiguous()).unsqueeze(0)
    got = model(test_mode=True, rgbs=raw, **data)
    err = model.last_cycle_error
    want = model(test_mode=True, rgbs=ops.frames_to_lab(u8, size).unsqueeze(0), **data)       # float frames with the key set: as ever
    _same(got, want)
    assert got[2].shape == (1, T, 6, 2) and bool(torch.isfinite(got[2]).all())
    if "occlusion" in extra:
        assert err is not None and torch.equal(err, model.last_cycle_error)
    plain = _tracker(dev, spec, **extra)
    with pytest.raises(TypeError, match="test_cfg.input"):
        plain(test_mode=True, rgbs=raw, **data)


def test_forward_warping_takes_uint8_frames(dev):
    from fgvc_amd import ops
    u8 = IC.texture_u8(5, 48, 64, 12).to(dev)
    model = _tracker(dev, HR, input=dict(type="rgb8"))
    ref = torch.tensor([[[20.0, 31.5, 12.0], [18.0, 40.25, 50.0]]], device=dev)       # (1, 2, P) rows (y, x)
    got = model.forward_test_forward(u8[None, None], ref=ref)
    lab = ops.frames_to_lab(u8)
    want = model.forward_test_forward(lab.transpose(0, 1)[None, None], ref=ref)
    _same(got, want)
    assert got[0].shape == (2, 3, 5)


LABEL_CASES = [("masks", dict()), ("coords", dict(coords=True)), ("maps", dict(return_maps=True))]


@pytest.mark.parametrize("spec", [VA, HR], ids=["vanilla", "hr"])
@pytest.mark.parametrize("form,extra", LABEL_CASES, ids=[c[0] for c in LABEL_CASES])
def test_label_calls_take_uint8_frames(dev, spec, form, extra):
    """5 x 41 x 47: both sides are padded (to 42 x 48 by either tracker's unit), by the kernel in the uint8 call and by F.pad of the unpadded
    conversion in the float call."""
    from fgvc_amd import ops
    T, h, w = 5, 41, 47
    u8 = IC.texture_u8(T, h, w, 13).to(dev)
    layout = "tchw" if form == "coords" else "thwc"
    model = _tracker(dev, spec, input=dict(type="rgb8", layout=layout), **extra)
    if form == "masks":
        seg = torch.zeros(1, h, w, dtype=torch.uint8)
        seg[0, 8:24, 10:30], seg[0, 20:36, 25:44] = 1, 2
    else:
        yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
        seg = torch.stack([torch.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / 18.0) for cx, cy in ((12.0, 10.0), (30.5, 25.0), (40.0, 33.0))])[None]
    seg, meta = seg.to(dev), [dict(original_shape=(h, w))]
    raw = (u8 if layout == "thwc" else u8.permute(0, 3, 1, 2).contiguous())[None, None]
    got = model(test_mode=True, imgs=raw, ref_seg_map=seg, img_meta=meta)
    lab = ops.frames_to_lab(u8)                                               # (T, 3, h, w), unpadded
    want = model(test_mode=True, imgs=lab.transpose(0, 1)[None, None].contiguous(), ref_seg_map=seg, img_meta=meta)
    _same(got, want)
    assert got[0].shape == {"masks": (T, h, w), "coords": (2, 3, T), "maps": (T, 3, h, w)}[form]
    plain = _tracker(dev, spec, **extra)
    with pytest.raises(TypeError, match="test_cfg.input"):
        plain(test_mode=True, imgs=raw, ref_seg_map=seg, img_meta=meta)


def test_sharded_path_refuses_uint8_frames(dev):
    from fgvc_amd import dist
    model = _tracker(dev, VA, input=dict(type="rgb8"))
    with pytest.raises(NotImplementedError, match="uint8"):
        dist.track_points_sharded(object(), torch.zeros(4, 64, 64, 3, dtype=torch.uint8, device=dev), torch.zeros(2, 3), model.engine_config())
