"""Host tests of the input stage (test_cfg.input): the key's parsing, the trackers' refusals that need no GPU, the
datasets' raw=True form, the C ABI's argument validation and the kernel's code-object notes.  No GPU."""
import ctypes as C
import importlib.util
import os
import pickle

import numpy as np
import pytest
import torch

from tests import input_cases as IC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tracker(typ="VanillaTracker", **test_cfg):
    import fgvc_amd.mmpt_api as api
    m = api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                        test_cfg=dict(test_cfg))
    return m.eval()


def test_input_key_parsing():
    from fgvc_amd import engine
    assert engine.parse_input(None) is None
    ic = engine.parse_input(dict(type="rgb8"))
    assert ic.size is None and ic.layout == "thwc"
    ic = engine.parse_input(dict(type="rgb8", size=[64, 48], layout="tchw"))
    assert ic.size == (64, 48) and ic.layout == "tchw"
    with pytest.raises(ValueError, match="type"):
        engine.parse_input(dict(type="bgr8"))
    with pytest.raises(ValueError, match="type"):
        engine.parse_input(dict(size=(4, 4)))
    with pytest.raises(ValueError, match="layout"):
        engine.parse_input(dict(type="rgb8", layout="hwc"))
    with pytest.raises(ValueError, match="unknown key"):
        engine.parse_input(dict(type="rgb8", antialias=True))
    with pytest.raises(ValueError, match="size"):
        engine.parse_input(dict(type="rgb8", size=(0, 4)))
    with pytest.raises(ValueError, match="size"):
        engine.parse_input(dict(type="rgb8", size=(4, 4, 4)))
    with pytest.raises(TypeError):
        engine.parse_input("rgb8")


@pytest.mark.parametrize("typ", ["VanillaTracker", "HRVanillaTracker"])
def test_trackers_read_the_key_and_refuse_without_a_gpu(typ):
    """A bad key fails at construction; uint8 frames without the key raise a TypeError that names it, in every call form; with the key a
    CPU tensor meets the GPU-only rule."""
    with pytest.raises(ValueError, match="type"):
        _tracker(typ, input=dict(type="yuv"))
    with pytest.raises(ValueError, match="layout"):
        _tracker(typ, input=dict(type="rgb8", layout="nhwc"))
    m = _tracker(typ)
    assert m.input_cfg is None
    u8 = torch.zeros(1, 3, 16, 16, 3, dtype=torch.uint8)
    pts = dict(query_points=torch.zeros(1, 1, 3), trajectories=torch.zeros(1, 3, 1, 2), visibilities=torch.zeros(1, 3, 1))
    meta = [dict(original_shape=(16, 16))]
    with pytest.raises(TypeError, match="test_cfg.input"):
        m(test_mode=True, rgbs=u8, **pts)
    with pytest.raises(TypeError, match="test_cfg.input"):
        m(test_mode=True, imgs=u8[None], ref_seg_map=torch.zeros(1, 16, 16, dtype=torch.uint8), img_meta=meta)
    if typ == "HRVanillaTracker":
        with pytest.raises(TypeError, match="test_cfg.input"):
            m.forward_test_forward(u8[None], ref=torch.zeros(1, 2, 1))
    k = _tracker(typ, input=dict(type="rgb8", size=(16, 16)))
    assert k.input_cfg.size == (16, 16)
    with pytest.raises(RuntimeError, match="GPU only"):
        k(test_mode=True, rgbs=u8, **pts)
    with pytest.raises(RuntimeError, match="GPU only"):
        k(test_mode=True, imgs=u8[None], ref_seg_map=torch.zeros(1, 16, 16, dtype=torch.uint8), img_meta=meta)
    with pytest.raises(RuntimeError, match="GPU"):                           # float frames with the key set: as ever
        k(test_mode=True, rgbs=torch.zeros(1, 3, 3, 16, 16), **pts)


def test_wrapper_refusals_without_a_gpu():
    from fgvc_amd import _lib, ops
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.frames_to_lab(torch.zeros(1, 4, 4, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="layout"):
        ops.frames_to_lab(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), layout="hwc")


def test_sharded_path_refuses_uint8_frames():
    from fgvc_amd import dist, engine
    from fgvc_amd.mmpt_api.config import ConfigDict
    cfg = engine.TrackerConfig.from_test_cfg(ConfigDict(dict(precede_frames=2, topk=5, temperature=0.07, neighbor_range=8)))
    with pytest.raises(NotImplementedError, match="uint8"):
        dist.track_points_sharded(object(), torch.zeros(3, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 3), cfg)


def test_restatement_is_the_contract_in_float64():
    """tests/input_cases.preprocess_f64 follows datasets.preprocess_tapvid_frames: the CPU f32 chain stays within f32 rounding of it on every
    kernel case, and the known answers of the contract hold (black, white, the greys' zero chroma).  A guard on the reference the GPU tests
    compare against, not on the feature: the one test of this file that passes without it.  Bound: twice the largest error the CPU chain was
    seen to make on these shapes when the cases were chosen (3.8e-6, the down-scale: its f32 source coordinates)."""
    from fgvc_amd.datasets import preprocess_tapvid_frames
    for name, (frames, size, _) in IC.kernel_cases().items():
        want = IC.preprocess_f64(frames, size)
        got = preprocess_tapvid_frames(frames, size or tuple(frames.shape[1:3]))[0]
        assert got.shape == want.shape, name
        assert float((got.double() - want).abs().max()) < 8e-6, name
    g = IC.preprocess_f64(IC.greys())
    assert torch.equal(g[0, :, 0, 0], torch.tensor([-1.0, 0.0, 0.0], dtype=torch.float64))
    assert float(g[0, 1:].abs().max()) < 1e-4
    assert abs(float(g[0, 0, 15, 15]) - 1.0) < 1e-5                          # white: L = 100


def test_synthetic_raw_frames():
    from fgvc_amd.datasets import SyntheticTapVid
    a, b = SyntheticTapVid(2, 4, (32, 40), 3, seed=3)[1], SyntheticTapVid(2, 4, (32, 40), 3, seed=3, raw=True)[1]
    assert b["rgbs"].dtype == torch.uint8 and b["rgbs"].shape == (1, 4, 32, 40, 3)
    want = (128.0 + 48.0 * a["rgbs"][0]).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    assert torch.equal(b["rgbs"][0], want)
    for k in ("query_points", "trajectories", "visibilities"):
        assert torch.equal(a[k], b[k])


def test_tapvid_pickles_raw_frames(tmp_path):
    from fgvc_amd.datasets import TapVidPickles
    rng = np.random.default_rng(0)
    T, H, W = 4, 24, 36
    video = rng.integers(0, 256, (T, H, W, 3)).astype(np.uint8)
    pts = np.stack([np.linspace(0.2, 0.8, 5)[:, None].repeat(T, 1), np.linspace(0.3, 0.7, 5)[:, None].repeat(T, 1)], -1).astype(np.float32)
    with open(tmp_path / "v.pkl", "wb") as f:
        pickle.dump({"a": dict(video=video, points=pts, occluded=np.zeros((5, T), bool))}, f)
    a, b = TapVidPickles(str(tmp_path / "v.pkl"), input_size=(16, 20))[0], TapVidPickles(str(tmp_path / "v.pkl"), input_size=(16, 20), raw=True)[0]
    assert a["rgbs"].shape == (1, T, 3, 16, 20) and a["rgbs"].dtype == torch.float32
    assert b["rgbs"].dtype == torch.uint8 and b["rgbs"].shape == (1, T, H, W, 3) and np.array_equal(b["rgbs"][0].numpy(), video)
    for k in ("query_points", "trajectories", "visibilities"):
        assert torch.equal(a[k], b[k])


def test_pose_and_mask_datasets_raw_frames(tmp_path):
    from PIL import Image
    from fgvc_amd.datasets import BadjaPoses, Davis2017, JhmdbPoses
    mk = _tool("make_fake_poses")
    mk.make_jhmdb(str(tmp_path / "j"), videos=1, frames=4, size=(60, 80), seed=1)
    for form in ("points", "heatmap"):
        (a, ma), (b, mb) = (JhmdbPoses(str(tmp_path / "j"), input_size=(64, 64), form=form, raw=r)[0] for r in (False, True))
        key = "rgbs" if form == "points" else "imgs"
        lead = (1,) if form == "points" else (1, 1)
        assert b[key].dtype == torch.uint8 and b[key].shape == lead + (4, 60, 80, 3)
        assert a[key].dtype == torch.float32
        for k in a:
            if k not in (key, "img_meta"):
                assert torch.equal(a[k], b[k]), k
        assert a.get("img_meta") == b.get("img_meta") and np.array_equal(ma["gt_poses"], mb["gt_poses"])
    mk.make_badja(str(tmp_path / "b"), videos=1, frames=5, size=(64, 96), seed=2)
    for form in ("points", "heatmap"):
        (a, ma), (b, mb) = (BadjaPoses(str(tmp_path / "b"), size=(32, 48), form=form, raw=r)[0] for r in (False, True))
        key = "rgbs" if form == "points" else "imgs"
        lead = (1,) if form == "points" else (1, 1)
        assert b[key].dtype == torch.uint8 and b[key].shape == lead + (5, 64, 96, 3)
        for k in a:
            if k not in (key, "img_meta"):
                assert torch.equal(a[k], b[k]), k
        assert a.get("img_meta") == b.get("img_meta") and ma["name"] == mb["name"]
    names = _tool("make_fake_davis").make(str(tmp_path / "d"), sequences=1, frames=3, size=(48, 64), objects=2, seed=2)
    (a, ma), (b, mb) = (Davis2017(str(tmp_path / "d"), raw=r)[0] for r in (False, True))
    assert b["imgs"].dtype == torch.uint8 and b["imgs"].shape == (1, 1, 3, 48, 64, 3)
    first = np.asarray(Image.open(os.path.join(str(tmp_path / "d"), "JPEGImages", "480p", names[0], "00000.jpg")).convert("RGB"))
    assert np.array_equal(b["imgs"][0, 0, 0].numpy(), first)
    assert torch.equal(a["ref_seg_map"], b["ref_seg_map"]) and a["img_meta"] == b["img_meta"] and np.array_equal(ma["gt"], mb["gt"])
    # the default form is the torch chain on those frames, bit for bit
    from fgvc_amd.datasets import preprocess_tapvid_frames
    assert torch.equal(a["imgs"], preprocess_tapvid_frames(b["imgs"][0, 0], (48, 64)).permute(0, 2, 1, 3, 4).unsqueeze(1))


def test_input_symbol_declared_and_validates_its_arguments():
    """fgvc_frames_rgb8_to_lab_f32 is exported, listed in _lib.SIGNATURES, and returns FGVC_ERR_INVALID_ARG for a null pointer, a non-positive
    size and a negative pad before any launch (no GPU here: a launch would fail with another code)."""
    from fgvc_amd import _lib
    lib = _lib.load()
    name = "fgvc_frames_rgb8_to_lab_f32"
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    fn = getattr(lib, name)
    p = C.c_void_p(4096)                     # never dereferenced: every call below is refused on the host
    ok = dict(T=1, h0=4, w0=4, h=4, w=4, pl=0, pr=0, pt=0, pb=0)

    def call(src=p, dst=p, **kw):
        a = dict(ok, **kw)
        return fn(src, a["T"], a["h0"], a["w0"], 48, 12, 3, 1, a["h"], a["w"], a["pl"], a["pr"], a["pt"], a["pb"], dst, None)

    assert call(src=None) == _lib.ERR_INVALID_ARG and b"null pointer" in lib.fgvc_last_error()
    assert call(dst=None) == _lib.ERR_INVALID_ARG
    for k in ("T", "h0", "w0", "h", "w"):
        for v in (0, -3):
            assert call(**{k: v}) == _lib.ERR_INVALID_ARG, (k, v)
            assert b"non-positive size" in lib.fgvc_last_error()
    for k in ("pl", "pr", "pt", "pb"):
        assert call(**{k: -1}) == _lib.ERR_INVALID_ARG, k
        assert b"negative pad" in lib.fgvc_last_error()


def test_input_kernel_uses_no_scratch():
    """The two instantiations of the input kernel (resize; same size) in the code-object notes of the built library: no scratch memory, no
    spilled register; the sRGB table is the 1 KiB of LDS of the same-size one."""
    notes = _tool("kernel_notes").kernel_notes()
    ks = {k: v for k, v in notes.items() if "frames_rgb8_to_lab_kernel" in k}
    assert len(ks) == 2, sorted(ks)
    for k, v in ks.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    assert sorted(v["group_segment_fixed_size"] for v in ks.values()) == [0, 1024]
