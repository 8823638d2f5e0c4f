"""Host tests of the YUV 4:2:0 input stage (test_cfg.input type='nv12' | 'i420'): the key's parsing, the trackers'
shape refusals, the coefficients, the Y4M reader and writer, the torch contract against the numpy float32 restatement, the C ABI's argument
validation, the kernels' code-object notes and the demo's argument parsing.  No GPU.  Except for the guards on the restatements and on
the tie case (marked in their docstrings) every test here fails without the feature."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import yuv_cases as YC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tracker(typ="VanillaTracker", **test_cfg):
    import fgvc_amd.mmpt_api as api
    m = api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                        test_cfg=dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, **test_cfg))
    return m.eval()


# ---- the key ----------------------------------------------------------------------------------------------------------------------------------
def test_input_key_parsing_yuv():
    from fgvc_amd import engine
    for typ in ("nv12", "i420"):
        ic = engine.parse_input(dict(type=typ))
        assert (ic.type, ic.size, ic.matrix, ic.range, ic.siting, ic.yuv) == (typ, None, "bt601", "limited", "left", True)
    ic = engine.parse_input(dict(type="nv12", size=[64, 48], matrix="bt709", range="full", siting="center"))
    assert (ic.size, ic.matrix, ic.range, ic.siting) == ((64, 48), "bt709", "full", "center")
    with pytest.raises(ValueError, match="layout"):
        engine.parse_input(dict(type="nv12", layout="thwc"))
    with pytest.raises(ValueError, match="matrix"):
        engine.parse_input(dict(type="i420", matrix="bt2020"))
    with pytest.raises(ValueError, match="range"):
        engine.parse_input(dict(type="i420", range="tv"))
    with pytest.raises(ValueError, match="siting"):
        engine.parse_input(dict(type="i420", siting="topleft"))
    with pytest.raises(ValueError, match="unknown key"):
        engine.parse_input(dict(type="i420", antialias=True))
    with pytest.raises(ValueError, match="size"):
        engine.parse_input(dict(type="nv12", size=(0, 4)))
    # rgb8: nothing changes -- the YUV keys stay unknown there, the positional constructor stays, other types stay refused
    for key in ("matrix", "range", "siting"):
        with pytest.raises(ValueError, match="unknown key"):
            engine.parse_input(dict(type="rgb8", **{key: "bt601"}))
    ic = engine.parse_input(dict(type="rgb8", size=(8, 6), layout="tchw"))
    assert (ic.size, ic.layout, ic.type, ic.yuv) == ((8, 6), "tchw", "rgb8", False)
    ic = engine.InputConfig((4, 6), "tchw")
    assert ic.size == (4, 6) and ic.layout == "tchw" and ic.type == "rgb8"
    for typ in ("yuv", "bgr8", "nv21", "p010", None):
        with pytest.raises(ValueError, match="type"):
            engine.parse_input(dict(type=typ))


@pytest.mark.parametrize("typ", ["VanillaTracker", "HRVanillaTracker"])
def test_trackers_refuse_bad_packed_shapes(typ):
    """The shape errors are ValueErrors that state the expected shape, raised before anything touches the device; CPU frames of the right
    shape meet the GPU-only rule, and uint8 frames without the key the unchanged TypeError."""
    with pytest.raises(ValueError, match="layout"):
        _tracker(typ, input=dict(type="nv12", layout="thwc"))
    pts = dict(query_points=torch.zeros(1, 1, 3), trajectories=torch.zeros(1, 3, 1, 2), visibilities=torch.zeros(1, 3, 1))
    meta = [dict(original_shape=(16, 16))]
    seg = torch.zeros(1, 16, 16, dtype=torch.uint8)
    good = torch.zeros(1, 3, 24, 16, dtype=torch.uint8)                      # (1, T, 3 h0 / 2, w0): 16 x 16
    plain = _tracker(typ)
    with pytest.raises(TypeError, match="test_cfg.input"):
        plain(test_mode=True, rgbs=good, **pts)
    for fmt in ("nv12", "i420"):
        m = _tracker(typ, input=dict(type=fmt, siting="center"))
        assert m.input_cfg.type == fmt and m.input_cfg.siting == "center"
        with pytest.raises(RuntimeError, match="GPU only"):
            m(test_mode=True, rgbs=good, **pts)
        with pytest.raises(RuntimeError, match="GPU only"):
            m(test_mode=True, imgs=good[None], ref_seg_map=seg, img_meta=meta)

    class OnDevice(torch.Tensor):                                            # a CPU tensor that claims to be on the GPU: the shape checks come first
        is_cuda = True

    def dev(t):
        return t.as_subclass(OnDevice)

    m = _tracker(typ, input=dict(type="i420"))
    for bad in (torch.zeros(1, 3, 16, 16, 3, dtype=torch.uint8), torch.zeros(3, 24, 16, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\(1, T, 3 h0 / 2, w0\)"):
            m(test_mode=True, rgbs=dev(bad), **pts)
    for bad in (torch.zeros(1, 3, 25, 16, dtype=torch.uint8), torch.zeros(1, 3, 24, 15, dtype=torch.uint8)):       # rows no multiple of 3; an odd width
        with pytest.raises(ValueError, match="3 h0 / 2, w0"):
            m(test_mode=True, rgbs=dev(bad), **pts)
    for bad in (torch.zeros(1, 1, 3, 16, 16, 3, dtype=torch.uint8), torch.zeros(1, 1, 24, 16, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"\(1, 1, T, 3 h0 / 2, w0\)"):
            m(test_mode=True, imgs=dev(bad), ref_seg_map=seg, img_meta=meta)
    if typ == "HRVanillaTracker":
        with pytest.raises(ValueError, match=r"\(1, 1, T, 3 h0 / 2, w0\)"):
            m.forward_test_forward(dev(torch.zeros(1, 1, 24, 16, dtype=torch.uint8)), ref=torch.zeros(1, 2, 1))


# ---- ops without a GPU --------------------------------------------------------------------------------------------------------------------------
def test_coefficients_match_the_published_figures():
    from fgvc_amd import ops
    got = ops.yuv_coefficients("bt601", "limited")
    assert got[0] == 16.0
    for g, w in zip(got[1:], (1.164384, 1.596027, -0.391762, -0.812968, 2.017232)):
        assert abs(g - w) < 1e-6, (g, w)
    assert ops.yuv_coefficients("bt601", "full")[:2] == (0.0, 1.0)
    for g, w in zip(ops.yuv_coefficients("bt709", "full")[2:], (1.5748, -0.187324, -0.468124, 1.8556)):
        assert abs(g - w) < 1e-6, (g, w)
    for matrix in YC.MATRICES:
        for rng in YC.RANGES:
            assert ops.yuv_coefficients(matrix, rng) == YC.coefficients_f64(matrix, rng)
    with pytest.raises(ValueError, match="matrix"):
        ops.yuv_coefficients("bt2020", "limited")
    with pytest.raises(ValueError, match="range"):
        ops.yuv_coefficients("bt601", "pc")


def test_planes_are_views_of_the_packed_frames():
    from fgvc_amd import ops
    y, u, v = YC.texture_planes(3, 16, 20, 1)
    for fmt in YC.FORMATS:
        packed = YC.pack(y, u, v, fmt)
        assert packed.shape == (3, 24, 20)
        py, pu, pv = ops.yuv420_planes(packed, fmt)
        assert torch.equal(py, y) and torch.equal(pu, u) and torch.equal(pv, v), fmt
        base = packed.untyped_storage().data_ptr()
        assert all(p.untyped_storage().data_ptr() == base for p in (py, pu, pv)), fmt           # no copy
        assert pu.stride() == pv.stride() and pu.stride(2) == (2 if fmt == "nv12" else 1)
        sy, su, sv = ops.yuv420_planes(packed[::2], fmt)                                           # a time slice stays a view
        assert torch.equal(su, u[::2]) and torch.equal(sv, v[::2]) and su.untyped_storage().data_ptr() == base
    for bad in (torch.zeros(2, 25, 20, dtype=torch.uint8), torch.zeros(2, 24, 19, dtype=torch.uint8), torch.zeros(2, 0, 20, dtype=torch.uint8),
                torch.zeros(24, 20, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="3 h0 / 2, w0"):
            ops.yuv420_planes(bad, "nv12")
    with pytest.raises(ValueError, match="fmt"):
        ops.yuv420_planes(torch.zeros(2, 24, 20, dtype=torch.uint8), "yv12")


def test_wrapper_refusals_without_a_gpu():
    from fgvc_amd import _lib, ops
    y, u, v = YC.texture_planes(1, 4, 4, 1)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.yuv_frames_to_lab(y, u, v)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.yuv_frames_to_rgb8(y, u, v)


# ---- the contract as torch ops ------------------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_decode():
    from fgvc_amd.datasets import yuv420_to_rgb, yuv420_to_rgb8

    def px(Y, U, V):
        return tuple(torch.tensor([[[c]]], dtype=torch.uint8) for c in (Y, U, V))

    assert yuv420_to_rgb(*px(235, 128, 128))[0, :, 0, 0].tolist() == [255.0, 255.0, 255.0]
    assert yuv420_to_rgb(*px(16, 128, 128))[0, :, 0, 0].tolist() == [0.0, 0.0, 0.0]
    red = yuv420_to_rgb(*px(81, 90, 240))[0, :, 0, 0]                        # unclamped, unrounded
    assert torch.allclose(red, torch.tensor([254.44, -0.48, -0.97]), atol=5e-3)
    for yuv, rgb in (((81, 90, 240), (254, 0, 0)), ((145, 54, 34), (0, 255, 1)), ((41, 240, 110), (0, 0, 255)),
                     ((235, 128, 128), (255, 255, 255)), ((16, 128, 128), (0, 0, 0))):
        assert tuple(yuv420_to_rgb8(*px(*yuv))[0, 0, 0].tolist()) == rgb, yuv
    grey = torch.arange(256, dtype=torch.uint8).view(1, 16, 16)
    neutral = torch.full((1, 8, 8), 128, dtype=torch.uint8)
    assert torch.equal(yuv420_to_rgb8(grey, neutral, neutral, range="full"), grey[..., None].expand(1, 16, 16, 3))


@pytest.mark.parametrize("name", list(YC.kernel_cases()))
def test_torch_bytes_equal_the_float32_restatement(name):
    from fgvc_amd.datasets import yuv420_to_rgb8
    (y, u, v), _, _, matrix, rng, siting, fmt = YC.kernel_cases()[name]
    u, v = YC.in_format(u, v, fmt)
    got = yuv420_to_rgb8(y, u, v, matrix, rng, siting)
    want = YC.rgb8_f32(*YC.np_planes((y, u, v)), matrix, rng, siting)
    assert got.shape == want.shape and np.array_equal(got.numpy(), want), name


def test_guard_cpu_chain_within_rounding_of_the_float64_restatement():
    """A guard on the restatement, not on the feature's kernels: datasets.preprocess_yuv420_frames on the CPU stays within 8e-6 of
    yuv_cases.preprocess_f64 on every case (DESIGN.md section 14's guard figure for the same shapes).  The Lab half of both is the parent's
    arithmetic."""
    from fgvc_amd.datasets import preprocess_yuv420_frames
    worst = 0.0
    for name, ((y, u, v), size, _, matrix, rng, siting, fmt) in YC.kernel_cases().items():
        if fmt != "i420":                                                    # (the layout does not enter a CPU chain)
            continue
        want = YC.preprocess_f64(*YC.np_planes((y, u, v)), size, matrix, rng, siting)
        got = preprocess_yuv420_frames(y, u, v, size, matrix, rng, siting)[0]
        assert got.shape == want.shape, name
        e = float((got.double() - want).abs().max())
        worst = max(worst, e)
        assert e < 8e-6, (name, e)
    print(f"[yuv] CPU f32 chain against float64: worst {worst:.3e}")


def test_guard_float32_and_float64_bytes_rarely_differ():
    """A guard on the two restatements (it passes on the parent's arithmetic: it calls nothing of the feature): on the lattice the float32
    order and float64 round to a different byte on fewer than 1e-4 of the values."""
    planes = YC.np_planes(YC.lattice_planes())
    for matrix in YC.MATRICES:
        for rng in YC.RANGES:
            for siting in YC.SITINGS:
                a, b = YC.rgb8_f32(*planes, matrix, rng, siting), YC.rgb8_f64(*planes, matrix, rng, siting)
                assert int(np.abs(a.astype(np.int16) - b).max()) <= 1
                assert float((a != b).mean()) < 1e-4, (matrix, rng, siting)


def test_guard_tie_case_separates_the_rounding_rules():
    """A guard on a case, not on the feature (it calls nothing of it): on yuv_cases.tie_planes the float32 restatement has exact ties in B,
    where half-up rounding, a fused multiply-add (emulated: the product exact in float64, one rounding to float32) each give
    other bytes than the contract's half-to-even on the float32 order."""
    f = np.float32
    planes = YC.np_planes(YC.tie_planes())
    rgb = YC.rgb_f32(*planes, "bt601", "full")
    want = YC.rgb8_f32(*planes, "bt601", "full")
    inside = (rgb[..., 2] > 0) & (rgb[..., 2] < 255)
    assert int((inside & (rgb[..., 2] % 1 == f(0.5))).sum()) == 34 + 34                  # Y = 222 .. 255 over U = 3, Y = 0 .. 33 over U = 253
    half_up = np.floor(np.clip(rgb, f(0), f(255)) + f(0.5)).astype(np.uint8)
    assert int((half_up != want).sum()) == 34                                           # the ties above an even byte
    cbu = f(YC.coefficients_f64("bt601", "full")[5])
    fused = (planes[0].astype(np.float64) + np.float64(cbu) * (planes[1].astype(np.float64).repeat(2, 1).repeat(2, 2) - 128.0)).astype(f)
    assert int((np.rint(np.clip(fused, f(0), f(255))).astype(np.uint8) != want[..., 2]).sum()) >= 16


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------------------------
def _y4m(path, header, frames=(b"",), frame_tag=b"FRAME\n"):
    with open(path, "wb") as fh:
        fh.write(header)
        for f in frames:
            fh.write(frame_tag + f)
    return str(path)


def test_y4m_round_trip_and_tags(tmp_path):
    from fgvc_amd.datasets import read_y4m, write_y4m
    frames = YC.packed_texture(3, 16, 20, 2, "i420")
    for siting, tag in (("left", b"C420mpeg2"), ("center", b"C420jpeg")):
        for rng in ("limited", "full"):
            p = str(tmp_path / f"{siting}_{rng}.y4m")
            write_y4m(p, frames, fps=(25, 1), siting=siting, range=rng)
            head = open(p, "rb").readline()
            assert head.startswith(b"YUV4MPEG2 W20 H16 F25:1 Ip") and tag in head.split() and b"XCOLORRANGE=" + rng.upper().encode() in head.split()
            got, info = read_y4m(p)
            assert got.dtype == torch.uint8 and torch.equal(got, frames)
            assert info == dict(width=20, height=16, fps=(25, 1), siting=siting, range=rng)
    assert os.path.getsize(p) == len(head) + 3 * (6 + 16 * 20 * 3 // 2)
    got, _ = read_y4m(p, max_frames=2)
    assert torch.equal(got, frames[:2])
    assert read_y4m(p, max_frames=0)[0].shape == (0, 24, 20)
    write_y4m(p, frames.numpy())                                             # an array; the defaults
    assert read_y4m(p)[1] == dict(width=20, height=16, fps=(30, 1), siting="left", range="limited")
    with pytest.raises(ValueError, match="packed I420"):
        write_y4m(p, torch.zeros(2, 25, 20, dtype=torch.uint8))
    # what other writers leave out or add: no C tag is 4:2:0 'jpeg'; plain C420 is 'mpeg2'; no range tag is limited; FRAME may carry parameters
    body = bytes(range(24)) * 1                                              # 4 x 4: 16 + 4 + 4 bytes
    g, info = read_y4m(_y4m(tmp_path / "bare.y4m", b"YUV4MPEG2 W4 H4 F30000:1001\n", [body, body], b"FRAME Ip\n"))
    assert info == dict(width=4, height=4, fps=(30000, 1001), siting="center", range="limited") and g.shape == (2, 6, 4)
    assert g[1].reshape(-1).tolist() == list(range(24))
    assert read_y4m(_y4m(tmp_path / "c420.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip A1:1 C420 XYSCSS=420\n", [body]))[1]["siting"] == "left"
    assert read_y4m(_y4m(tmp_path / "full.y4m", b"YUV4MPEG2 W4 H4 F25:1 C420jpeg XCOLORRANGE=FULL\n", [body]))[1]["range"] == "full"


def test_y4m_refusals(tmp_path):
    from fgvc_amd.datasets import read_y4m
    body = bytes(24)
    for tag in ("C422", "C444", "C420p10", "Cmono", "C420paldv"):
        with pytest.raises(ValueError, match=tag):
            read_y4m(_y4m(tmp_path / "c.y4m", f"YUV4MPEG2 W4 H4 F25:1 Ip {tag}\n".encode(), [body]))
    for tag in ("It", "Ib", "Im"):
        with pytest.raises(ValueError, match=tag):
            read_y4m(_y4m(tmp_path / "i.y4m", f"YUV4MPEG2 W4 H4 F25:1 {tag} C420jpeg\n".encode(), [body]))
    for size in ("W5 H4", "W4 H3"):
        with pytest.raises(ValueError, match="odd size"):
            read_y4m(_y4m(tmp_path / "o.y4m", f"YUV4MPEG2 {size} F25:1 Ip\n".encode(), [bytes(30)]))
    with pytest.raises(ValueError, match="truncated"):
        read_y4m(_y4m(tmp_path / "t.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip\n", [body, body[:23]]))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        read_y4m(_y4m(tmp_path / "n.y4m", b"RIFF W4 H4\n", [body]))
    with pytest.raises(ValueError, match="FRAME"):
        read_y4m(_y4m(tmp_path / "f.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip\n", [body], b"FRANE\n"))
    with pytest.raises(ValueError, match="XCOLORRANGE"):
        read_y4m(_y4m(tmp_path / "r.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip XCOLORRANGE=TV\n", [body]))
    with pytest.raises(ValueError, match="size"):
        read_y4m(_y4m(tmp_path / "s.y4m", b"YUV4MPEG2 F25:1 Ip\n", [body]))


# ---- the library --------------------------------------------------------------------------------------------------------------------------------
def test_yuv_symbols_declared_and_validate_their_arguments():
    """Both entry points are exported and listed in _lib.SIGNATURES, input_yuv.hip is a build source, and a null pointer, a non-positive
    size, a negative pad, a bad siting and a shape beyond the grid return FGVC_ERR_INVALID_ARG with a message that names the entry point,
    before any launch (no GPU here: a launch would fail with another code)."""
    from fgvc_amd import _lib, build
    assert "input_yuv.hip" in build.SOURCES
    lib = _lib.load()
    p = C.c_void_p(4096)                     # never dereferenced: every call below is refused on the host
    coef = (16.0, 1.16, 1.6, -0.39, -0.81, 2.02)
    ok = dict(y=p, u=p, v=p, out=p, T=1, h0=4, w0=4, h=4, w=4, pl=0, pr=0, pt=0, pb=0, siting=0)

    def lab(**kw):
        a = dict(ok, **kw)
        return lib.fgvc_frames_yuv420_to_lab_f32(a["y"], a["u"], a["v"], a["T"], a["h0"], a["w0"], 16, 4, 8, 4, 2, *coef, a["siting"], a["h"], a["w"],
                                                 a["pl"], a["pr"], a["pt"], a["pb"], a["out"], None)

    def rgb(**kw):
        a = dict(ok, **kw)
        return lib.fgvc_frames_yuv420_to_rgb8(a["y"], a["u"], a["v"], a["T"], a["h0"], a["w0"], 16, 4, 8, 4, 2, *coef, a["siting"], a["out"], None)

    for name, fn, sizes in (("fgvc_frames_yuv420_to_lab_f32", lab, ("T", "h0", "w0", "h", "w")), ("fgvc_frames_yuv420_to_rgb8", rgb, ("T", "h0", "w0"))):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        for ptr in ("y", "u", "v", "out"):
            assert fn(**{ptr: None}) == _lib.ERR_INVALID_ARG, (name, ptr)
            assert lib.fgvc_last_error().startswith(name.encode() + b": null pointer")
        for k in sizes:
            for val in (0, -3):
                assert fn(**{k: val}) == _lib.ERR_INVALID_ARG, (name, k, val)
                assert lib.fgvc_last_error().startswith(name.encode() + b": non-positive size")
        for s in (-1, 2):
            assert fn(siting=s) == _lib.ERR_INVALID_ARG and lib.fgvc_last_error().startswith(name.encode() + b": siting")
        assert fn(T=65536) == _lib.ERR_INVALID_ARG and lib.fgvc_last_error().startswith(name.encode() + b": shape beyond the launch grid")
        assert fn(h0=1 << 18, h=1 << 18) == _lib.ERR_INVALID_ARG and b"launch grid" in lib.fgvc_last_error()
    for k in ("pl", "pr", "pt", "pb"):
        assert lab(**{k: -1}) == _lib.ERR_INVALID_ARG, k
        assert lib.fgvc_last_error().startswith(b"fgvc_frames_yuv420_to_lab_f32: negative pad")


def test_yuv_kernels_use_no_scratch():
    """The three fixed-format kernels (Yuv420 -- Lab: resize and same size; bytes) in the code-object notes of the built library: no scratch
    memory, no spilled register, no LDS, and no more registers than they had as a file of their own (153 / 72 / 65 VGPRs: the next
    occupancy steps)."""
    notes = _tool("kernel_notes").kernel_notes()
    lab = {k: v for k, v in notes.items() if "frames_yuv_to_lab_kernel" in k and "Yuv420" in k}
    rgb = {k: v for k, v in notes.items() if "frames_yuv_to_rgb8_kernel" in k and "Yuv420" in k}
    assert len(lab) == 2 and len(rgb) == 1, (sorted(lab), sorted(rgb))
    for k, v in {**lab, **rgb}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)
    resize, same = (next(v for k, v in lab.items() if flag in k) for flag in ("Lb1E", "Lb0E"))       # <Yuv420, RESIZE>
    assert resize["vgpr_count"] <= 153 and same["vgpr_count"] <= 72 and next(iter(rgb.values()))["vgpr_count"] <= 65, (lab, rgb)


# ---- the demo -----------------------------------------------------------------------------------------------------------------------------------
def test_demo_takes_a_y4m_clip(tmp_path):
    from fgvc_amd.datasets import write_y4m
    demo = _tool("demo")
    clip = str(tmp_path / "clip.y4m")
    write_y4m(clip, YC.packed_texture(2, 16, 20, 3, "i420"), siting="center")
    a = demo.parse_args([clip, "--task", "points", "--query-points", "0", "5", "5", "--out", str(tmp_path / "o")])
    assert a.frames == clip and a.yuv_matrix is None and demo.is_y4m(a.frames)
    a = demo.parse_args([clip, "--task", "points", "--query-points", "0", "5", "5", "--out", "o", "--yuv-matrix", "bt709"])
    assert a.yuv_matrix == "bt709"
    assert [demo.yuv_matrix_default(h) for h in (16, 480, 719, 720, 1080, 2160)] == ["bt601", "bt601", "bt601", "bt709", "bt709", "bt709"]
    assert not demo.is_y4m(str(tmp_path)) and not demo.is_y4m(None)
    with pytest.raises(SystemExit):
        demo.parse_args([clip, "--task", "points", "--query-points", "0", "5", "5", "--out", "o", "--yuv-matrix", "bt2020"])
    with pytest.raises(SystemExit):                                          # a matrix for RGB stills says nothing
        demo.parse_args([str(tmp_path), "--task", "points", "--query-points", "0", "5", "5", "--out", "o", "--yuv-matrix", "bt709"])
    a.yuv_input, a.yuv_packed = dict(type="i420", matrix="bt709", range="limited", siting="center"), None
    assert demo._input(a, (8, 10)) == dict(type="i420", matrix="bt709", range="limited", siting="center", size=(8, 10))
    a.yuv_input = None
    assert demo._input(a, None) == dict(type="rgb8", size=None, layout="thwc")
