"""Host tests of the input stage for Y'CbCr at 8 to 16 bits, 4:2:0 / 4:2:2 / 4:4:4 (test_cfg.input type = an ops.YUV_PIXEL_FORMATS name,
DESIGN.md section 26): the format table and the coefficients, ops.yuv_planes' views, the key's parsing, the trackers' dtype refusals, the
torch contract against the numpy restatements (tests/yuvp_cases.py), the Y4M reader and writer, the C ABI's argument validation and the
kernels' code-object notes.  No GPU.  Every test here fails without the feature: the names do not exist."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import yuvp_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = PC.kernel_cases()


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


# ---- the table and the constants -------------------------------------------------------------------------------------------------------------
def test_format_table():
    from fgvc_amd import ops
    assert sorted(ops.YUV_PIXEL_FORMATS) == sorted(PC.FORMATS)
    for name, (layout, sx, sy, depth, shift, dt) in PC.FORMATS.items():
        want = (layout, sx, sy, depth, shift, torch.uint16 if dt is np.uint16 else torch.uint8)
        assert ops.YUV_PIXEL_FORMATS[name] == want, name
        assert depth + shift <= 8 * np.dtype(dt).itemsize
    assert ops.YUV_FORMATS == ("nv12", "i420") and not set(ops.YUV_FORMATS) & set(ops.YUV_PIXEL_FORMATS)
    assert [ops.YUV_PIXEL_FORMATS[n][4] for n in ("p010", "p012", "p016")] == [6, 4, 0]


def test_coefficients_of_the_depth():
    from fgvc_amd import ops
    for matrix in PC.MATRICES:
        for rng in PC.RANGES:
            six = ops.yuv_coefficients(matrix, rng)
            assert ops.yuv_coefficients_depth(matrix, rng, 8) == six[:2] + (128.0,) + six[2:]          # ==, not close
            assert ops.yuv_coefficients_depth(matrix, rng) == ops.yuv_coefficients_depth(matrix, rng, 8)
            for depth in range(8, 17):
                got = ops.yuv_coefficients_depth(matrix, rng, depth)
                assert all(isinstance(c, float) for c in got) and len(got) == 7
                assert np.allclose(got, PC.coefficients_f64(matrix, rng, depth), rtol=1e-15, atol=0)
                if rng == "limited":                                         # exact powers of two away from the 8-bit constants
                    s = float(1 << (depth - 8))
                    eight = ops.yuv_coefficients_depth(matrix, rng, 8)
                    assert got == (eight[0] * s, eight[1] / s, eight[2] * s) + tuple(c / s for c in eight[3:])
    lim, full = ops.yuv_coefficients_depth("bt601", "limited", 10), ops.yuv_coefficients_depth("bt709", "full", 16)
    assert lim[:3] == (64.0, 255.0 / 876.0, 512.0) and full[:3] == (0.0, 255.0 / 65535.0, 32768.0)
    for bad in (dict(matrix="bt2020"), dict(range="tv"), dict(depth=7), dict(depth=17)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ops.yuv_coefficients_depth(**bad)


# ---- ops.yuv_planes -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(PC.FORMATS))
def test_planes_are_views_of_the_packed_frames(fmt):
    from fgvc_amd import ops
    layout, sx, sy, _, _, dt = PC.FORMATS[fmt]
    T, h0, w0 = 3, 8, 12
    rows = h0 + 2 * h0 // (sx * sy)
    assert rows == ops.yuv_packed_rows(fmt, h0) and ops.yuv_packed_height(fmt, rows) == h0
    flat = np.arange(T * rows * w0).astype(dt)
    frames = torch.from_numpy(flat.reshape(T, rows, w0))
    y, u, v = ops.yuv_planes(frames, fmt)
    ch, cw = h0 // sy, w0 // sx
    assert tuple(y.shape) == (T, h0, w0) and tuple(u.shape) == tuple(v.shape) == (T, ch, cw)
    per = flat.reshape(T, -1)
    luma, rest = per[:, :h0 * w0], per[:, h0 * w0:]
    if layout == "planar":                                                   # by hand: the file's order
        want_u, want_v = rest[:, :ch * cw].reshape(T, ch, cw), rest[:, ch * cw:].reshape(T, ch, cw)
    else:
        want_u, want_v = rest[:, 0::2].reshape(T, ch, cw), rest[:, 1::2].reshape(T, ch, cw)
    assert np.array_equal(y.numpy(), luma.reshape(T, h0, w0)) and np.array_equal(u.numpy(), want_u) and np.array_equal(v.numpy(), want_v)
    for p in (y, u, v):                                                      # views: the storage is the frames'
        assert p.untyped_storage().data_ptr() == frames.untyped_storage().data_ptr()
    assert u.stride() == v.stride() and u.stride(2) == (2 if layout == "semi" else 1)
    # a time slice stays a view
    y2, u2, v2 = ops.yuv_planes(frames[::2], fmt)
    assert np.array_equal(u2.numpy(), want_u[::2]) and np.array_equal(v2.numpy(), want_v[::2]) and np.array_equal(y2.numpy(), y.numpy()[::2])
    assert ops.yuv_planes(frames[:0], fmt)[1].shape == (0, ch, cw)
    # refusals
    other = torch.uint8 if dt is np.uint16 else torch.uint16
    with pytest.raises(TypeError, match=fmt):
        ops.yuv_planes(torch.zeros(T, rows, w0, dtype=other), fmt)
    with pytest.raises(TypeError, match=fmt):
        ops.yuv_planes(torch.zeros(T, rows, w0), fmt)
    with pytest.raises(ValueError, match="packed"):
        ops.yuv_planes(frames[0], fmt)
    with pytest.raises(ValueError, match="packed"):
        ops.yuv_planes(frames[:, :rows - 1], fmt)                            # no whole h0
    if sx == 2:
        with pytest.raises(ValueError, match="w0 even"):
            ops.yuv_planes(frames[:, :, :w0 - 1], fmt)
    if layout == "planar" and sx == 2:
        wide = torch.from_numpy(np.zeros((T, rows, w0 + 4), dt))[:, :, :w0]
        with pytest.raises(ValueError, match="adjacent"):
            ops.yuv_planes(wide, fmt)
    with pytest.raises(ValueError, match="fmt"):
        ops.yuv_planes(frames, "nv12")


def test_planes_refuse_rows_that_are_no_whole_frame():
    """An odd luma height of a 4:2:0 frame has no whole number of packed rows (3 h0 / 2), and no rows are no frame."""
    from fgvc_amd import ops
    for fmt in ("p010", "yuv420p10"):
        for rows in (0, 1, 2, 4, 10):
            with pytest.raises(ValueError, match="h0 and w0 even"):
                ops.yuv_planes(torch.zeros(1, rows, 4, dtype=torch.uint16), fmt)
        assert ops.yuv_planes(torch.zeros(1, 9, 4, dtype=torch.uint16), fmt)[0].shape == (1, 6, 4)
    with pytest.raises(ValueError, match="w0 even"):
        ops.yuv_planes(torch.zeros(1, 7, 4, dtype=torch.uint16), "yuv422p10")
    with pytest.raises(ValueError, match="packed"):
        ops.yuv_planes(torch.zeros(1, 7, 4, dtype=torch.uint16), "yuv444p10")


def test_wrapper_refusals_without_a_gpu():
    from fgvc_amd import _lib, ops
    z = torch.zeros(1, 4, 4, dtype=torch.uint16)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.yuv_planes_to_lab(z, z[:, :2, :2], z[:, :2, :2], 10)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.yuv_planes_to_rgb8(z, z[:, :2, :2], z[:, :2, :2], 10)


# ---- the key ----------------------------------------------------------------------------------------------------------------------------------
def test_input_key_parsing():
    from fgvc_amd import engine
    assert engine.INPUT_TYPES[:3] == ("rgb8", "nv12", "i420") and set(PC.FORMATS) <= set(engine.INPUT_TYPES)
    for typ, (_, sx, _, _, _, dt) in PC.FORMATS.items():
        with pytest.raises(ValueError, match=f"type='{typ}' needs matrix="):         # no default matrix: the type alone stays refused
            engine.parse_input(dict(type=typ))
        with pytest.raises(ValueError, match="needs matrix="):
            engine.parse_input(dict(type=typ, range="full", size=(8, 8)))
        ic = engine.parse_input(dict(type=typ, matrix="bt601"))
        assert (ic.type, ic.size, ic.matrix, ic.range, ic.siting, ic.yuv) == (typ, None, "bt601", "limited", "left", True)
        assert engine.input_dtype(typ) == (torch.uint16 if dt is np.uint16 else torch.uint8)
        ic = engine.parse_input(dict(type=typ, size=[64, 48], matrix="bt709", range="full"))
        assert (ic.size, ic.matrix, ic.range) == ((64, 48), "bt709", "full")
        with pytest.raises(ValueError, match="layout"):
            engine.parse_input(dict(type=typ, matrix="bt709", layout="thwc"))
        with pytest.raises(ValueError, match="matrix"):
            engine.parse_input(dict(type=typ, matrix="bt2020"))
        with pytest.raises(ValueError, match="range"):
            engine.parse_input(dict(type=typ, matrix="bt709", range="pc"))
        with pytest.raises(ValueError, match="unknown key"):
            engine.parse_input(dict(type=typ, matrix="bt709", depth=10))
        if sx == 1:                                                          # 4:4:4: the key is refused by name, whatever its value
            for val in ("left", "center"):
                with pytest.raises(ValueError, match="siting"):
                    engine.parse_input(dict(type=typ, matrix="bt709", siting=val))
        else:
            assert engine.parse_input(dict(type=typ, matrix="bt709", siting="center")).siting == "center"
            with pytest.raises(ValueError, match="siting"):
                engine.parse_input(dict(type=typ, matrix="bt709", siting="top"))
    assert [engine.input_dtype(t) for t in ("rgb8", "nv12", "i420")] == [torch.uint8] * 3
    for typ in ("p210", "yuv420p16", "yuv440p", "yuva444p10", "v210", "yuv420p10be"):
        with pytest.raises(ValueError, match="type"):
            engine.parse_input(dict(type=typ))


@pytest.mark.parametrize("typ", ["VanillaTracker", "HRVanillaTracker"])
def test_trackers_refuse_frames_of_another_dtype(typ):
    """uint16 frames without the key, and frames whose dtype is not the configured type's, raise a TypeError that names both -- before
    anything touches the device; frames of the right dtype on the CPU meet the GPU-only rule."""
    pts = dict(query_points=torch.zeros(1, 1, 3), trajectories=torch.zeros(1, 3, 1, 2), visibilities=torch.zeros(1, 3, 1))
    meta, seg = [dict(original_shape=(16, 16))], torch.zeros(1, 16, 16, dtype=torch.uint8)
    p010 = torch.zeros(1, 3, 24, 16, dtype=torch.uint16)
    plain = _tracker(typ)
    with pytest.raises(TypeError, match="uint16.*test_cfg.input"):
        plain(test_mode=True, rgbs=p010, **pts)
    with pytest.raises(TypeError, match="uint16.*test_cfg.input"):
        plain(test_mode=True, imgs=p010[None], ref_seg_map=seg, img_meta=meta)
    m = _tracker(typ, input=dict(type="p010", matrix="bt709"))
    with pytest.raises(TypeError, match="uint8.*'p010'.*uint16"):
        m(test_mode=True, rgbs=p010.to(torch.uint8), **pts)
    with pytest.raises(TypeError, match="uint8.*'p010'.*uint16"):
        m(test_mode=True, imgs=p010.to(torch.uint8)[None], ref_seg_map=seg, img_meta=meta)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(test_mode=True, rgbs=p010, **pts)
    for key, kw in (("nv12", {}), ("rgb8", {}), ("yuv422p", dict(matrix="bt601"))):
        m = _tracker(typ, input=dict(type=key, **kw))
        with pytest.raises(TypeError, match=f"uint16.*'{key}'.*uint8"):
            m(test_mode=True, rgbs=p010, **pts)

    class OnDevice(torch.Tensor):                                            # a CPU tensor that claims to be on the GPU: the shape checks come first
        is_cuda = True

    m = _tracker(typ, input=dict(type="yuv422p10", matrix="bt709"))
    for bad in (torch.zeros(1, 3, 33, 16, dtype=torch.uint16), torch.zeros(1, 3, 32, 15, dtype=torch.uint16)):     # no whole h0; an odd width
        with pytest.raises(ValueError, match=r"uint16 yuv422p10 frames of shape \(1, T, 2 h0, w0\)"):
            m(test_mode=True, rgbs=bad.as_subclass(OnDevice), **pts)
    with pytest.raises(ValueError, match=r"\(1, 1, T, 2 h0, w0\)"):
        m(test_mode=True, imgs=torch.zeros(1, 1, 32, 16, dtype=torch.uint16).as_subclass(OnDevice), ref_seg_map=seg, img_meta=meta)


# ---- the torch contract against the restatements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_torch_bytes_equal_the_float32_restatement(name):
    from fgvc_amd.datasets import yuv_to_rgb8
    fmt, _, _, _, _, matrix, rng, siting = CASES[name]
    planes = PC.case_planes(CASES[name])
    got = yuv_to_rgb8(*PC.to_torch(planes, fmt), **PC.fmt_args(fmt), matrix=matrix, range=rng, siting=siting)
    want = PC.rgb8_f32(*planes, fmt, matrix, rng, siting)
    assert got.shape == want.shape and np.array_equal(got.numpy(), want), name


@pytest.mark.parametrize("fmt", list(PC.FORMATS))
def test_cpu_chain_within_rounding_of_the_float64_restatement(fmt):
    """datasets.preprocess_yuv_frames on the CPU against yuvp_cases.preprocess_f64, per format, at 17 x 22 the same size and resized both
    ways.  Bound: 8e-6, DESIGN.md section 14's figure for the f32 chain at such shapes (the decode adds four rounded operations on values
    below 2^9 to it: 4 x 2^-15 / 255 in the unit, below 1e-6 after the Lab slopes) -- plus, resized, F.interpolate's f32 source coordinate:
    w0 2^-23 pixels off at most, times a neighbour difference of the whole unit range and the Lab planes' slope of at most 10."""
    from fgvc_amd.datasets import preprocess_yuv_frames
    planes = PC.texture_planes(2, 17, 22, 3, fmt)
    t = PC.to_torch(planes, fmt)
    for size in (None, (9, 13), (31, 40)):
        for matrix, rng, siting in PC.SETTINGS[::3]:
            want = PC.preprocess_f64(*planes, fmt, size, matrix, rng, siting)
            got = preprocess_yuv_frames(*t, **PC.fmt_args(fmt), matrix=matrix, range=rng, siting=siting, size=size)
            assert got.dtype == torch.float32 and tuple(got.shape[1:]) == tuple(want.shape)
            e = float((got[0].double() - want).abs().max())
            bound = 8e-6 + (0 if size is None else 10 * 22 * 2.0 ** -23)
            print(f"[yuvp] {fmt} {size} {matrix} {rng} {siting}: E = {e:.3e}, bound = {bound:.3e}")
            assert e <= bound, (fmt, size, e)


def test_contract_masks_the_unused_bits_and_keeps_full_resolution_chroma():
    from fgvc_amd.datasets import yuv_chroma_at_luma, yuv_samples, yuv_to_rgb
    rs = np.random.RandomState(0)
    s = rs.randint(0, 1024, size=(1, 4, 6))
    for fmt in ("p010", "yuv420p10"):
        w = torch.from_numpy(PC.words(s, fmt, rs))
        assert np.array_equal(yuv_samples(w, 10, PC.FORMATS[fmt][4]).numpy(), s.astype(np.float32))
    c = torch.from_numpy(rs.randint(0, 65536, size=(2, 5, 7)).astype(np.float32))
    assert torch.equal(yuv_chroma_at_luma(c, 5, 7, (1, 1), "left"), c)                       # 4:4:4: the plane itself
    assert torch.equal(yuv_chroma_at_luma(c, 5, 7, (1, 1), "center"), c)
    half = yuv_chroma_at_luma(c, 5, 13, (2, 1), "left")                                      # 4:2:2: rows untouched, even columns co-sited
    assert torch.equal(half[:, :, ::2], c)
    y = torch.from_numpy(PC.words(s, "yuv444p10", rs))
    a = yuv_to_rgb(y, y, y, 10, 0, (1, 1), siting="left")
    assert torch.equal(a, yuv_to_rgb(y, y, y, 10, 0, (1, 1), siting="center"))
    with pytest.raises(ValueError, match="subsampling"):
        yuv_to_rgb(y, y, y, 10, 0, (4, 1))
    with pytest.raises(ValueError, match="depth"):
        yuv_samples(torch.zeros(2, dtype=torch.uint8), 10, 0)
    with pytest.raises(TypeError, match="uint16"):
        yuv_samples(torch.zeros(2), 10, 0)
    with pytest.raises(ValueError, match="chroma planes"):
        yuv_to_rgb(y, y[:, :2], y[:, :2], 10, 0, (2, 2))


def test_tie_cases_hold_exact_ties():
    """A guard on the cases: the searched (U, Y) codes put the float32 restatement's B exactly on a half inside (0, 255) for every kernel
    format -- pixels at which half-up rounding gives another byte than half-to-even."""
    f = np.float32
    for fmt in PC.KERNEL_FORMATS:
        planes, n = PC.tie_planes(fmt)
        assert n >= 2, (fmt, n)
        B = PC.rgb_f32(*planes, fmt, "bt601", "full")[..., 2]
        ties = (B > 0) & (B < 255) & (B % 1 == f(0.5))
        assert int(ties.sum()) >= n, (fmt, n, int(ties.sum()))


# ---- Y4M ------------------------------------------------------------------------------------------------------------------------------------------
def _y4m(path, header, frames=(b"",), frame_tag=b"FRAME\n"):
    with open(path, "wb") as fh:
        fh.write(header)
        for f in frames:
            fh.write(frame_tag + f)
    return str(path)


Y4M_TAGS = {"yuv422p": "C422", "yuv444p": "C444", "yuv420p10": "C420p10", "yuv420p12": "C420p12", "yuv422p10": "C422p10", "yuv422p12": "C422p12",
            "yuv444p10": "C444p10", "yuv444p12": "C444p12"}


@pytest.mark.parametrize("fmt", list(Y4M_TAGS))
def test_y4m_round_trip_per_tag(tmp_path, fmt):
    from fgvc_amd import ops
    from fgvc_amd.datasets import read_y4m_planes, write_y4m_planes
    _, _, _, depth, _, dt = PC.FORMATS[fmt]
    planes = PC.texture_planes(3, 16, 20, 2, fmt)                            # (garbage above the depth travels too: bit for bit)
    frames = PC.pack(*planes, fmt)
    p = str(tmp_path / "clip.y4m")
    write_y4m_planes(p, frames, fmt, fps=(25, 1), range="full")
    head = open(p, "rb").readline()
    assert head.startswith(b"YUV4MPEG2 W20 H16 F25:1 Ip") and Y4M_TAGS[fmt].encode() in head.split() and b"XCOLORRANGE=FULL" in head.split()
    assert os.path.getsize(p) == len(head) + 3 * (6 + frames[0].numel() * np.dtype(dt).itemsize)
    got, info = read_y4m_planes(p)
    assert got.dtype == frames.dtype and torch.equal(got.view(torch.uint8), frames.view(torch.uint8))
    assert info == dict(width=20, height=16, fps=(25, 1), siting="left", range="full", format=fmt, depth=depth)
    y, u, v = ops.yuv_planes(got, fmt)
    assert all(np.array_equal(a.numpy(), b) for a, b in zip((y, u, v), planes))
    if dt is np.uint16:                                                      # little-endian words in the file
        raw = open(p, "rb").read()[len(head) + 6:len(head) + 10]
        assert raw == bytes([int(planes[0][0, 0, 0]) & 255, int(planes[0][0, 0, 0]) >> 8, int(planes[0][0, 0, 1]) & 255, int(planes[0][0, 0, 1]) >> 8])
    assert torch.equal(read_y4m_planes(p, max_frames=2)[0], frames[:2])
    assert read_y4m_planes(p, max_frames=0)[0].shape == (0, frames.shape[1], 20)
    write_y4m_planes(p, frames.numpy(), fmt)                                 # an array; the defaults
    assert read_y4m_planes(p)[1] == dict(width=20, height=16, fps=(30, 1), siting="left", range="limited", format=fmt, depth=depth)
    with pytest.raises(TypeError, match=fmt):
        write_y4m_planes(p, frames.to(torch.float32), fmt)
    with pytest.raises(ValueError, match="packed"):
        write_y4m_planes(p, frames[:, :-1], fmt)


def test_y4m_planes_read_what_read_y4m_reads(tmp_path):
    """8-bit 4:2:0 files through the new reader: read_y4m's frames and keys, format 'i420'; and hand-written headers."""
    from fgvc_amd.datasets import read_y4m, read_y4m_header, read_y4m_planes, write_y4m, write_y4m_planes
    frames = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(2, 24, 20)).astype(np.uint8))
    for siting, tag in (("left", "420mpeg2"), ("center", "420jpeg")):
        p = str(tmp_path / f"{siting}.y4m")
        write_y4m_planes(p, frames, "i420", fps=(24, 1), siting=siting)
        assert open(p, "rb").read() == (write_y4m(p + "2", frames, fps=(24, 1), siting=siting), open(p + "2", "rb").read())[1]
        assert read_y4m_header(p) == tag
        got, info = read_y4m_planes(p)
        old, old_info = read_y4m(p)
        assert torch.equal(got, old) and info == dict(old_info, format="i420", depth=8)
    body = bytes(range(24))                                                  # 4 x 4 8-bit 4:2:0
    g, info = read_y4m_planes(_y4m(tmp_path / "bare.y4m", b"YUV4MPEG2 W4 H4 F30000:1001\n", [body, body], b"FRAME Ip\n"))
    assert info == dict(width=4, height=4, fps=(30000, 1001), siting="center", range="limited", format="i420", depth=8) and g.shape == (2, 6, 4)
    assert read_y4m_header(tmp_path / "bare.y4m") == "420jpeg"
    # C422p10 by hand: 4 x 2 luma, 2 x 2 chroma planes, little-endian words 0x0301 ..
    words = np.arange(16, dtype="<u2") + 0x0300
    g, info = read_y4m_planes(_y4m(tmp_path / "h.y4m", b"YUV4MPEG2 W4 H2 F25:1 Ip A1:1 C422p10 XCOLORRANGE=LIMITED\n", [words.tobytes()]))
    assert info["format"] == "yuv422p10" and info["depth"] == 10 and g.dtype == torch.uint16 and g.shape == (1, 4, 4)
    assert g.reshape(-1).tolist() == list(range(0x0300, 0x0310))
    g, info = read_y4m_planes(_y4m(tmp_path / "h444.y4m", b"YUV4MPEG2 W3 H1 F25:1 Ip C444\n", [bytes(range(9))]))       # odd sides: no subsampled axis
    assert info["format"] == "yuv444p" and g.shape == (1, 3, 3) and g.reshape(-1).tolist() == list(range(9))
    g, info = read_y4m_planes(_y4m(tmp_path / "h422.y4m", b"YUV4MPEG2 W2 H3 F25:1 Ip C422\n", [bytes(range(12))]))     # an odd height is fine for 4:2:2
    assert info["format"] == "yuv422p" and g.shape == (1, 6, 2)
    with pytest.raises(ValueError, match="nv16"):                            # Y4M holds planar frames
        write_y4m_planes(str(tmp_path / "x.y4m"), torch.zeros(1, 8, 4, dtype=torch.uint8), "nv16")
    with pytest.raises(ValueError, match="p010"):
        write_y4m_planes(str(tmp_path / "x.y4m"), torch.zeros(1, 6, 4, dtype=torch.uint16), "p010")
    with pytest.raises(ValueError, match="siting"):
        write_y4m_planes(str(tmp_path / "x.y4m"), torch.zeros(1, 6, 4, dtype=torch.uint8), "i420", siting="top")


def test_y4m_planes_refusals(tmp_path):
    from fgvc_amd.datasets import read_y4m_planes
    body = bytes(48)
    for tag in ("Cmono", "Cmono16", "C411", "C444alpha", "C420paldv", "C420p16", "C440"):
        with pytest.raises(ValueError, match=tag + " is not supported"):
            read_y4m_planes(_y4m(tmp_path / "c.y4m", f"YUV4MPEG2 W4 H4 F25:1 Ip {tag}\n".encode(), [body]))
    for tag in ("It", "Ib", "Im"):
        with pytest.raises(ValueError, match=tag):
            read_y4m_planes(_y4m(tmp_path / "i.y4m", f"YUV4MPEG2 W4 H4 F25:1 {tag} C422p10\n".encode(), [body]))
    for size, tag in (("W5 H4", "C420p10"), ("W4 H3", "C420p10"), ("W5 H4", "C422"), ("W5 H3", "C422p12"), ("W4 H3", "C420mpeg2")):
        with pytest.raises(ValueError, match="odd size"):
            read_y4m_planes(_y4m(tmp_path / "o.y4m", f"YUV4MPEG2 {size} F25:1 Ip {tag}\n".encode(), [bytes(120)]))
    with pytest.raises(ValueError, match="truncated"):
        read_y4m_planes(_y4m(tmp_path / "t.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip C420p10\n", [body, body[:47]]))
    with pytest.raises(ValueError, match="truncated"):                       # 8-bit 4:4:4 is 48 bytes, 10-bit 96
        read_y4m_planes(_y4m(tmp_path / "t2.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip C444p10\n", [body]))
    with pytest.raises(ValueError, match="YUV4MPEG2"):
        read_y4m_planes(_y4m(tmp_path / "n.y4m", b"RIFF W4 H4\n", [body]))
    with pytest.raises(ValueError, match="FRAME"):
        read_y4m_planes(_y4m(tmp_path / "f.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip C444\n", [body], b"FRANE\n"))
    with pytest.raises(ValueError, match="XCOLORRANGE"):
        read_y4m_planes(_y4m(tmp_path / "r.y4m", b"YUV4MPEG2 W4 H4 F25:1 Ip C444 XCOLORRANGE=TV\n", [body]))
    with pytest.raises(ValueError, match="size"):
        read_y4m_planes(_y4m(tmp_path / "s.y4m", b"YUV4MPEG2 F25:1 Ip C444\n", [body]))


# ---- the library --------------------------------------------------------------------------------------------------------------------------------
def test_yuvp_symbols_declared_and_validate_their_arguments():
    """Both entry points are exported and listed in _lib.SIGNATURES, input_yuv.hip (the one YUV input file) is a build source, and every
    bad argument of the header's list returns FGVC_ERR_INVALID_ARG with a message that names the entry point, before any launch (no GPU
    here: a launch would fail with another code)."""
    from fgvc_amd import _lib, build
    assert "input_yuv.hip" in build.SOURCES
    lib = _lib.load()
    p = C.c_void_p(4096)                     # never dereferenced: every call below is refused on the host
    coef = (64.0, 0.29, 512.0, 0.4, -0.1, -0.2, 0.5)
    ok = dict(y=p, u=p, v=p, out=p, sb=2, depth=10, shift=6, sx=2, sy=2, T=1, h0=4, w0=4, h=4, w=4, pl=0, pr=0, pt=0, pb=0, siting=0)

    def lab(**kw):
        a = dict(ok, **kw)
        return lib.fgvc_frames_yuvp_to_lab_f32(a["y"], a["u"], a["v"], a["sb"], a["depth"], a["shift"], a["sx"], a["sy"], a["T"], a["h0"], a["w0"],
                                               16, 4, 8, 4, 2, *coef, a["siting"], a["h"], a["w"], a["pl"], a["pr"], a["pt"], a["pb"], a["out"], None)

    def rgb(**kw):
        a = dict(ok, **kw)
        return lib.fgvc_frames_yuvp_to_rgb8(a["y"], a["u"], a["v"], a["sb"], a["depth"], a["shift"], a["sx"], a["sy"], a["T"], a["h0"], a["w0"],
                                            16, 4, 8, 4, 2, *coef, a["siting"], a["out"], None)

    for name, fn, sizes in (("fgvc_frames_yuvp_to_lab_f32", lab, ("T", "h0", "w0", "h", "w")), ("fgvc_frames_yuvp_to_rgb8", rgb, ("T", "h0", "w0"))):
        assert name in _lib.SIGNATURES and hasattr(lib, name)

        def refused(what, **kw):
            assert fn(**kw) == _lib.ERR_INVALID_ARG, (name, kw)
            assert lib.fgvc_last_error().startswith(name.encode() + b": " + what), (name, kw, lib.fgvc_last_error())
        for ptr in ("y", "u", "v", "out"):
            refused(b"null pointer", **{ptr: None})
        for k in sizes:
            for val in (0, -3):
                refused(b"non-positive size", **{k: val})
        for sb in (0, 3, 4, -1):
            refused(b"sample_bytes", sb=sb)
        for depth, shift, sb in ((7, 0, 1), (17, 0, 2), (9, 0, 1), (8, 1, 1), (10, 7, 2), (16, 1, 2), (10, -1, 2), (12, 0, 1)):
            refused(b"depth", depth=depth, shift=shift, sb=sb)
        for sx, sy in ((0, 2), (3, 2), (2, 0), (2, 4), (-1, 1)):
            refused(b"sub_x", sx=sx, sy=sy)
        for s in (-1, 2):
            refused(b"siting", siting=s)
        refused(b"alignment", u=C.c_void_p(4097))
        refused(b"shape beyond the launch grid", T=65536)
        assert fn(h0=1 << 18, h=1 << 18) == _lib.ERR_INVALID_ARG and b"launch grid" in lib.fgvc_last_error()
    for k in ("pl", "pr", "pt", "pb"):
        assert lab(**{k: -1}) == _lib.ERR_INVALID_ARG, k
        assert lib.fgvc_last_error().startswith(b"fgvc_frames_yuvp_to_lab_f32: negative pad")


def test_yuvp_kernels_use_no_scratch():
    """The six run-time-format kernels (Yuvp -- Lab: resize and same size, bytes; each for 8- and 16-bit words) in the code-object notes of
    the built library: no scratch memory, no spilled register, no LDS."""
    notes = _tool("kernel_notes").kernel_notes()
    lab = {k: v for k, v in notes.items() if "frames_yuv_to_lab_kernel" in k and "Yuvp" in k}
    rgb = {k: v for k, v in notes.items() if "frames_yuv_to_rgb8_kernel" in k and "Yuvp" in k}
    assert len(lab) == 4 and len(rgb) == 2, (sorted(lab), sorted(rgb))
    for k, v in {**lab, **rgb}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 0, (k, v)
        print(f"[yuvp] {k}: {v.get('vgpr_count')} VGPRs")


# ---- the demo -----------------------------------------------------------------------------------------------------------------------------------
def test_demo_tells_the_files_apart(tmp_path):
    from fgvc_amd.datasets import read_y4m_header, write_y4m_planes, _Y4M_SITING
    demo = _tool("demo")
    assert callable(demo.load_y4m_planes)
    p = str(tmp_path / "a.y4m")
    write_y4m_planes(p, PC.pack(*PC.texture_planes(2, 16, 20, 3, "yuv422p10"), "yuv422p10"), "yuv422p10")
    assert demo.is_y4m(p) and read_y4m_header(p) == "422p10" and read_y4m_header(p) not in _Y4M_SITING
    write_y4m_planes(p, torch.zeros(2, 24, 20, dtype=torch.uint8), "i420")
    assert read_y4m_header(p) in _Y4M_SITING                                 # 8-bit 4:2:0 stays with load_y4m
