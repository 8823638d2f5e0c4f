"""GPU: the YUV 4:2:0 output stage (fgvc_frames_rgb8_to_yuv420, ops.rgb_frames_to_yuv420, viz.frames_to_yuv420(backend='hip'), tools/demo.py
--out-video).

No tolerance anywhere: the kernel's bytes equal datasets.rgb8_to_yuv420's (the host restatement, computed once per case on the CPU and held to
the numpy float32 chain and to float64 by tests/test_yuv_out_host.py) with `==` -- every size, matrix, range and siting, the exact ties of
full-range colours included -- through every input form (packed, planar, a time slice, a crop at an odd column) and output form (packed I420
and NV12, separate planes with wide rows, odd sizes); every output sits between sentinel bytes that must survive the launch."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import yuv_out_cases as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = OC.frame_sets()
CASES = OC.cases()
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def restated():
    """(frames, matrix, range, siting) by key -> datasets.rgb8_to_yuv420 on the CPU, computed once and never written to."""
    from fgvc_amd import datasets
    memo = {}

    def get(key, frames, m, r, s):
        k = (key, m, r, s)
        if k not in memo:
            memo[k] = datasets.rgb8_to_yuv420(frames, m, r, s)
        return memo[k]

    return get


class Guarded:
    """T planes of h x w bytes inside a larger buffer of sentinels: `lead` bytes in front, `gap` after every row, 5 more after every frame."""

    def __init__(self, dev, T, h, w, lead=256, gap=3, pixel=1):
        self.shape, self.lead = (T, h, w), lead
        row = (w - 1) * pixel + 1 + gap
        self.strides = (h * row + 5, row, pixel)
        self.buf = torch.full((lead + T * self.strides[0] + 64,), SENTINEL, dtype=torch.uint8, device=dev)

    def view(self, buf=None, offset=0):
        return (self.buf if buf is None else buf).as_strided(self.shape, self.strides, self.lead + offset)

    def intact(self, *offsets):
        """every byte outside the planes (at `offsets`, default the one at 0) still holds the sentinel"""
        rest = self.buf.clone()
        for o in offsets or (0,):
            self.view(rest, o).fill_(SENTINEL)
        return bool((rest == SENTINEL).all())


def _same(got, want):
    return all(torch.equal(g.cpu(), w) for g, w in zip(got, want))


def _encode_into_guarded(dev, frames_dev, shape, m, r, s, layout="thwc", lead=256, gap=3):
    from fgvc_amd import ops
    T, h, w = shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    gy, gu, gv = Guarded(dev, T, h, w, lead, gap), Guarded(dev, T, ch, cw, lead, gap), Guarded(dev, T, ch, cw, lead, gap)
    planes = (gy.view(), gu.view(), gv.view())
    got = ops.rgb_frames_to_yuv420(frames_dev, layout=layout, matrix=m, range=r, siting=s, planes=planes)
    assert all(a is b for a, b in zip(got, planes))
    assert gy.intact() and gu.intact() and gv.intact(), "bytes outside the planes were written"
    return got


def test_tile_extents(dev):
    from fgvc_amd import _lib, ops
    lib = _lib.load()
    assert (lib.fgvc_yuv_out_tile_rows(), lib.fgvc_yuv_out_tile_cols()) == ops.YUV_OUT_TILE


# ---- the kernel == the restatement -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_kernel_equals_the_restatement(dev, restated, cid):
    """Every frame set (T in {1, 3}; 1 x 1 up to 65 x 131, odd sizes included; the saturated colours and the exact luma ties) in every
    setting, written into strided planes between sentinels; the even sizes also as packed I420 and NV12."""
    from fgvc_amd import datasets, ops
    name, m, r, s = CASES[cid]
    frames = SETS[name]
    T, h, w, _ = frames.shape
    want = restated(name, frames, m, r, s)
    got = _encode_into_guarded(dev, frames.to(dev), (T, h, w), m, r, s)
    for g, x, plane in zip(got, want, "yuv"):
        assert torch.equal(g.cpu(), x), (cid, plane, int((g.cpu() != x).sum()))
    if h % 2 == 0 and w % 2 == 0:
        for fmt in OC.FORMATS:
            packed = ops.rgb_frames_to_yuv420(frames.to(dev), fmt, matrix=m, range=r, siting=s)
            assert packed.dtype == torch.uint8 and packed.shape == (T, 3 * h // 2, w)
            assert torch.equal(packed.cpu(), datasets.pack_yuv420(*want, fmt)), (cid, fmt)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("m,r,s", OC.COMBOS, ids=["-".join(c) for c in OC.COMBOS])
def test_one_past_the_tile(dev, restated, T, m, r, s):
    """One row and one column past what a workgroup owns: a second workgroup both ways whose lanes hold one pixel, one chroma sample."""
    from fgvc_amd import _lib
    lib = _lib.load()
    h, w = lib.fgvc_yuv_out_tile_rows() + 1, lib.fgvc_yuv_out_tile_cols() + 1
    frames = OC.texture(T, h, w, 40 + T)
    want = restated(f"tile{T}", frames, m, r, s)
    got = _encode_into_guarded(dev, frames.to(dev), (T, h, w), m, r, s)
    assert _same(got, want)
    even = frames[:, :h - 1, :w - 1]                                          # the tile itself, a view: rows of 3 (w - 1) bytes in rows of 3 w
    want = restated(f"tile{T}-even", even, m, r, s)
    assert _same(_encode_into_guarded(dev, frames.to(dev)[:, :h - 1, :w - 1], (T, h - 1, w - 1), m, r, s), want)


def test_no_frames(dev):
    from fgvc_amd import ops
    empty = torch.empty(0, 6, 10, 3, dtype=torch.uint8, device=dev)
    for fmt in OC.FORMATS:
        assert ops.rgb_frames_to_yuv420(empty, fmt).shape == (0, 9, 10)
    y, u, v = _encode_into_guarded(dev, torch.empty(0, 3, 5, 3, dtype=torch.uint8, device=dev), (0, 3, 5), "bt601", "limited", "left")
    assert y.shape == (0, 3, 5) and u.shape == (0, 2, 3) and v.shape == (0, 2, 3)


# ---- input forms -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", OC.SITINGS)
def test_input_forms_are_read_in_place(dev, restated, s):
    """'tchw' (planar: the dword path per channel where aligned), a [::2] time slice, crops at every byte alignment of the first column -- the
    odd ones take the byte path -- and an odd-sized crop: the same bytes as the contiguous copy gives."""
    from fgvc_amd import ops
    big = OC.texture(5, 40, 72, 50)
    on_dev = big.to(dev)
    kw = dict(matrix="bt709", range="full", siting=s)
    for x0 in (0, 1, 2, 3, 4, 5):
        for hh, ww in ((34, 64), (33, 61)):
            crop = big[:, 3:3 + hh, x0:x0 + ww]
            want = restated(f"crop{x0}-{hh}x{ww}", crop.contiguous(), "bt709", "full", s)
            view = on_dev[:, 3:3 + hh, x0:x0 + ww]
            assert not view.is_contiguous()
            assert _same(_encode_into_guarded(dev, view, (5, hh, ww), "bt709", "full", s), want), (x0, hh, ww)
            planar = on_dev.permute(0, 3, 1, 2).contiguous()[:, :, 3:3 + hh, x0:x0 + ww]                 # (T, 3, hh, ww), a view
            assert _same(_encode_into_guarded(dev, planar, (5, hh, ww), "bt709", "full", s, layout="tchw"), want), (x0, hh, ww)
    want = restated("slice", big[::2].contiguous(), "bt709", "full", s)
    assert _same(_encode_into_guarded(dev, on_dev[::2], (3, 40, 72), "bt709", "full", s), want)
    assert torch.equal(ops.rgb_frames_to_yuv420(on_dev.permute(0, 3, 1, 2)[::2], "nv12", layout="tchw", **kw).cpu(),
                       ops.rgb_frames_to_yuv420(on_dev[::2].contiguous(), "nv12", **kw).cpu())


# ---- output forms ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", OC.FORMATS)
@pytest.mark.parametrize("shape", [(3, 34, 66), (1, 6, 10), (3, 2, 2), (2, 18, 1030)], ids=lambda s: "x".join(map(str, s)))
def test_packed_output_between_guard_bands(dev, restated, fmt, shape):
    """`out=` in the middle of a buffer of sentinels, at every byte alignment: the words of the luma rows and of I420's planes or NV12's pairs
    fall on aligned and unaligned addresses; (2, 18, 1030): three workgroups along a row."""
    from fgvc_amd import datasets, ops
    T, h, w = shape
    frames = OC.texture(T, h, w, 60)
    for s in OC.SITINGS:
        want = datasets.pack_yuv420(*restated(f"packed-{shape}", frames, "bt601", "limited", s), fmt)
        n = want.numel()
        for lead in (256, 257, 258, 259):
            buf = torch.full((lead + n + 61,), SENTINEL, dtype=torch.uint8, device=dev)
            out = buf[lead:lead + n].view(T, 3 * h // 2, w)
            assert ops.rgb_frames_to_yuv420(frames.to(dev), fmt, siting=s, out=out) is out
            assert torch.equal(out.cpu(), want), (s, lead)
            assert bool((buf[:lead] == SENTINEL).all()) and bool((buf[lead + n:] == SENTINEL).all()), (s, lead)


@pytest.mark.parametrize("shape", [(2, 34, 66), (2, 33, 61), (1, 9, 513)], ids=lambda s: "x".join(map(str, s)))
def test_interleaved_and_swapped_planes(dev, restated, shape):
    """NV12's pairs as planes= views of one (T, ch, cw, 2) region with sentinels in its row gaps, odd sizes included; NV21 (the same region with
    u and v swapped: the pairs in the other order); YV12 is planes=(y, v, u) of separate planes."""
    from fgvc_amd import ops
    T, h, w = shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    frames = OC.texture(T, h, w, 61)
    for s in OC.SITINGS:
        y, u, v = restated(f"pairs-{shape}", frames, "bt709", "limited", s)
        for lead in (256, 257, 258):
            for swapped in (False, True):
                gy, gc = Guarded(dev, T, h, w, lead), Guarded(dev, T, ch, cw, lead, gap=4, pixel=2)
                first, second = gc.view(), gc.view(offset=1)
                planes = (gy.view(), second, first) if swapped else (gy.view(), first, second)
                ops.rgb_frames_to_yuv420(frames.to(dev), matrix="bt709", siting=s, planes=planes)
                assert _same(planes, (y, u, v)), (s, lead, swapped)
                assert gy.intact() and gc.intact(0, 1), (s, lead, swapped)
        gy, gu, gv = (Guarded(dev, T, *hw) for hw in ((h, w), (ch, cw), (ch, cw)))
        ops.rgb_frames_to_yuv420(frames.to(dev), matrix="bt709", siting=s, planes=(gy.view(), gv.view(), gu.view()))
        assert _same((gy.view(), gu.view(), gv.view()), (y, v, u)) and gu.intact() and gv.intact()


def test_planes_of_a_packed_buffer_and_a_second_stream(dev, restated):
    from fgvc_amd import datasets, ops
    frames = OC.texture(3, 34, 66, 62)
    on_dev = frames.to(dev)
    want = restated("views", frames, "bt601", "full", "center")
    kw = dict(matrix="bt601", range="full", siting="center")
    for fmt in OC.FORMATS:
        packed = torch.full((3, 51, 66), SENTINEL, dtype=torch.uint8, device=dev)
        ops.rgb_frames_to_yuv420(on_dev, planes=ops.yuv420_planes(packed, fmt), **kw)
        assert torch.equal(packed.cpu(), datasets.pack_yuv420(*want, fmt)), fmt
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        again = ops.rgb_frames_to_yuv420(on_dev, "i420", **kw)
    s.synchronize()
    assert torch.equal(again.cpu(), datasets.pack_yuv420(*want, "i420"))


# ---- viz and the demo ------------------------------------------------------------------------------------------------------------------------------
def test_viz_hip_backend_equals_host(dev):
    from fgvc_amd import viz
    frames = OC.texture(3, 34, 66, 63)
    for fmt in OC.FORMATS:
        for m, r, s in OC.COMBOS:
            want = viz.frames_to_yuv420(frames.numpy(), fmt, m, r, s, backend="host")
            got = viz.frames_to_yuv420(frames.numpy(), fmt, m, r, s, backend="hip")
            assert isinstance(got, np.ndarray) and np.array_equal(got, want), (fmt, m, r, s)
            on_dev = viz.frames_to_yuv420(frames.to(dev), fmt, m, r, s, backend="hip")
            assert on_dev.is_cuda and np.array_equal(on_dev.cpu().numpy(), want), (fmt, m, r, s)
    with pytest.raises(ValueError, match="odd"):
        viz.frames_to_yuv420(OC.texture(1, 3, 5, 6).to(dev), backend="hip")


def _demo():
    spec = importlib.util.spec_from_file_location("fgvc_demo_out", os.path.join(ROOT, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    return demo


def test_demo_writes_a_y4m_video(dev, tmp_path):
    """A 3-frame 16 x 24 Y4M clip (full range, 'center' siting, 25 fps) through tools/demo.py's own functions: the written file reads back with
    read_y4m, carries the clip's tags, and its frames are the host encoding of the rendered frames with the settings the clip was decoded with."""
    from fgvc_amd import datasets, viz
    demo = _demo()
    clip = str(tmp_path / "clip.y4m")
    source = datasets.pack_yuv420(*datasets.rgb8_to_yuv420(OC.texture(3, 16, 24, 64), "bt601", "full", "center"), "i420")
    datasets.write_y4m(clip, source, fps=(25, 1), siting="center", range="full")
    video = str(tmp_path / "out.y4m")
    r = demo.main([clip, "--task", "points", "--query-points", "0", "8", "6", "1", "15", "10", "--out", str(tmp_path / "o"), "--radius", "2",
                   "--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--precede-frames", "2", "--batch-step", "2", "--out-video", video])
    assert r["video_settings"] == dict(matrix="bt601", range="full", siting="center", fps=(25, 1))            # 16 rows: bt601, the clip's tags
    assert (r["rendered"] != r["frames"]).any()
    back, info = datasets.read_y4m(video)
    assert info == dict(width=24, height=16, fps=(25, 1), siting="center", range="full")
    want = viz.frames_to_yuv420(r["rendered"], "i420", "bt601", "full", "center", backend="host")
    assert np.array_equal(back.numpy(), want) and np.array_equal(r["video"], want)
    # the host encoder writes the same file; another matrix and range by the options
    a = demo.parse_args([clip, "--task", "points", "--query-points", "0", "8", "6", "--out", "o", "--out-video", video, "--out-matrix", "bt709",
                         "--out-range", "limited"])
    a.yuv_info = dict(info, matrix="bt601")
    settings = demo.video_settings(a, 16)
    assert settings == dict(matrix="bt709", range="limited", siting="center", fps=(25, 1))
    for host in (True, False):
        path = str(tmp_path / f"again_{host}.y4m")
        packed = demo.write_video(path, torch.from_numpy(r["rendered"]).to(dev), settings, dev, host=host)
        want = viz.frames_to_yuv420(r["rendered"], "i420", "bt709", "limited", "center", backend="host")
        assert np.array_equal(packed.numpy(), want) and np.array_equal(datasets.read_y4m(path)[0].numpy(), want)
        assert datasets.read_y4m(path)[1]["range"] == "limited"
    # no .y4m input: the defaults; an odd side: refused before anything runs
    a = demo.parse_args(["--synthetic", "3", "16", "24", "--task", "flow", "--out", "o", "--out-video", video, "--fps", "12.5"])
    assert demo.video_settings(a, 16) == dict(matrix="bt601", range="limited", siting="left", fps=(25, 2))
    assert demo.video_settings(a, 720)["matrix"] == "bt709"
    with pytest.raises(ValueError, match="odd"):
        demo.main(["--synthetic", "3", "15", "24", "--task", "flow", "--out", str(tmp_path / "odd"), "--out-video", video])
    with pytest.raises(SystemExit):
        demo.parse_args([clip, "--task", "flow", "--out", "o", "--out-matrix", "bt709"])


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_refusals(dev):
    from fgvc_amd import _lib, ops
    f = OC.texture(2, 6, 10, 1).to(dev)
    y, u, v = (torch.empty(s, dtype=torch.uint8, device=dev) for s in ((2, 6, 10), (2, 3, 5), (2, 3, 5)))
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.rgb_frames_to_yuv420(f.cpu())
    with pytest.raises(TypeError, match="uint8"):
        ops.rgb_frames_to_yuv420(f.float())
    with pytest.raises(ValueError, match="4 dimensions"):
        ops.rgb_frames_to_yuv420(f[0])
    with pytest.raises(ValueError, match="3 channels"):
        ops.rgb_frames_to_yuv420(f, layout="tchw")
    with pytest.raises(ValueError, match="3 channels"):
        ops.rgb_frames_to_yuv420(f[..., :2])
    for bad in (dict(matrix="bt2020"), dict(range="tv"), dict(siting="top"), dict(fmt="yv12"), dict(layout="hwc")):
        with pytest.raises(ValueError, match=list(bad)[0]):
            ops.rgb_frames_to_yuv420(f, **bad)
    with pytest.raises(ValueError, match="planes="):
        ops.rgb_frames_to_yuv420(f[:, :5])
    with pytest.raises(ValueError, match="planes="):
        ops.rgb_frames_to_yuv420(f[:, :, :9], "nv12")
    with pytest.raises(ValueError, match="out"):
        ops.rgb_frames_to_yuv420(f, out=torch.empty(2, 9, 11, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="out"):
        ops.rgb_frames_to_yuv420(f, out=torch.empty(2, 9, 10, device=dev))
    with pytest.raises(ValueError, match="out"):
        ops.rgb_frames_to_yuv420(f, out=torch.empty(2, 9, 20, dtype=torch.uint8, device=dev)[:, :, ::2])
    with pytest.raises(ValueError, match="out"):
        ops.rgb_frames_to_yuv420(f, out=torch.empty(2, 9, 10, dtype=torch.uint8, device=dev), planes=(y, u, v))
    with pytest.raises(ValueError, match="planes"):
        ops.rgb_frames_to_yuv420(f, planes=(y, u))
    with pytest.raises(ValueError, match="planes: u"):
        ops.rgb_frames_to_yuv420(f, planes=(y, u[:, :2], v))
    with pytest.raises(ValueError, match="planes: y"):
        ops.rgb_frames_to_yuv420(f, planes=(y[:1], u, v))
    with pytest.raises(TypeError, match="uint8"):
        ops.rgb_frames_to_yuv420(f, planes=(y, u, v.float()))
    with pytest.raises(ValueError, match="planes: v on"):
        ops.rgb_frames_to_yuv420(f, planes=(y, u, v.cpu()))
    with pytest.raises(ValueError, match="same strides"):
        ops.rgb_frames_to_yuv420(f, planes=(y, u, torch.empty(2, 3, 5, 2, dtype=torch.uint8, device=dev)[..., 0]))
    with pytest.raises(ValueError, match="adjacent"):
        ops.rgb_frames_to_yuv420(f, planes=(torch.empty(2, 6, 20, dtype=torch.uint8, device=dev)[:, :, ::2], u, v))


def test_entry_point_refusals(dev):
    """The C entry point's own checks, before any launch: overlapping output rows, a siting it does not know, a null pointer, T < 0."""
    from fgvc_amd import _lib, ops
    f = OC.texture(2, 6, 10, 1).to(dev)
    y, u, v = (torch.empty(s, dtype=torch.uint8, device=dev) for s in ((2, 6, 10), (2, 3, 5), (2, 3, 5)))
    coef = ops.rgb_to_yuv_coefficients()

    def call(T=2, ys=(60, 10), cs=(15, 5, 1), siting=0, yp=y.data_ptr()):
        _lib.call("fgvc_frames_rgb8_to_yuv420", f.data_ptr(), T, 6, 10, *f.stride(), yp, *ys, u.data_ptr(), v.data_ptr(), *cs, *coef, siting, None)
    call()
    torch.cuda.synchronize()
    for bad, what in ((dict(ys=(60, 9)), "luma"), (dict(ys=(59, 10)), "luma"), (dict(cs=(15, 4, 1)), "chroma"), (dict(cs=(14, 5, 1)), "chroma"),
                      (dict(cs=(15, 5, 0)), "chroma"), (dict(cs=(30, 5, 2)), "chroma"), (dict(siting=2), "siting"), (dict(T=-1), "T=-1"),
                      (dict(yp=None), "null")):
        with pytest.raises(_lib.FgvcHipError, match=what):
            call(**bad)
    call(T=0, yp=None)                                                        # nothing to write: no launch, no complaint
