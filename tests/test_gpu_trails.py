"""GPU tests of the trail renderer (fgvc_render_trails_u8): ops.render_trails and viz's backend='hip' against viz's host
backend on every case of tests/trails_cases.py (itself held to a plain restatement in tests/test_trails_host.py) with torch.equal -- float64
without contraction, no square root, one correctly rounded division: there is no tolerance -- and tools/demo.py --trails in-process."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import trails_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(TC.cases())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _want(name):
    return torch.from_numpy(TC.expected(name).copy())                 # (the shared array is read-only)


def _on(dev, c):
    """A case as ops.render_trails takes it: (frames, keyword arguments), everything on the device."""
    from fgvc_amd import viz

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    frames = up(c["frames"])
    kw = dict(tracks=up(c["tracks"]), trail=c["trail"], linewidth=c.get("linewidth", 2.0), dots=c.get("dots", True), radius=c.get("radius"))
    for k in ("visibles", "colors", "ids"):
        if c.get(k) is not None:
            kw[k] = up(c[k])
    if c.get("trail_fade") is not None:
        kw["fade"] = up(c["trail_fade"])
    if c.get("trail_color_by", "track") == "time":
        kw["time_colors"] = up(viz.spring_colors(frames.shape[0]))
    return frames, kw


def _report(name, got, want):
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist()) if len(bad) else ()
    return f"{name}: {bad.shape[0]} bytes differ; first (t, y, x, c) {bad[:6].tolist()}: got {got[first] if first else ''}, want {want[first] if first else ''}"


@pytest.mark.parametrize("name", NAMES)
def test_render_trails_equals_the_host_backend(dev, name):
    from fgvc_amd import ops
    frames, kw = _on(dev, TC.cases()[name])
    before = frames.clone()
    got = ops.render_trails(frames, **kw)
    assert got.dtype == torch.uint8 and got.shape == frames.shape and got.data_ptr() != frames.data_ptr()
    assert torch.equal(got.cpu(), _want(name)), _report(name, got.cpu(), _want(name))
    assert torch.equal(frames, before)


@pytest.mark.parametrize("name", NAMES)
def test_viz_hip_backend_equals_the_host_backend(dev, name):
    c = TC.cases()[name]
    got = TC.render(c, backend="hip")                                                     # numpy in, numpy out
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    assert np.array_equal(got, TC.expected(name)), _report(name, torch.from_numpy(got), _want(name))


def test_cuda_tensor_in_cuda_tensor_out(dev):
    from fgvc_amd import viz
    for name in ("mixed_3x35x57", "mixed_3x35x57_time", "mixed_3x35x57_no_dots", "degenerate_4x12x20"):
        c = TC.cases()[name]
        on = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
        got = TC.render(on, backend="hip")
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), _want(name)), name
        got = TC.render(dict(c, frames=on["frames"]), backend="hip")                      # CUDA frames, numpy for the rest
        assert got.is_cuda and torch.equal(got.cpu(), _want(name)), name
    c = TC.cases()["mixed_3x35x57"]
    got = viz.paint_trails(c["frames"], c["tracks"], c["visibles"], trail=2, radius=2, backend="hip")      # the default colours, fade and width
    assert np.array_equal(got, viz.paint_trails(c["frames"], c["tracks"], c["visibles"], trail=2, radius=2))
    with pytest.raises(ValueError, match="trail"):                                        # one set of refusals for both backends
        viz.render(c["frames"], tracks=c["tracks"], trail=65, radius=2, backend="hip")
    with pytest.raises(ValueError, match="tracks"):
        viz.render(c["frames"], trail=2, backend="hip")


@pytest.mark.parametrize("name", ["mixed_3x35x57", "cross_5x17x258_w3.5", "rounds_6x20x40"])
def test_out_in_place_side_stream_and_sliced_views(dev, name):
    from fgvc_amd import ops
    frames, kw = _on(dev, TC.cases()[name])
    want = _want(name)
    T, H, W, _ = frames.shape
    out = torch.full_like(frames, 0xA5)                                                   # every byte is written: nothing to clear
    assert ops.render_trails(frames, out=out, **kw) is out and torch.equal(out.cpu(), want)
    own = frames.clone()
    assert ops.render_trails(own, out=own, **kw) is own and torch.equal(own.cpu(), want)  # in place
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = ops.render_trails(frames, **kw)
    side.synchronize()
    assert torch.equal(got.cpu(), want)
    # a cropped window of larger frames written into a cropped window between guard bands: the bands keep their sentinel
    big = torch.full((T, H + 3, W + 5, 3), 9, device=dev, dtype=torch.uint8)
    big[:, 2:-1, 3:-2] = frames
    kw3 = dict(kw)
    if "ids" in kw:
        big_ids = torch.full((T, H + 3, W + 5), 3, device=dev, dtype=torch.uint8)
        big_ids[:, 2:-1, 1:-4] = kw["ids"]
        kw3["ids"] = big_ids[:, 2:-1, 1:-4]
    big_out = torch.full((T, H + 4, W + 2, 3), 0x33, device=dev, dtype=torch.uint8)
    win = big_out[:, 1:-3, 1:-1]
    assert ops.render_trails(big[:, 2:-1, 3:-2], out=win, **kw3) is win
    assert torch.equal(win.cpu(), want)
    keep = torch.ones(big_out.shape[:3], dtype=torch.bool, device=dev)
    keep[:, 1:-3, 1:-1] = False
    assert bool((big_out[keep] == 0x33).all())
    ops.render_trails(big[:, 2:-1, 3:-2], out=big[:, 2:-1, 3:-2], **kw3)                  # in place on the cropped window
    assert torch.equal(big[:, 2:-1, 3:-2].cpu(), want) and bool((big[:, :2] == 9).all()) and bool((big[:, :, :3] == 9).all())
    assert bool((big[:, -1:] == 9).all()) and bool((big[:, :, -2:] == 9).all())
    # tracks and visibles seen through transposed views of (T, P, ...) tensors: read through their strides
    tp = kw["tracks"].transpose(0, 1).contiguous()
    kw4 = dict(kw, tracks=tp.transpose(0, 1))
    if "visibles" in kw:
        kw4["visibles"] = kw["visibles"].t().contiguous().t()
    assert torch.equal(ops.render_trails(frames, **kw4).cpu(), want)
    # refusals
    with pytest.raises(ValueError, match="out"):
        ops.render_trails(frames, out=torch.empty((T, H, W + 1, 3), device=dev, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="trail"):
        ops.render_trails(frames, **dict(kw, trail=0))
    with pytest.raises(ValueError, match="linewidth"):
        ops.render_trails(frames, **dict(kw, linewidth=17.0))
    with pytest.raises(ValueError, match="fade"):
        ops.render_trails(frames, **dict(kw, fade=torch.full((kw["trail"] + 1,), 0.5, device=dev, dtype=torch.float64)))
    with pytest.raises(ValueError, match="fade"):
        ops.render_trails(frames, **dict(kw, fade=torch.full((kw["trail"],), 1.5, device=dev, dtype=torch.float64)))
    with pytest.raises(ValueError, match="time_colors"):
        ops.render_trails(frames, **dict(kw, time_colors=torch.zeros((T, 3), device=dev, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="tracks"):
        ops.render_trails(frames, None)


def test_the_library_refuses_bad_arguments_before_any_launch(dev):
    from fgvc_amd import _lib
    lib = _lib.load()
    f = torch.zeros((2, 8, 8, 3), device=dev, dtype=torch.uint8)
    tr = torch.zeros((1, 2, 2), device=dev, dtype=torch.float64)
    fade = torch.ones(8, device=dev, dtype=torch.float64)
    col = torch.zeros((1, 3), device=dev, dtype=torch.uint8)

    def call(trail=8, lw=2.0, fade_ptr=None, tracks_ptr=None, colors_ptr=col.data_ptr()):
        return lib.fgvc_render_trails_u8(f.data_ptr(), 192, 24, f.data_ptr(), 192, 24, 2, 8, 8, None, 0, 0, None, 128, 1,
                                         tracks_ptr or tr.data_ptr(), 4, 2, None, 0, 0, colors_ptr, 1, 0, None, trail, lw, 2.25, 0.5,
                                         fade_ptr or fade.data_ptr(), None, None)
    for kw, text in ((dict(trail=0), b"trail"), (dict(trail=65), b"trail"), (dict(lw=0.5), b"linewidth"), (dict(lw=16.5), b"linewidth"),
                     (dict(fade_ptr=fade.data_ptr() + 4), b"8-byte"), (dict(tracks_ptr=tr.data_ptr() + 4), b"8-byte"),
                     (dict(colors_ptr=None), b"colors")):
        assert call(**kw) == _lib.ERR_INVALID_ARG and text in lib.fgvc_last_error(), kw
    assert call() == _lib.FGVC_OK
    torch.cuda.synchronize()


def _demo():
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(ROOT, "tools", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DEMO_MODEL = ["--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--precede-frames", "3", "--batch-step", "2"]


@pytest.mark.parametrize("chain", [False, True])
def test_demo_trails_write_what_the_host_renderer_gives(dev, tmp_path, chain):
    from PIL import Image
    from fgvc_amd import viz
    demo = _demo()
    T, H, W = 6, 64, 96
    argv = ["--synthetic", str(T), str(H), str(W), "--task", "points", "--out", str(tmp_path / "hip"), "--radius", "2", *DEMO_MODEL,
            "--query-points", "0", "20.5", "12", "0", "40", "30.25", "1", "10", "40", "3", "90", "60", "--trails"]
    if chain:
        argv += ["--chain", "--trail-color", "time", "--trail-width", "3"]
    r = demo.main(argv)
    extra = dict(linewidth=3.0, trail_color_by="time") if chain else {}
    want = viz.render(r["frames"], tracks=r["tracks"], visibles=r["visibles"], radius=2, trail=8, **extra)
    dots = viz.render(r["frames"], tracks=r["tracks"], visibles=r["visibles"], radius=2)
    assert np.array_equal(r["rendered"], want) and (want != dots).any()
    for t in (1, T - 1):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "hip" / f"frame_{t:05d}.png").convert("RGB")), want[t]), t
    r2 = demo.main([*argv[:argv.index("--out")], "--out", str(tmp_path / "host"), *argv[argv.index("--out") + 2:], "--host-render"])
    assert np.array_equal(r2["rendered"], r["rendered"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "host" / f"frame_{T - 1:05d}.png").convert("RGB")), want[T - 1])
