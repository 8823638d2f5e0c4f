"""GPU tests of the renderer (fgvc_render_frames_u8): ops.render_frames and viz's backend='hip' against the numpy
restatement of tests/render_cases.py (itself pinned to the reference's painter, tests/test_render_host.py) with torch.equal on every case --
the arithmetic is integer for the overlay and float64 without contraction for the points, so there is no tolerance -- and tools/demo.py
in-process on a tiny synthetic clip."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import render_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(RC.cases())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _want(name):
    return torch.from_numpy(RC.expected(name))


def _on(dev, c):
    """A case's arrays as ops.render_frames takes them."""
    kw = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    frames = kw.pop("frames")
    return frames, kw


def _report(name, got, want):
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist()) if len(bad) else ()
    return f"{name}: {bad.shape[0]} bytes differ; first (t, y, x, c) {bad[:6].tolist()}: got {got[first] if first else ''}, want {want[first] if first else ''}"


@pytest.mark.parametrize("name", NAMES)
def test_render_equals_the_restatement(dev, name):
    from fgvc_amd import ops
    frames, kw = _on(dev, RC.cases()[name])
    before = frames.clone()
    got = ops.render_frames(frames, **kw)
    assert got.dtype == torch.uint8 and got.shape == frames.shape and got.data_ptr() != frames.data_ptr()
    assert torch.equal(got.cpu(), _want(name)), _report(name, got.cpu(), _want(name))
    assert torch.equal(frames, before)


@pytest.mark.parametrize("name", list(RC.FIXTURES))
def test_render_equals_the_reference_painter(dev, name):
    from fgvc_amd import ops
    g = RC.fixture(name)
    on = {k: torch.from_numpy(g[k]).to(dev) for k in ("frames", "tracks", "visibles", "colors")}
    got = ops.render_frames(on["frames"], tracks=on["tracks"], visibles=on["visibles"], colors=on["colors"])      # radius=None: the reference's
    want = torch.from_numpy(g["out"])
    assert torch.equal(got.cpu(), want), _report(name, got.cpu(), want)
    # float32 tracks are widened exactly; visibles as uint8; tracks as a (T, P, 2) tensor seen through a transposed view
    t32 = on["tracks"].float()
    want32 = torch.from_numpy(RC.viz.paint_point_track(g["frames"], t32.cpu().numpy().astype(np.float64), g["visibles"], g["colors"]))
    assert torch.equal(ops.render_frames(on["frames"], tracks=t32, visibles=on["visibles"].to(torch.uint8), colors=on["colors"]).cpu(), want32)
    tp = on["tracks"].transpose(0, 1).contiguous()
    vp = on["visibles"].t().contiguous()
    assert torch.equal(ops.render_frames(on["frames"], tracks=tp.transpose(0, 1), visibles=vp.t(), colors=on["colors"]).cpu(), want)


@pytest.mark.parametrize("name", ["mixed_2x35x57", "mixed_2x17x258", "ref_3x40x56"])
def test_out_in_place_side_stream_and_sliced_views(dev, name):
    from fgvc_amd import ops
    frames, kw = _on(dev, RC.cases()[name])
    want = _want(name)
    T, H, W, _ = frames.shape
    out = torch.full_like(frames, 0xA5)                                                  # every byte is written: nothing to clear
    assert ops.render_frames(frames, out=out, **kw) is out and torch.equal(out.cpu(), want)
    assert torch.equal(ops.render_frames(frames, out=out, **kw).cpu(), want)              # a second call on the same buffer
    own = frames.clone()
    assert ops.render_frames(own, out=own, **kw) is own and torch.equal(own.cpu(), want)  # in place
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        got = ops.render_frames(frames, **kw)
    side.synchronize()
    assert torch.equal(got.cpu(), want)
    # every other frame of an interleaved stack, frames and ids alike, written into every other frame of a sentinel stack
    ids = kw.get("ids")
    junk = torch.full_like(frames, 7)
    f2 = torch.stack([frames, junk], 1).reshape(2 * T, H, W, 3)
    kw2 = dict(kw)
    if ids is not None:
        kw2["ids"] = torch.stack([ids, 255 - ids], 1).reshape(2 * T, H, W)[::2]
    assert T == 1 or not f2[::2].is_contiguous()
    o2 = torch.full((2 * T, H, W, 3), 0x5A, device=dev, dtype=torch.uint8)
    ops.render_frames(f2[::2], out=o2[::2], **kw2)
    assert torch.equal(o2[::2].cpu(), want) and bool((o2[1::2] == 0x5A).all())
    # a cropped window of larger frames / ids, written into a cropped window: the border keeps its sentinel, rows start at any alignment
    big = torch.full((T, H + 3, W + 5, 3), 9, device=dev, dtype=torch.uint8)
    big[:, 2:-1, 3:-2] = frames
    kw3 = dict(kw)
    if ids is not None:
        big_ids = torch.full((T, H + 3, W + 5), 3, device=dev, dtype=torch.uint8)
        big_ids[:, 2:-1, 1:-4] = ids
        kw3["ids"] = big_ids[:, 2:-1, 1:-4]
    big_out = torch.full((T, H + 4, W + 2, 3), 0x33, device=dev, dtype=torch.uint8)
    win = big_out[:, 1:-3, 1:-1]
    assert ops.render_frames(big[:, 2:-1, 3:-2], out=win, **kw3) is win
    assert torch.equal(win.cpu(), want)
    keep = torch.ones(big_out.shape[:3], dtype=torch.bool, device=dev)
    keep[:, 1:-3, 1:-1] = False
    assert bool((big_out[keep] == 0x33).all())
    # in place on the cropped window
    ops.render_frames(big[:, 2:-1, 3:-2], out=big[:, 2:-1, 3:-2], **kw3)
    assert torch.equal(big[:, 2:-1, 3:-2].cpu(), want) and bool((big[:, :2] == 9).all()) and bool((big[:, :, :3] == 9).all())
    # a channel-planar tensor seen as (T, H, W, 3) has no packed pixels: copied, same result
    planar = frames.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert torch.equal(ops.render_frames(planar, **kw).cpu(), want)
    # refusals
    with pytest.raises(ValueError, match="out"):
        ops.render_frames(frames, out=torch.empty((T, H, W + 1, 3), device=dev, dtype=torch.uint8), **kw)
    with pytest.raises(ValueError, match="out"):
        ops.render_frames(frames, out=torch.empty((T, H, W, 3), device=dev, dtype=torch.int8), **kw)
    with pytest.raises(ValueError, match="out"):
        ops.render_frames(frames, out=torch.empty((T, 3, H, W), device=dev, dtype=torch.uint8).permute(0, 2, 3, 1), **kw)
    with pytest.raises(TypeError, match="uint8"):
        ops.render_frames(frames.float(), **kw)
    with pytest.raises(ValueError, match="radius"):
        ops.render_frames(frames, tracks=torch.zeros(1, T, 2, device=dev), radius=32)
    with pytest.raises(ValueError, match="radius"):
        ops.render_frames(frames, tracks=torch.zeros(1, T, 2, device=dev), radius=0)
    with pytest.raises(ValueError, match="alpha"):
        ops.render_frames(frames, ids=torch.zeros((T, H, W), device=dev, dtype=torch.uint8), alpha=300)
    assert tuple(ops.render_frames(frames[:0]).shape) == (0, H, W, 3)


def test_viz_hip_backend_returns_the_matching_container(dev):
    from fgvc_amd import viz
    for name in ("mixed_2x35x57", "ref_2x100x104", "objects_255_1x32x40", "neither_2x35x57"):
        c = RC.cases()[name]
        got = viz.render(backend="hip", **c)                                              # numpy in, numpy out
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, RC.expected(name)), name
        frames, kw = _on(dev, c)
        got = viz.render(frames, backend="hip", **kw)                                     # CUDA in, CUDA out
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), _want(name)), name
        mixed = dict(c, frames=frames)                                                    # CUDA frames, numpy for the rest
        assert torch.equal(viz.render(backend="hip", **mixed).cpu(), _want(name))
    c = RC.cases()["mixed_2x35x57"]
    got = viz.paint_point_track(c["frames"], c["tracks"], c["visibles"], backend="hip", radius=2)       # the default colours
    assert np.array_equal(got, viz.paint_point_track(c["frames"], c["tracks"], c["visibles"], radius=2))
    got = viz.overlay_masks(torch.from_numpy(c["frames"]).to(dev), c["ids"], alpha=99, contour=False, backend="hip")
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), viz.overlay_masks(c["frames"], c["ids"], alpha=99, contour=False))


def _demo():
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(ROOT, "tools", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DEMO_MODEL = ["--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--precede-frames", "3", "--batch-step", "2"]


@pytest.mark.parametrize("task", ["points", "vos"])
def test_demo_writes_what_the_host_renderer_gives(dev, tmp_path, task):
    from PIL import Image
    from fgvc_amd import viz
    demo = _demo()
    T, H, W = 5, 48, 64
    argv = ["--synthetic", str(T), str(H), str(W), "--task", task, "--out", str(tmp_path), "--radius", "2", *DEMO_MODEL]
    if task == "points":
        argv += ["--query-points", "0", "20.5", "12", "0", "40", "30.25", "1", "10", "40", "2", "63", "47"]
    else:
        mask = np.zeros((H, W), np.uint8)
        mask[6:22, 8:28], mask[24:44, 30:58] = 1, 2
        Image.fromarray(mask).save(tmp_path / "first.png")
        argv += ["--first-mask", str(tmp_path / "first.png")]
    r = demo.main(argv)
    frames = r["frames"]
    assert frames.dtype == np.uint8 and frames.shape == (T, H, W, 3)
    if task == "points":
        assert r["tracks"].shape == (4, T, 2) and r["visibles"].shape == (4, T) and r["ids"] is None
        assert sorted(r["query_points"][:, 0].tolist()) == [0.0, 0.0, 1.0, 2.0]            # (in the order of the tracks' rows)
        assert np.array_equal(r["visibles"], np.arange(T)[None, :] >= r["query_points"][:, :1]) and not r["visibles"].all()
        assert np.isfinite(r["tracks"]).all() and r["tracks"].dtype == np.float64
        want = viz.render(frames, tracks=r["tracks"], visibles=r["visibles"], radius=2)
    else:
        assert r["tracks"] is None and r["ids"].shape == (T, H, W) and r["ids"].dtype == np.uint8 and np.array_equal(r["ids"][0], mask)
        want = viz.render(frames, ids=r["ids"])
    assert (want != frames).any()
    for t in range(T):
        png = np.asarray(Image.open(tmp_path / f"frame_{t:05d}.png").convert("RGB"))
        assert np.array_equal(png, want[t]), (task, t)
    gif = Image.open(tmp_path / "demo.gif")
    assert gif.n_frames == T and gif.size == (W, H)
    # the host renderer writes the same files
    other = tmp_path / "host"
    r2 = demo.main([*argv[:argv.index("--out")], "--out", str(other), *argv[argv.index("--out") + 2:], "--host-render"])
    assert np.array_equal(r2["rendered"], r["rendered"]) and np.array_equal(r["rendered"], want)
    assert np.array_equal(np.asarray(Image.open(other / "frame_00004.png").convert("RGB")), want[4])
