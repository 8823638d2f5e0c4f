"""GPU tests of the pose renderer (fgvc_render_pose_u8) and of the joint peaks (fgvc_heatmap_coords_peak_f32):
ops.render_pose and viz's backend='hip' against viz's host backend on every case of tests/pose_cases.py with torch.equal -- float64 without
contraction, no square root, one correctly rounded division: there is no tolerance; the peaks against the merged soft-map read-out with `==`;
test_cfg.pose through both trackers; tools/demo.py --task pose in-process and tools/test.py --render as a command."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import pose_cases as PC
from tests import render_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(PC.cases())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _want(name):
    return torch.from_numpy(PC.expected(name).copy())                 # (the shared array is read-only)


def _on(dev, c):
    """A case as ops.render_pose takes it: (frames, keyword arguments), everything on the device."""
    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    kw = {k: c[k] for k in ("limb_width", "limb_alpha", "heat_gain", "heat_alpha", "radius", "alpha", "contour", "dots") if k in c}
    for k in ("tracks", "visibles", "colors", "skeleton", "limb_colors", "heat", "heat_colors", "ids", "palette"):
        if c.get(k) is not None:
            kw[k] = up(c[k])
    return up(c["frames"]), kw


def _report(name, got, want):
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist()) if len(bad) else ()
    return f"{name}: {bad.shape[0]} bytes differ; first (t, y, x, c) {bad[:6].tolist()}: got {got[first] if first else ''}, want {want[first] if first else ''}"


@pytest.mark.parametrize("name", NAMES)
def test_render_pose_equals_the_host_backend(dev, name):
    from fgvc_amd import ops
    frames, kw = _on(dev, PC.cases()[name])
    before = frames.clone()
    got = ops.render_pose(frames, **kw)
    assert got.dtype == torch.uint8 and got.shape == frames.shape and got.data_ptr() != frames.data_ptr()
    assert torch.equal(got.cpu(), _want(name)), _report(name, got.cpu(), _want(name))
    assert torch.equal(frames, before)


@pytest.mark.parametrize("name", NAMES)
def test_viz_hip_backend_equals_the_host_backend(dev, name):
    got = PC.render(PC.cases()[name], backend="hip")                                      # numpy in, numpy out
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8
    assert np.array_equal(got, PC.expected(name)), _report(name, torch.from_numpy(got), _want(name))


def test_cuda_tensor_in_cuda_tensor_out_and_refusals(dev):
    from fgvc_amd import ops, viz
    for name in ("all_3x35x57", "all_3x35x57_no_dots", "all_3x35x57_default_colours", "heat_2x11x261_k3_float64"):
        c = PC.cases()[name]
        on = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if isinstance(v, np.ndarray) and k != "skeleton" else v)
              for k, v in c.items()}
        got = PC.render(on, backend="hip")
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), _want(name)), name
    c = PC.cases()["all_3x35x57"]
    f, tr = c["frames"], c["tracks"]
    with pytest.raises(ValueError, match="trail: not together with skeleton= or heat="):  # one set of refusals for both backends
        viz.render(f, tracks=tr, trail=2, skeleton=c["skeleton"], radius=2, backend="hip")
    with pytest.raises(ValueError, match="skeleton: needs tracks"):
        viz.render(f, skeleton=c["skeleton"], backend="hip")
    with pytest.raises(ValueError, match=r"skeleton: edge 0 = \(0, 99\)"):
        viz.render(f, tracks=tr, skeleton=[(0, 99)], radius=2, backend="hip")
    with pytest.raises(ValueError, match="heat_gain"):
        viz.render(f, heat=c["heat"], heat_gain=0.0, backend="hip")
    with pytest.raises(ValueError, match="heat: "):
        viz.render(f, heat=c["heat"][:, :, 1:], backend="hip")
    frames, kw = _on(dev, c)
    with pytest.raises(ValueError, match="skeleton: needs tracks"):
        ops.render_pose(frames, skeleton=kw["skeleton"])
    with pytest.raises(ValueError, match=r"skeleton: edge 1 = "):
        ops.render_pose(frames, **dict(kw, skeleton=torch.tensor([(0, 1), (2, 10 ** 6)], device=dev)))
    with pytest.raises(ValueError, match="heat_alpha"):
        ops.render_pose(frames, **dict(kw, heat_alpha=1.5))
    with pytest.raises(ValueError, match="limb_width"):
        ops.render_pose(frames, **dict(kw, limb_width=17.0))
    with pytest.raises(TypeError, match="heat"):
        ops.render_pose(frames, **dict(kw, heat=kw["heat"].half()))


@pytest.mark.parametrize("name", list(RC.cases()))
def test_render_pose_without_a_pose_is_render_frames(dev, name):
    from fgvc_amd import ops
    c = RC.cases()[name]

    def up(x):
        return torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    kw = {k: (up(v) if isinstance(v, np.ndarray) else v) for k, v in c.items() if k != "frames" and v is not None}
    frames = up(c["frames"])
    got = ops.render_pose(frames, **kw)
    assert torch.equal(got, ops.render_frames(frames, **kw)) and torch.equal(got.cpu(), torch.from_numpy(RC.expected(name).copy())), name


@pytest.mark.parametrize("name", ["heat_2x11x261_k3_float32", "heat_2x11x261_k17_float64", "all_3x35x57"])
def test_strided_maps_time_slices_and_windows_in_place(dev, name):
    from fgvc_amd import ops
    frames, kw = _on(dev, PC.cases()[name])
    want = _want(name)
    T, H, W, _ = frames.shape
    heat = kw["heat"]
    K = heat.shape[1]
    # the maps as every second channel of a larger tensor, inside a window of larger planes, at an odd element offset
    big = torch.full((T, 2 * K + 1, H + 3, W + 5), float("nan"), device=dev, dtype=heat.dtype)
    view = big[:, 1:2 * K + 1:2, 2:2 + H, 3:3 + W]
    view.copy_(heat)
    assert not view.is_contiguous() and view.stride(1) == 2 * big.stride(1)
    assert torch.equal(ops.render_pose(frames, **dict(kw, heat=view)).cpu(), want)
    # a time slice of frames, maps and tracks
    sl = dict(kw, heat=view[1:])
    for k in ("tracks", "visibles"):
        if k in kw:
            sl[k] = kw[k][:, 1:]
    if "ids" in kw:
        sl["ids"] = kw["ids"][1:]
    assert torch.equal(ops.render_pose(frames[1:], **sl).cpu(), want[1:])
    # a cropped window of larger frames, painted in place: the guard bands keep their sentinel
    wide = torch.full((T, H + 3, W + 5, 3), 9, device=dev, dtype=torch.uint8)
    win = wide[:, 2:-1, 3:-2]
    win.copy_(frames)
    assert ops.render_pose(win, out=win, **dict(kw, heat=view)) is win
    assert torch.equal(win.cpu(), want)
    keep = torch.ones(wide.shape[:3], dtype=torch.bool, device=dev)
    keep[:, 2:-1, 3:-2] = False
    assert bool((wide[keep] == 9).all())
    out = torch.full_like(frames, 0xA5)                                                   # every byte is written: nothing to clear
    assert ops.render_pose(frames, out=out, **kw) is out and torch.equal(out.cpu(), want)


def test_the_library_refuses_bad_arguments_before_any_launch(dev):
    from fgvc_amd import _lib
    lib = _lib.load()
    f = torch.zeros((2, 8, 8, 3), device=dev, dtype=torch.uint8)
    tr = torch.zeros((2, 2, 2), device=dev, dtype=torch.float64)
    sk = torch.zeros((1, 2), device=dev, dtype=torch.int32)
    col = torch.zeros((2, 3), device=dev, dtype=torch.uint8)
    heat = torch.zeros((2, 2, 8, 8), device=dev, dtype=torch.float32)

    def call(E=1, lw=2.0, la=1.0, K=2, gain=1.0, ha=0.5, heat_ptr=heat.data_ptr(), hcol=col.data_ptr(), lcol=col.data_ptr(), h_sy=8):
        return lib.fgvc_render_pose_u8(f.data_ptr(), 192, 24, f.data_ptr(), 192, 24, 2, 8, 8, None, 0, 0, None, 128, 1, tr.data_ptr(), 4, 2,
                                       None, 0, 0, col.data_ptr(), 2, 0, None, sk.data_ptr(), E, lcol, lw, 2.25, 0.5, la, heat_ptr, 0, K, 128, 64,
                                       h_sy, hcol, gain, ha, None)
    for kw, text in ((dict(lw=0.5), b"limb_width"), (dict(lw=16.5), b"limb_width"), (dict(la=1.5), b"limb_alpha"), (dict(K=0), b"K=0"),
                     (dict(K=257), b"K=257"), (dict(gain=0.0), b"heat_gain"), (dict(gain=float("inf")), b"heat_gain"), (dict(ha=-0.5), b"heat_alpha"),
                     (dict(heat_ptr=heat.data_ptr() + 2), b"aligned"), (dict(hcol=None), b"heat_colors"), (dict(lcol=None), b"limb_colors"),
                     (dict(h_sy=7), b"row stride"), (dict(E=-1), b"E=-1")):
        assert call(**kw) == _lib.ERR_INVALID_ARG and text in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())
    assert call() == _lib.FGVC_OK
    torch.cuda.synchronize()


# ---- the peaks --------------------------------------------------------------------------------------------------------------------------
def _peak_cases():
    from tests.test_gpu_heatmap import READOUT_CASES
    return list(READOUT_CASES) + [(1, 6, (41, 47), 2, (21, 24), (45, 52), torch.float32), (1, 3, (30, 40), 2, (15, 20), (30, 40), torch.float64)]


@pytest.mark.parametrize("case", _peak_cases(), ids=lambda c: f"T{c[0]}K{c[1]}_{c[2][0]}x{c[2][1]}_to_{c[5][0]}x{c[5][1]}_{str(c[6])[-7:]}")
def test_peaks_are_the_readouts_largest_values(dev, case):
    """The oracle is the merged read-out: ops.softmap_readout writes the field that the coordinate kernels scan, bit for bit."""
    from fgvc_amd import ops
    from tests.test_gpu_heatmap import _readout_case
    heat, bank, map_pad, Hf, Wf, out_shape = _readout_case(dev, case, 7)
    heat, bank = heat.to(dev), bank.to(dev)
    T, K = bank.shape[0], heat.shape[0]
    plain = ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape)
    coords, peak = ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape, peak=True)
    assert coords.shape == (2, K, T) and peak.shape == (K, T) and peak.dtype == torch.float64
    assert torch.equal(coords.view(torch.int64), plain.view(torch.int64))                 # bit for bit
    want = torch.empty((T, K), device=dev, dtype=torch.float64)
    for f in range(T):                                                                    # a frame at a time: the whole stack is never needed
        want[f] = ops.softmap_readout(bank, heat, Hf, Wf, map_pad, out_shape, frames=(f, f + 1)).amax((2, 3)).double()[0]
    assert torch.equal(peak, want.t()), (peak - want.t()).abs().max()
    if K >= 4:                                                                            # _readout_case's all-zero joint
        assert bool((peak[0] == 0).all()) and bool((coords[:, 0] == -1).all())
    for other in (True, False):                                                           # the arithmetic flag does not touch the peak
        c2, p2 = ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape, f64_arith=other, peak=True)
        assert torch.equal(p2, peak)
        assert torch.equal(c2.view(torch.int64), ops.heatmap_coords(bank, heat, Hf, Wf, map_pad, out_shape, f64_arith=other).view(torch.int64))


def test_engine_propagate_heatmaps_with_peaks(dev):
    from fgvc_amd import engine
    from tests.test_gpu_heatmap import _clip, heat_maps
    T, h, w, d, K = 4, 30, 38, 2, 5
    (hp, wp), _ = engine.pad_divide_by(h, w, d)
    Hf, Wf = hp // d, wp // d
    _, map_pad = engine.pad_divide_by(h, w, d)
    heat = heat_maps(K, h, w, 3.0, np.random.default_rng(5), torch.float32).to(dev)
    feats = _clip(dev, T, 64, Hf, Wf, 11)
    cfg = engine.TrackerConfig(neighbor_range=8, precede_frames=3)
    plain = engine.propagate_heatmaps(feats, Hf, Wf, heat, map_pad, (h, w), cfg)
    field = []
    coords, peak = engine.propagate_heatmaps(feats, Hf, Wf, heat, map_pad, (h, w), cfg, peak=True, field_out=field)
    assert torch.equal(coords, plain) and peak.shape == (K, T)
    maps = engine.propagate_softmaps(feats, Hf, Wf, heat, map_pad, (h, w), cfg)
    assert torch.equal(field[0].maps(0, T), maps) and torch.equal(field[0].maps(1, 3), maps[1:3])
    assert torch.equal(peak, maps.amax((2, 3)).double().t())


# ---- the trackers -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["softmap_jhmdb_6x48x64", "hr_softmap_jhmdb_6x48x64"])
def test_trackers_keep_their_output_and_report_the_peaks(dev, golden, name):
    from fgvc_amd import engine
    from tests.test_gpu_softmap import _call, _model
    g = golden(name)
    kind = "HRVanillaTracker" if name.startswith("hr_") else "VanillaTracker"
    plain_model = _model(dev, g, kind, "f16x3", dict(coords=True))
    plain = _call(plain_model, g, dev)
    assert plain_model.last_pose is None and len(plain) == 1
    model = _model(dev, g, kind, "f16x3", dict(coords=True, pose=dict(confidence=True, keep_field=True)))
    out = _call(model, g, dev)
    K, T = plain[0].shape[1:]
    assert len(out) == 1 and out[0].dtype == np.float64 and np.array_equal(out[0], plain[0])
    lp = model.last_pose
    assert sorted(lp) == ["field", "peak"] and lp["peak"].shape == (K, T) and lp["peak"].dtype == np.float64
    assert isinstance(lp["field"], engine.PoseField) and lp["field"].num_frames == T and lp["field"].num_joints == K
    maps = _call(_model(dev, g, kind, "f16x3", dict(return_maps=True)), g, dev)[0]
    got = lp["field"].maps(0, T)
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), maps)
    assert np.array_equal(lp["field"].maps(2, 4).cpu().numpy(), maps[2:4])
    assert np.array_equal(lp["peak"], maps.max((2, 3)).T.astype(np.float64))
    light = _model(dev, g, kind, "f16x3", dict(coords=True, pose=dict(keep_field=False)))
    assert np.array_equal(_call(light, g, dev)[0], plain[0]) and light.last_pose["field"] is None
    assert np.array_equal(light.last_pose["peak"], lp["peak"])
    off = _model(dev, g, kind, "f16x3", dict(coords=True, pose=dict(confidence=False)))
    assert np.array_equal(_call(off, g, dev)[0], plain[0]) and off.last_pose == dict(peak=None, field=None)


# ---- the tools --------------------------------------------------------------------------------------------------------------------------
def _demo():
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(ROOT, "tools", "demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


DEMO_MODEL = ["--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--precede-frames", "3", "--batch-step", "2"]


@pytest.mark.parametrize("tracker", ["VanillaTracker", "HRVanillaTracker"])
def test_demo_pose_writes_what_the_host_renderer_gives(dev, tmp_path, tracker):
    from PIL import Image
    from fgvc_amd import viz
    demo = _demo()
    T, H, W = 3, 32, 48
    argv = ["--synthetic", str(T), str(H), str(W), "--task", "pose", "--out", str(tmp_path / "hip"), "--radius", "2", *DEMO_MODEL, "--tracker",
            tracker, "--joints", "10", "8", "24.5", "16", "40", "25", "--skeleton", "0-1", "1-2", "--heat", "--heat-gain", "1.5", "--limb-width", "3"]
    r = demo.main(argv)
    assert r["tracks"].shape == (3, T, 2) and r["visibles"].shape == (3, T) and r["peak"].shape == (3, T) and r["visibles"].all()
    dots = viz.render(r["frames"], tracks=r["tracks"], visibles=r["visibles"], radius=2)
    assert r["rendered"].shape == r["frames"].shape and (r["rendered"] != dots).any()
    for t in range(T):
        assert np.array_equal(np.asarray(Image.open(tmp_path / "hip" / f"frame_{t:05d}.png").convert("RGB")), r["rendered"][t]), t
    r2 = demo.main([*argv[:argv.index("--out")], "--out", str(tmp_path / "host"), *argv[argv.index("--out") + 2:], "--host-render"])
    assert np.array_equal(r2["rendered"], r["rendered"]) and np.array_equal(r2["tracks"], r["tracks"])
    assert np.array_equal(np.asarray(Image.open(tmp_path / "host" / f"frame_{T - 1:05d}.png").convert("RGB")), r["rendered"][T - 1])
    hidden = demo.main([*argv, "--min-conf", "1e9"])                                      # no joint is that sure: no limb, no dot, the maps alone
    assert not hidden["visibles"].any() and (hidden["rendered"] != r["rendered"]).any()
    with pytest.raises(ValueError, match="--heat: the heat overlay needs maps at the frames' size"):
        a = demo.parse_args(argv)
        a.size, a.yuv_packed, a.yuv_input = (16, 24), None, None
        demo.run_pose(a, r["frames"], dev)


def test_tools_test_renders_every_clip(dev, tmp_path):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("make_fake_poses", os.path.join(ROOT, "tools", "make_fake_poses.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mk.make_jhmdb(str(tmp_path), videos=2, frames=4, seed=3)
    out = tmp_path / "painted"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--task", "jhmdb", "--data-root", str(tmp_path), "--pose-form",
                          "heatmap", "--render", str(out), "--min-conf", "0.01", "--out", str(tmp_path / "pck.json")], capture_output=True,
                         text=True, timeout=600, cwd=ROOT)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    clips = sorted(os.listdir(out))
    assert len(clips) == 2, clips
    for c in clips:
        names = sorted(os.listdir(out / c))
        assert names == [f"frame_{t:05d}.png" for t in range(4)], (c, names)
        assert np.asarray(Image.open(out / c / names[0])).shape == (60, 80, 3)            # the clip's own size
