"""Host tests of the soft-map output (test_cfg.return_maps=True: the propagated (T, K, h0, w0) maps themselves, the reference's
coords=False return value of forward_test_backward_save_mem, vanilla_tracker.py:770-784, :800-803): dispatch and refusals on both
trackers, the new library entry and its argument checks, the read-out kernels' code-object notes, the chunk plan of the host-bound
result, the host decoder of tools/test.py --pose-form softmap, and the fixtures' own consistency.  No GPU."""
import ctypes
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
DENSE_FIXTURES = ["softmap_jhmdb_6x48x64", "softmap_badja_6x56x80", "softmap_pad_5x41x47"]
LOCAL_FIXTURES = ["hr_softmap_jhmdb_6x48x64", "hr_softmap_pad_5x41x47"]
HR_CFG = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8)


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _model(kind, **test_cfg):
    import fgvc_amd.mmpt_api as api
    if kind == "HRVanillaTracker":
        test_cfg = {**HR_CFG, **test_cfg}
    return api.build_model(dict(type=kind, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                           test_cfg=dict(test_cfg)).eval()


IMGS = torch.zeros(1, 1, 3, 3, 16, 16)
META = [dict(original_shape=(16, 16))]


@pytest.mark.parametrize("kind", ["VanillaTracker", "HRVanillaTracker"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_return_maps_reaches_the_gpu_path(kind, dtype):
    """return_maps=True with 4-D labels passes every refusal and stops only at the device check (NotImplementedError before this change)."""
    m = _model(kind, return_maps=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(test_mode=True, imgs=IMGS, ref_seg_map=torch.zeros(1, 2, 16, 16, dtype=dtype), img_meta=META)


@pytest.mark.parametrize("kind", ["VanillaTracker", "HRVanillaTracker"])
def test_refusals(kind):
    heat = torch.zeros(1, 2, 16, 16)
    seg = torch.zeros(1, 16, 16, dtype=torch.long)
    call = lambda m, **kw: m(test_mode=True, **{**dict(imgs=IMGS, ref_seg_map=heat, img_meta=META), **kw})
    with pytest.raises(NotImplementedError, match="full-resolution soft maps are not returned"):      # without the key: as before
        call(_model(kind))
    with pytest.raises(NotImplementedError, match="full-resolution soft maps are not returned"):
        call(_model(kind, return_maps=False))
    with pytest.raises(ValueError, match="two read-outs"):
        call(_model(kind, return_maps=True, coords=True))
    with pytest.raises(NotImplementedError, match="one-hot"):
        call(_model(kind, return_maps=True), ref_seg_map=seg)
    with pytest.raises(NotImplementedError, match="save_np"):
        call(_model(kind, return_maps=True, save_np=True))
    m = _model(kind, return_maps=True)
    with pytest.raises(NotImplementedError, match="hard_prop"):
        call(_model(kind, return_maps=True, hard_prop=True))
    with pytest.raises(NotImplementedError, match="batch size 1"):
        call(m, imgs=IMGS.repeat(2, 1, 1, 1, 1, 1), ref_seg_map=heat.repeat(2, 1, 1, 1), img_meta=META * 2)
    with pytest.raises(TypeError, match="float32 or float64"):
        call(m, ref_seg_map=heat.to(torch.float16))
    with pytest.raises(NotImplementedError, match="1 to 256 joints"):
        call(m, ref_seg_map=torch.zeros(1, 257, 16, 16))
    # the heat-map path's order: hard_prop is read before the batch size, the batch size before the dtype
    with pytest.raises(NotImplementedError, match="hard_prop"):
        call(_model(kind, return_maps=True, hard_prop=True), imgs=IMGS.repeat(2, 1, 1, 1, 1, 1), ref_seg_map=heat.to(torch.float16))
    with pytest.raises(NotImplementedError, match="batch size 1"):
        call(m, imgs=IMGS.repeat(2, 1, 1, 1, 1, 1), ref_seg_map=heat.to(torch.float16))


def test_hr_tracker_keeps_its_own_refusals():
    import fgvc_amd.mmpt_api as api
    with pytest.raises(AttributeError, match="temperature"):                 # _label_config: attributes with no default, read first
        api.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                    pool_type="none")),
                        test_cfg=dict(return_maps=True, precede_frames=3, topk=10)).eval()(
            test_mode=True, imgs=IMGS, ref_seg_map=torch.zeros(1, 2, 16, 16), img_meta=META)


def _args(**kw):
    """Arguments of fgvc_softmap_readout_f32 with non-null dummy pointers; the argument checks return before anything is launched."""
    a = dict(bank=8, map0=8, map0_f64=0, T=4, Hf=5, Wf=6, K=3, hm=10, wm=12, hp=10, wp=12, top=0, left=0, h0=10, w0=12, f_begin=0, f_end=4,
             out_f64=0, out=8, stream=None)
    a.update(kw)
    return [ctypes.c_void_p(v) if k in ("bank", "map0", "out", "stream") else v for k, v in a.items()]


def test_library_entry_and_argument_checks():
    from fgvc_amd import _lib
    assert "fgvc_softmap_readout_f32" in _lib.SIGNATURES
    lib = _lib.load()
    fn = lib.fgvc_softmap_readout_f32
    with open(os.path.join(ROOT, "include", "fgvc_hip.h")) as f:
        assert "int fgvc_softmap_readout_f32(" in f.read()
    for bad, word in ((dict(map0=None), "null pointer"), (dict(out=None), "null pointer"), (dict(bank=None), "null pointer"),
                      (dict(f_begin=2, f_end=2), "frame range"), (dict(f_begin=3, f_end=1), "frame range"), (dict(f_end=5), "frame range"),
                      (dict(f_begin=-1), "frame range"), (dict(K=0), "1 <= K <= 256"), (dict(K=257), "1 <= K <= 256"),
                      (dict(top=1), "inside the padded frame"), (dict(h0=0), "bad shape")):
        assert fn(*_args(**bad)) == _lib.ERR_INVALID_ARG, bad
        text = lib.fgvc_last_error().decode()
        assert text.startswith("fgvc_softmap_readout_f32:") and word in text, (bad, text)


def test_readout_kernels_are_scratch_free():
    notes = _tool("kernel_notes").kernel_notes()
    later = {k: v for k, v in notes.items() if "softmap_kernel" in k}
    first = {k: v for k, v in notes.items() if "softmap0_kernel" in k}
    assert len(later) == 4 and len(first) == 2, (sorted(later), sorted(first))      # COMPOSED x output dtype; map dtype (output dtype: a flag)
    for k, v in {**later, **first}.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
    for k, v in later.items():
        assert v["group_segment_fixed_size"] <= 32 << 10, (k, v)               # the staged footprint + the row taps: 5 workgroups / CU or more


def test_chunk_plan():
    from fgvc_amd import engine
    assert engine.MAPS_BUDGET == 512 << 20
    frame = 16 * 480 * 854 * 4
    assert engine.plan_map_chunks(100, 16, (480, 854), 4) == [(f, min(f + 20, 100)) for f in range(0, 100, 20)]     # 26.2 MB a frame
    assert engine.plan_map_chunks(100, 16, (480, 854), 8)[0] == (0, 10)
    assert engine.plan_map_chunks(8, 16, (480, 854), 4) == [(0, 8)]
    assert engine.plan_map_chunks(7, 16, (480, 854), 4, budget=2 * frame) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert engine.plan_map_chunks(7, 16, (480, 854), 4, budget=3 * frame - 1) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert engine.plan_map_chunks(3, 16, (480, 854), 4, budget=frame) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError, match=str(frame)):
        engine.plan_map_chunks(3, 16, (480, 854), 4, budget=frame - 1)
    with pytest.raises(ValueError, match="maps_budget"):
        engine.plan_map_chunks(3, 16, (480, 854), 8, budget=frame)
    for kind in ("VanillaTracker", "HRVanillaTracker"):
        assert _model(kind, return_maps=True)._maps_budget() == engine.MAPS_BUDGET
        assert _model(kind, return_maps=True, maps_budget=12345)._maps_budget() == 12345


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_host_decoder_is_img2coord(dtype):
    from fgvc_amd.datasets import MapsAsCoords, img2coord_maps
    from oracle import fgvc_oracle as O
    rng = np.random.default_rng(3)
    maps = rng.random((4, 5, 23, 31)).astype(dtype)                 # continuous values: no ties
    maps[:, 2] = 0                                                  # a zero map: (-1, -1)
    maps[2, 3] -= 0.5                                               # negative values
    want = O.img2coord(maps)
    got = img2coord_maps(maps)
    assert got.shape == (2, 5, 4) and got.dtype == np.float64
    assert np.array_equal(got, want)
    assert np.array_equal(got[:, 2], np.full((2, 4), -1.0))
    # ties: the higher flat index first among equals
    flat = np.zeros((1, 1, 2, 8), dtype=dtype)
    flat[0, 0, 0, :] = 1.0
    flat[0, 0, 1, :3] = 1.0                                        # 11 equal maxima: the top 5 are flat indices 10, 9, 8, 7, 6
    c = img2coord_maps(flat)
    assert c[0, 0, 0] == pytest.approx((2 + 1 + 0 + 7 + 6) / 5, abs=1e-6) and c[1, 0, 0] == pytest.approx(3 / 5, abs=1e-6)
    # the adapter the tool scores through
    seen = []
    wrapped = MapsAsCoords(lambda **kw: [maps], on_maps=lambda i, m: seen.append((i, m.shape)))
    assert np.array_equal(wrapped(test_mode=True)[0], got) and np.array_equal(wrapped(test_mode=True)[0], got)
    assert seen == [(0, maps.shape), (1, maps.shape)]


@pytest.mark.parametrize("name", DENSE_FIXTURES + LOCAL_FIXTURES)
def test_fixture_self_checks(name):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 1000000
    g = dict(np.load(path, allow_pickle=False))
    heat = g["ref_seg_map"]
    T = g["imgs"].shape[1]                                   # (1, T, 3, h, w)
    K = heat.shape[0]
    shape = tuple(int(v) for v in g["original_shape"])
    assert g["imgs"].dtype == np.float16 and heat.ndim == 3 and heat.dtype in (np.float32, np.float64)
    assert g["maps0"].shape == (K, *shape) and g["maps0"].dtype == heat.dtype           # frame 0 in the stack's dtype
    assert g["maps"].shape == (T - 1, K, *shape) and g["maps"].dtype == np.float32       # frames >= 1: float32 values
    assert np.isfinite(g["maps"]).all() and np.isfinite(g["maps0"]).all()
    cfg = json.loads(str(g["test_cfg"]))
    assert "coords" not in cfg and "return_maps" not in cfg
    # the clip is the heat-map fixture's: same frames, labels and settings, so that fixture's coords describe the same run
    h = dict(np.load(os.path.join(GOLDEN, name.replace("softmap", "heatmap") + ".npz"), allow_pickle=False))
    assert np.array_equal(h["imgs"], g["imgs"]) and np.array_equal(h["ref_seg_map"], heat) and json.loads(str(h["test_cfg"])) == cfg
    if name in DENSE_FIXTURES:
        assert g["ref_noise_max"].shape == (T,) and g["share_over"].shape == (T,)
        assert np.all(g["share_over"] == 0)                      # the reference's own f32-vs-f64 difference stays inside atol(f) everywhere
        M = float(np.abs(heat).max())
        assert np.all(g["ref_noise_max"][1:] <= 2 * 1e-3 * np.arange(1, T) * M)
    else:
        assert "ref_noise_max" not in g and "share_over" not in g     # the genuine local operator does not run in float64 (generator's docstring)
    if "jhmdb" in name:
        off = int(np.where(~heat.reshape(K, -1).any(1))[0][0])
        assert not g["maps"][:, off].any() and not g["maps0"][off].any()


def test_frame0_kernels_execute_one_rounding_sequence(tmp_path):
    """Frame 0 of the map read-out must be bit-identical to what the coordinate read-out scans.  Both call padded_bilinear, whose
    rounding sequence is written out (contraction off, explicit fma); this checks the compiled code: per map dtype, the two frame-0
    kernels hold the same floating-point operations of that dtype -- fused multiply-adds, multiplies and (f32) adds / subtracts, packed
    forms counted twice.  The band kernel's own f64 sums (the map's sum, in f64 for both dtypes) are not part of the value."""
    import re
    import subprocess
    from fgvc_amd import build as b
    asm = tmp_path / "seg.s"
    r = subprocess.run([b._hipcc(), *b.FLAGS, "-S", "--cuda-device-only", "-o", str(asm), os.path.join(b.CSRC, "seg.hip")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()

    def ops_of(kernel, ty):
        m = re.search(r"^(_ZN4fgvc\d+%s[^:\n]*):[^\n]*\n(.*?)^\.Lfunc_end" % kernel, text, re.S | re.M)
        assert m, kernel
        count = {"fma": 0, "mul": 0, "addsub": 0}
        for pk, op in re.findall(r"^\s+v_(pk_)?(fma|fmac|mac|mul|add|sub)_%s\b" % ty, m.group(2), re.M):
            count["fma" if op in ("fma", "fmac", "mac") else "mul" if op == "mul" else "addsub"] += 2 if pk else 1
        return count

    for T, ty in (("f", "f32"), ("d", "f64")):
        band, maps = ops_of("heatmap_band0_kernelI%sEE" % T, ty), ops_of("softmap0_kernelI%sEE" % T, ty)
        assert band["fma"] == maps["fma"] and band["mul"] == maps["mul"] and band["fma"] >= 5, (T, band, maps)
        if ty == "f32":                                   # (f64 adds also serve the band kernel's sum of the map)
            assert band["addsub"] == maps["addsub"], (band, maps)
