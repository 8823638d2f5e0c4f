"""Host tests of the heat-map path (soft first-frame labels read out as joint coordinates): the tracker's dispatch and refusals, the
JHMDB / BADJA heat-map adapters on synthetic files with the draw_label_map / INTER_LINEAR restatements, and the new kernels' code-object
notes and exports.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tracker(**test_cfg):
    import fgvc_amd.mmpt_api as api
    m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                   pool_type="none")), test_cfg=dict(test_cfg))
    return m.eval()


def test_heatmap_dispatch_and_refusals():
    imgs = torch.zeros(1, 1, 3, 3, 16, 16)
    meta = [dict(original_shape=(16, 16))]
    heat = torch.zeros(1, 2, 16, 16)
    seg = torch.zeros(1, 16, 16, dtype=torch.long)
    m = _tracker(coords=True)
    # 4-D + coords now reaches the GPU-only rule (CPU tensors), in both dtypes
    for dt in (torch.float32, torch.float64):
        with pytest.raises(RuntimeError, match="GPU only"):
            m(test_mode=True, imgs=imgs, ref_seg_map=heat.to(dt), img_meta=meta)
    # the refusals that stay
    with pytest.raises(NotImplementedError, match="query points"):
        _tracker()(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)                # 4-D without coords
    with pytest.raises(NotImplementedError, match="query points"):
        m(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)                           # coords with an index map
    with pytest.raises(NotImplementedError, match="hard_prop"):
        _tracker(coords=True, hard_prop=True)(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
    with pytest.raises(NotImplementedError, match="save_np"):
        _tracker(coords=True, save_np=True)(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
    with pytest.raises(NotImplementedError, match="batch size 1"):
        m(test_mode=True, imgs=imgs.repeat(2, 1, 1, 1, 1, 1), ref_seg_map=heat.repeat(2, 1, 1, 1), img_meta=meta * 2)
    with pytest.raises(NotImplementedError, match="batch size 1"):
        m(test_mode=True, imgs=imgs.repeat(1, 2, 1, 1, 1, 1), ref_seg_map=heat, img_meta=meta)
    with pytest.raises(TypeError, match="float32 or float64"):
        m(test_mode=True, imgs=imgs, ref_seg_map=heat.half(), img_meta=meta)
    with pytest.raises(NotImplementedError, match="256 joints"):
        m(test_mode=True, imgs=imgs, ref_seg_map=torch.zeros(1, 257, 16, 16), img_meta=meta)


def test_draw_label_map_restatement_edge_cases():
    from fgvc_amd.datasets import draw_label_map
    s = 4
    img = np.zeros((40, 50))
    draw_label_map(img, (20.7, 10.2), s)                    # int() truncates: the patch's corner is (8, -1) -> clipped at the top,
    assert img.max() == 1.0 and img[11, 20] == 1.0          # and its centre lands on row 11 (floor would give row 10)
    assert np.argwhere(img > 0).min(0).tolist() == [0, 8] and np.argwhere(img > 0).max(0).tolist() == [22, 32]
    # assigned, not max-combined: a second joint's patch overwrites the first where they overlap
    img2 = np.zeros((40, 50))
    draw_label_map(img2, (20.0, 20.0), s)
    draw_label_map(img2, (26.0, 20.0), s)
    assert img2[20, 20] == pytest.approx(np.exp(-36 / 32))  # the second patch's value, below the first's 1.0
    # truncation toward zero: x = -0.5 gives int(-12.5) = -12, one column fewer than floor would give
    img3 = np.zeros((40, 50))
    draw_label_map(img3, (-0.5, 20.0), s)
    assert np.argwhere(img3 > 0)[:, 1].max() == 11
    # off the frame: a zero map
    for pt in ((-13.5, 20.0), (80.0, 20.0), (20.0, -14.0), (20.0, 60.0)):
        z = np.zeros((40, 50))
        draw_label_map(z, pt, s)
        assert not z.any(), pt
    # BADJA's (y, x) order is the same drawing with the point reversed; sigma 3 gives a 19 x 19 patch
    b = np.zeros((30, 30))
    draw_label_map(b, (15.0, 12.0), 3)
    assert np.argwhere(b > 0).min(0).tolist() == [3, 6] and np.argwhere(b > 0).max(0).tolist() == [21, 24]


def test_cv2_linear_restatement():
    from fgvc_amd.datasets import cv2_resize_linear, _cv2_linear_taps
    rng = np.random.default_rng(0)
    a = rng.random((6, 8, 3))
    assert np.array_equal(cv2_resize_linear(a, (6, 8)), a)                       # same size: a copy
    # 2x upsample: interior samples at (d + 0.5) / 2 - 0.5 -> weights 0.25 / 0.75, the borders clamp to the edge pixels
    s0, s1, w0, w1 = _cv2_linear_taps(4, 8)
    assert s0.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and s1.tolist() == [1, 1, 1, 2, 2, 3, 3, 3]
    assert w1.tolist() == [0.0, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.0]
    up = cv2_resize_linear(a, (12, 16))
    assert up.shape == (12, 16, 3) and up.dtype == np.float64
    np.testing.assert_allclose(up[0, 0], a[0, 0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(up[-1, -1], a[-1, -1], rtol=0, atol=1e-15)
    # away from the borders it is the half-pixel bilinear of torch.nn.functional.interpolate, up to the float weights
    want = torch.nn.functional.interpolate(torch.from_numpy(a).permute(2, 0, 1)[None], size=(12, 16), mode="bilinear",
                                           align_corners=False)[0].permute(1, 2, 0).numpy()
    np.testing.assert_allclose(up, want, rtol=0, atol=1e-7)


def test_jhmdb_heatmap_adapter(tmp_path):
    from fgvc_amd.datasets import JhmdbPoses, draw_label_map, cv2_resize_linear
    _tool("make_fake_poses").make_jhmdb(str(tmp_path), videos=2, frames=4, size=(60, 80), seed=1)
    pts = JhmdbPoses(str(tmp_path), input_size=(64, 64))
    ds = JhmdbPoses(str(tmp_path), input_size=(64, 64), form="heatmap")
    assert len(ds) == 2
    data, meta = ds[1]
    assert data["imgs"].shape == (1, 1, 3, 4, 64, 64) and data["imgs"].dtype == torch.float32
    heat = data["ref_seg_map"]
    assert heat.shape == (1, 15, 64, 64) and heat.dtype == torch.float64
    assert data["img_meta"][0]["original_shape"] == (60, 80) and meta["original_shape"] == (60, 80)
    # the map = draw_label_map (sigma 4) at the video's resolution, then the INTER_LINEAR restatement to the network size
    j = meta["gt_poses"][:, 3, 0]                                            # (x, y), 0-based
    m = np.zeros((60, 80))
    draw_label_map(m, j, 4)
    np.testing.assert_array_equal(heat[0, 3].numpy(), cv2_resize_linear(m[..., None], (64, 64))[..., 0])
    # the points form is unchanged: same frames, the joints as query points
    p_data, p_meta = pts[1]
    assert set(p_data) == {"rgbs", "query_points", "trajectories", "visibilities"}
    assert torch.equal(p_data["rgbs"].permute(0, 2, 1, 3, 4).unsqueeze(1), data["imgs"])
    np.testing.assert_array_equal(p_meta["gt_poses"], meta["gt_poses"])
    with pytest.raises(ValueError):
        JhmdbPoses(str(tmp_path), form="maps")


def test_badja_heatmap_adapter(tmp_path):
    from fgvc_amd.datasets import BadjaPoses, draw_label_map, cv2_resize_linear
    _tool("make_fake_poses").make_badja(str(tmp_path), videos=1, frames=5, size=(64, 96), seed=2)
    ds = BadjaPoses(str(tmp_path), size=(32, 48), form="heatmap")
    data, meta = ds[0]
    heat = data["ref_seg_map"]
    assert heat.shape == (1, 20, 32, 48) and heat.dtype == torch.float64
    assert data["img_meta"][0]["original_shape"] == (32, 48)                 # `size`, not the video's own
    yx = meta["joints"][0][5]                                                # (y, x) at the network size
    m = np.zeros((16, 24))
    draw_label_map(m, (yx[1] / 2, yx[0] / 2), 3)                              # half-size canvas, sigma 3
    np.testing.assert_array_equal(heat[0, 5].numpy(), cv2_resize_linear(m[..., None], (32, 48))[..., 0])
    assert BadjaPoses(str(tmp_path), size=(32, 48)).form == "points"


def test_heatmap_evaluate_feeds_pck(tmp_path):
    """The evaluate functions hand the API's (2, K, T) arrays to the PCK functions as they are: an oracle model that returns the ground
    truth scores 100."""
    from fgvc_amd import datasets
    _tool("make_fake_poses").make_jhmdb(str(tmp_path / "j"), videos=2, frames=4, size=(60, 80), seed=1)
    ds = datasets.JhmdbPoses(str(tmp_path / "j"), input_size=(64, 64), form="heatmap")
    gts = [ds[i][1]["gt_poses"] for i in range(len(ds))]
    it = iter(gts)
    pck = datasets.jhmdb_evaluate_heatmap(lambda test_mode, **d: [next(it)], ds)
    assert pck["PCK@0.1"] == pytest.approx(100.0)
    _tool("make_fake_poses").make_badja(str(tmp_path / "b"), videos=1, frames=5, size=(64, 96), seed=2)
    bd = datasets.BadjaPoses(str(tmp_path / "b"), size=(32, 48), form="heatmap")
    _, meta = bd[0]
    T = len(meta["joints"])
    pred = np.zeros((2, 20, T))
    for t, j in enumerate(meta["joints"]):
        if j is not None:
            pred[:, :, t] = j[:, ::-1].T
    pck = datasets.badja_evaluate_heatmap(lambda test_mode, **d: [pred], bd)
    assert pck["PCK@0.1"] == pytest.approx(100.0)


def test_heatmap_kernels_use_no_scratch():
    kn = _tool("kernel_notes")
    notes = kn.kernel_notes()
    for fam, want in (("seg_soft_labels_kernel", 2), ("heatmap_band_kernel", 2), ("heatmap_band0_kernel", 2), ("heatmap_merge_kernel", 1)):
        ks = {k: v for k, v in notes.items() if fam in k}
        assert len(ks) == want, (fam, sorted(ks))
        for k, v in ks.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)


def test_heatmap_exports_declared():
    from fgvc_amd import _lib
    lib = _lib.load()
    for name in ("fgvc_seg_soft_labels_f32", "fgvc_seg_soft_labels_f64", "fgvc_heatmap_coords_workspace_bytes", "fgvc_heatmap_coords_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.fgvc_heatmap_coords_f32(None, None, 0, 2, 4, 4, 2, 8, 8, 8, 8, 0, 0, 8, 8, 0, None, None, None) == _lib.ERR_INVALID_ARG
    assert b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_seg_soft_labels_f64(None, 2, 8, 8, 8, 8, 0, 0, 4, 4, None, None) == _lib.ERR_INVALID_ARG
    assert lib.fgvc_heatmap_coords_workspace_bytes(8, 15) == 8 * 15 * 8 * (5 * 8 + 5 * 4 + 8)
