"""Host tests of the segmentation-mask path (semi-supervised VOS): the Pillow-nearest rule the label kernels use, the J&F metric,
the DAVIS-2017 adapter, the config keys and refusals of the mask path, and the new kernels' code-object notes.  No GPU."""
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


def test_pil_nearest_rule_matches_pillow():
    """ops.pil_nearest_index (the rule fgvc_seg_*_u8 evaluate) against Pillow's own NEAREST resize, including non-integer ratios,
    up-sampling and the sizes where floor((o + 0.5) * in / out) is off by one (100 -> 27)."""
    from PIL import Image
    from fgvc_amd import ops
    rng = np.random.default_rng(0)
    sizes = [(100, 27), (64, 16), (62, 31), (854, 427), (480, 240), (7, 3), (10, 40), (5, 1), (481, 241)]
    sizes += [tuple(int(v) for v in rng.integers(1, 400, 2)) for _ in range(200)]
    for n_in, n_out in sizes:
        a = np.arange(n_in, dtype=np.int32)[None, :].repeat(2, 0)
        want = np.asarray(Image.fromarray(a).resize((n_out, 2), Image.NEAREST))[0]
        assert np.array_equal(ops.pil_nearest_index(n_in, n_out).numpy(), want), (n_in, n_out)
    # the naive closed form is NOT Pillow's rule
    assert (((2 * 13 + 1) * 100) // (2 * 27)) != int(ops.pil_nearest_index(100, 27)[13])


def test_pad_divide_by_sizes():
    from fgvc_amd import engine
    assert engine.pad_divide_by(62, 70, 4) == ((64, 72), (1, 1, 1, 1))
    assert engine.pad_divide_by(61, 75, 4) == ((64, 76), (0, 1, 1, 2))
    assert engine.pad_divide_by(480, 854, 2) == ((480, 854), (0, 0, 0, 0))
    x = torch.zeros(1, 61, 75)
    (hp, wp), pad = engine.pad_divide_by(61, 75, 4)
    y = torch.nn.functional.pad(x, pad)
    assert y.shape[-2:] == (hp, wp)


def test_jf_metric_known_answers():
    from fgvc_amd import metrics
    a = np.zeros((40, 50), bool)
    a[10:30, 10:30] = True
    b = np.zeros_like(a)
    b[10:30, 20:40] = True
    assert metrics.db_eval_iou(a, b) == pytest.approx(200 / 600)
    assert metrics.db_eval_iou(a, a) == 1.0 and metrics.db_eval_iou(~a & False, a & False) == 1.0
    assert metrics.f_measure(a, a) == 1.0
    f = metrics.f_measure(b, a)
    assert 0.0 < f < 1.0
    # empty prediction against a non-empty annotation: precision 1, recall 0
    assert metrics.f_measure(np.zeros_like(a), a) == 0.0
    # boundary map: a 20 x 20 square has its boundary on the square's last row / column and the pixels before its first
    bm = metrics._seg2bmap(a)
    assert bm[9, 15] and bm[29, 15] and bm[15, 29] and not bm[15, 15]
    M, O, D = metrics.db_statistics(np.array([1.0, 0.9, 0.8, 0.7, 0.4, 0.3, 0.2, 0.1]))
    assert M == pytest.approx(0.55) and O == pytest.approx(0.5)
    assert D == pytest.approx(np.mean([1.0, 0.9, 0.8]) - np.mean([0.3, 0.2, 0.1]))      # bins [0:3] and [5:8]
    gt = np.stack([a, a, a])[None]
    r = metrics.JFM(gt, gt, 1)
    assert r["JM"] == [1.0] and r["FM"] == [1.0]


def test_jf_boundary_dilation_is_a_disk():
    """A boundary displaced by exactly the tolerance (ceil(0.008 * diagonal) pixels) still matches; one pixel further does not."""
    from fgvc_amd import metrics
    h, w = 120, 160
    r = int(np.ceil(0.008 * np.hypot(h, w)))
    a = np.zeros((h, w), bool)
    a[40:80, 40:100] = True
    b = np.zeros_like(a)
    b[40:80, 40 + r:100 + r] = True
    c = np.zeros_like(a)
    c[40:80, 40 + r + 1:100 + r + 1] = True
    # the vertical edges move by r (within the disk); the horizontal ones overlap except at the ends
    fb, fc = metrics.f_measure(b, a), metrics.f_measure(c, a)
    assert fb > fc


def test_davis_adapter_reads_the_layout(tmp_path):
    from fgvc_amd.datasets import Davis2017
    mk = _tool("make_fake_davis")
    names = mk.make(str(tmp_path), sequences=2, frames=5, size=(48, 64), objects=3, seed=2)
    ds = Davis2017(str(tmp_path))
    assert len(ds) == 2 and ds.sequences == names
    data, meta = ds[1]
    assert data["imgs"].shape == (1, 1, 3, 5, 48, 64) and data["imgs"].dtype == torch.float32
    assert data["ref_seg_map"].shape == (1, 48, 64) and data["ref_seg_map"].dtype == torch.uint8
    assert data["img_meta"][0]["original_shape"] == (48, 64)
    assert meta["gt"].shape == (5, 48, 64) and meta["n_objects"] == 3
    assert set(np.unique(meta["gt"])) <= {0, 1, 2, 3}
    # palette PNG: the stored indices are the ids
    from PIL import Image
    im = Image.open(os.path.join(str(tmp_path), "Annotations", "480p", names[1], "00000.png"))
    assert im.mode == "P" and np.array_equal(np.asarray(im), meta["gt"][0])
    # Lab + Normalize contract: L channel (x - 50) / 50 within [-1, 1]
    L = data["imgs"][0, 0, 0]
    assert float(L.min()) >= -1.0 - 1e-5 and float(L.max()) <= 1.0 + 1e-5


def _tracker(**test_cfg):
    import fgvc_amd.mmpt_api as api
    m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                   pool_type="none")), test_cfg=dict(test_cfg))
    return m.eval()


def test_mask_path_config_keys_and_refusals():
    from fgvc_amd import engine
    from fgvc_amd.mmpt_api.config import ConfigDict
    cfg = engine.TrackerConfig.from_test_cfg(ConfigDict(dict(hard_prop=True, norm_mask=False)))
    assert cfg.hard_prop is True and cfg.norm_mask is False
    cfg = engine.TrackerConfig.from_test_cfg(ConfigDict(dict()))
    assert cfg.hard_prop is False and cfg.norm_mask is True
    assert _tracker(hard_prop=True).engine_config().hard_prop is True
    m = _tracker()
    assert m.output_stride() == 2
    imgs = torch.zeros(1, 1, 3, 3, 16, 16)
    meta = [dict(original_shape=(16, 16))]
    seg = torch.zeros(1, 16, 16, dtype=torch.long)
    with pytest.raises(NotImplementedError, match="query points"):
        m(test_mode=True, imgs=imgs, ref_seg_map=torch.zeros(1, 2, 16, 16), img_meta=meta)       # 4-D soft labels
    with pytest.raises(NotImplementedError, match="query points"):
        _tracker(coords=True)(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
    with pytest.raises(NotImplementedError, match="save_np"):
        _tracker(save_np=True)(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
    with pytest.raises(NotImplementedError, match="batch size 1"):
        m(test_mode=True, imgs=imgs.repeat(2, 1, 1, 1, 1, 1), ref_seg_map=seg.repeat(2, 1, 1), img_meta=meta * 2)
    with pytest.raises(NotImplementedError, match="batch size 1"):                                  # two clips per sample
        m(test_mode=True, imgs=imgs.repeat(1, 2, 1, 1, 1, 1), ref_seg_map=seg, img_meta=meta)
    big = seg.clone()
    big[0, 3, 3] = 256
    with pytest.raises(NotImplementedError, match="255"):
        m(test_mode=True, imgs=imgs, ref_seg_map=big, img_meta=meta)
    # past the refusals a CPU tensor meets the GPU-only rule, as on the points path
    with pytest.raises(RuntimeError, match="GPU only"):
        m(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(test_mode=True, rgbs=torch.zeros(1, 3, 3, 16, 16), query_points=torch.zeros(1, 1, 3), trajectories=torch.zeros(1, 3, 1, 2),
          visibilities=torch.zeros(1, 3, 1))


def test_mask_kernels_use_no_scratch():
    """The segmentation kernels in the code-object notes of the built library: no scratch memory, no spilled register."""
    kn = _tool("kernel_notes")
    notes = kn.kernel_notes()
    for fam, want in (("seg_max_label_kernel", 1), ("seg_onehot_kernel", 1), ("seg_hard_onehot_kernel", 1), ("seg_minmax_kernel", 2),
                      ("seg_argmax_kernel", 2)):
        ks = {k: v for k, v in notes.items() if fam in k}
        assert len(ks) == want, (fam, sorted(ks))
        for k, v in ks.items():
            assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0, (k, v)


def test_mask_exports_declared():
    from fgvc_amd import _lib
    lib = _lib.load()
    for name in ("fgvc_seg_max_label_u8", "fgvc_seg_onehot_labels_u8", "fgvc_seg_hard_onehot_f32", "fgvc_seg_readout_workspace_bytes",
                 "fgvc_seg_readout_u8"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.fgvc_seg_readout_u8(None, 1, 4, 4, 2, 8, 8, 0, 0, 8, 8, 8, 8, 1, None, None, None) == _lib.ERR_INVALID_ARG
    assert b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_seg_readout_workspace_bytes(8, 11) == 8 * 32 * 11 * 2 * 4


def test_jf_matches_reference_fixture():
    """tests/golden/vos_jf.npz: the reference's db_eval_iou / db_eval_boundary / JFM on 3 objects x 9 frames (pinned under the
    stand-ins gen_golden_vos.py names: scipy dilation for cv2.dilate, the x^2 + y^2 <= r^2 disk for skimage's)."""
    from fgvc_amd import metrics
    g = np.load(os.path.join(ROOT, "tests", "golden", "vos_jf.npz"))
    gt, pr = g["gt"], g["pred"]
    for o in range(gt.shape[0]):
        np.testing.assert_allclose(metrics.db_eval_iou(gt[o], pr[o]), g[f"iou_{o}"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(metrics.db_eval_boundary(gt[o], pr[o]), g[f"f_{o}"], rtol=0, atol=1e-12)
    r = metrics.JFM(gt, pr, gt.shape[0])
    for k in ("JM", "JR", "JD", "FM", "FR", "FD"):
        np.testing.assert_allclose(np.asarray(r[k]), g["JFM_" + k], rtol=0, atol=1e-12)
