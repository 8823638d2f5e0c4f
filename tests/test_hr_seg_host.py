"""Host tests of HRVanillaTracker's label-map path (vanilla_tracker.py:663-830 on its own local-window affinity): dispatch and refusals,
the config keys as the reference reads them, the pad unit, the clip plan (key slots, duplicates, chunks under the pair-list budget), the
v1 operator's export, and the new merge kernel's code-object notes.  No GPU."""
import importlib.util
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


CFG = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8)


def _hr(strides=(1, 1, 1, 4), model_kw=None, **test_cfg):
    import fgvc_amd.mmpt_api as api
    m = api.build_model(dict(type="HRVanillaTracker", **(model_kw or {}), backbone=dict(type="ResNet", depth=18, strides=strides, out_indices=(2,),
                                                                     pool_type="none")), test_cfg=dict(test_cfg))
    return m.eval()


def test_dispatch_and_refusals():
    m = _hr(**CFG)
    imgs = torch.zeros(1, 1, 3, 3, 16, 16)
    meta = [dict(original_shape=(16, 16))]
    seg = torch.zeros(1, 16, 16, dtype=torch.long)
    heat = torch.zeros(1, 2, 16, 16)
    with pytest.raises(NotImplementedError, match="query points"):
        m(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)                           # 4-D without coords
    with pytest.raises(NotImplementedError, match="query points"):
        _hr(coords=True, **CFG)(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)      # coords with an index map
    with pytest.raises(NotImplementedError, match="save_np"):
        _hr(save_np=True, **CFG)(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
    with pytest.raises(NotImplementedError, match="batch size 1"):
        m(test_mode=True, imgs=imgs.repeat(2, 1, 1, 1, 1, 1), ref_seg_map=seg.repeat(2, 1, 1), img_meta=meta * 2)
    with pytest.raises(NotImplementedError, match="batch size 1"):
        m(test_mode=True, imgs=imgs.repeat(1, 2, 1, 1, 1, 1), ref_seg_map=seg, img_meta=meta)
    big = seg.clone()
    big[0, 3, 3] = 256
    with pytest.raises(NotImplementedError, match="255"):
        m(test_mode=True, imgs=imgs, ref_seg_map=big, img_meta=meta)
    with pytest.raises(RuntimeError, match="GPU only"):
        m(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
    hc = _hr(coords=True, **CFG)
    with pytest.raises(NotImplementedError, match="hard_prop"):
        _hr(coords=True, hard_prop=True, **CFG)(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
    with pytest.raises(TypeError, match="float32 or float64"):
        hc(test_mode=True, imgs=imgs, ref_seg_map=heat.to(torch.float16), img_meta=meta)
    with pytest.raises(NotImplementedError, match="1 to 256 joints"):
        hc(test_mode=True, imgs=imgs, ref_seg_map=torch.zeros(1, 257, 16, 16), img_meta=meta)
    with pytest.raises(RuntimeError, match="GPU only"):
        hc(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
    # points and label maps in one call: refused; the points signature still takes its four tensors positionally
    with pytest.raises(TypeError):
        m(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta, rgbs=torch.zeros(1, 3, 3, 16, 16),
          query_points=torch.zeros(1, 1, 3))
    with pytest.raises(TypeError, match="missing rgbs"):
        m(test_mode=True, trajectories=torch.zeros(1, 3, 1, 2))
    assert list(inspect.signature(type(m).forward_test).parameters)[1:5] == ["rgbs", "query_points", "trajectories", "visibilities"]


def test_config_keys_as_the_reference_reads_them():
    m = _hr(withnorm=False, neighbor_range=30, sstep=7, tstep=2, step=3, mask_mode="square", with_first_neighbor=False,
            **{k: v for k, v in CFG.items() if k != "neighbor_range"})
    c = m._label_config()
    assert c.with_norm is True                      # `withnorm` (the points path's key) does not reach the label maps
    assert c.radius == 15 and c.window == 31 and c.mask.ry == c.mask.rx == 15 and c.mask.is_none is False
    assert (c.temperature, c.topk, c.precede_frames, c.with_first) == (0.07, 10, 3, True)
    assert c.hard_prop is False and c.norm_mask is True and c.pair_precision == "auto"
    assert _hr(with_norm=False, **CFG)._label_config().with_norm is False
    assert _hr(with_first=False, hard_prop=True, norm_mask=False, **CFG)._label_config().with_first is False
    assert _hr(**{k: v for k, v in CFG.items() if k != "neighbor_range"})._label_config().radius == 12    # constructor default 24 // 2
    for key in ("temperature", "topk", "precede_frames"):                  # attributes with no default (:728, :754-755)
        mk = _hr(**{k: v for k, v in CFG.items() if k != key})
        with pytest.raises(AttributeError, match=key):
            mk._label_config()
    with pytest.raises(AttributeError, match="temperature"):              # ... read before anything else on the heat-map path
        _hr(coords=True, precede_frames=3, topk=10)(test_mode=True, imgs=torch.zeros(1, 1, 3, 3, 16, 16), ref_seg_map=torch.zeros(1, 2, 16, 16),
                                                     img_meta=[dict(original_shape=(16, 16))])


def test_pad_unit_is_the_trackers_stride():
    """vanilla_tracker.py:671-672 pads by self.stride (constructor default 2), not by the encoder's output stride: under a stride-4
    encoder a 41 x 47 frame pads to 42 x 48 and the feature grid (11 x 12) is whatever the encoder makes of it -- not 42 / 4 x 48 / 4."""
    from fgvc_amd import engine
    m = _hr(strides=(1, 2, 1, 1), **CFG)
    assert m.stride == 2 and m.output_stride() == 4
    (hp, wp), pad = engine.pad_divide_by(41, 47, m.stride)
    assert (hp, wp) == (42, 48) and pad == (0, 1, 0, 1)
    with torch.no_grad():
        f = m.backbone(torch.zeros(1, 3, hp, wp))
    f = f[0] if isinstance(f, (list, tuple)) else f
    assert tuple(f.shape[-2:]) == (11, 12) and (11 * 4, 12 * 4) != (hp, wp)
    assert engine.pad_divide_by(45, 52, 2) == ((46, 52), (0, 0, 0, 1))
    assert _hr(model_kw=dict(stride=4), **CFG).stride == 4


def test_local_plan_slots_duplicates_and_chunks():
    from fgvc_amd import engine
    cfg = engine.LocalConfig(temperature=0.07, topk=10, precede_frames=5)
    plan = engine.plan_local_clip(8, cfg, 240 * 427)
    assert plan.pair_bytes == 240 * 427 * 10 * 8                              # 8.2 MB per pair at 480 x 854
    assert plan.slot_frame[0][:2] == [0, 0] and plan.slot_pair[0][:2] == [0, 0] and plan.slot_pair[0][2:] == [-1] * 4
    assert plan.slot_frame[6] == [0, 2, 3, 4, 5, 6]                           # key_start = f - precede_frames, then frame 0 first
    assert len(plan.pairs) == 27 and plan.t_max == 6 and plan.chunks == [(0, 7, 0, 27)]
    for r, row in enumerate(plan.slot_pair):                                  # every slot names the pair of (its row's frame, its key frame)
        for j, p in enumerate(row):
            if p >= 0:
                assert plan.pairs[p] == (r + 1, plan.slot_frame[r][j])
    cfg.pair_budget = 12 * plan.pair_bytes
    small = engine.plan_local_clip(8, cfg, 240 * 427)
    assert small.chunks[0][0] == 0 and small.chunks[-1][1] == 7 and len(small.chunks) > 2
    for (r0, r1, p0, p1), nxt in zip(small.chunks, small.chunks[1:] + [None]):
        assert (p1 - p0) * small.pair_bytes <= cfg.pair_budget
        if nxt is not None:
            assert nxt[0] == r1 and nxt[2] == p1
    assert small.pairs == plan.pairs and small.slot_pair == plan.slot_pair
    cfg.pair_budget = 5 * plan.pair_bytes
    with pytest.raises(ValueError, match="pair_budget"):
        engine.plan_local_clip(8, cfg, 240 * 427)
    nf = engine.plan_local_clip(4, engine.LocalConfig(temperature=1.0, topk=5, precede_frames=2, with_first=False), 100)
    assert nf.slot_frame == [[0, 0], [0, 1], [1, 2]] and nf.slot_pair == [[0, -1], [1, 2], [3, 4]]


def test_v1_operator_exported_with_the_reference_signature():
    from fgvc_amd.mmpt_api import common
    assert "masked_attention_efficient_correlation" in common.__all__
    params = list(inspect.signature(common.masked_attention_efficient_correlation).parameters)
    assert params == ["query_frame", "key_frames", "value", "radius", "corr_infer", "feat_extractor", "temperature", "topk", "normalize",
                      "sstep", "tstep"]


def test_merge_plan_exported_and_scratch_free():
    from fgvc_amd import _lib
    assert hasattr(_lib.load(), "fgvc_local_merge_plan_f32")
    kn = _tool("kernel_notes")
    notes = kn.kernel_notes()
    ks = {k: v for k, v in notes.items() if "local_merge_plan_kernel" in k}
    assert len(ks) == 4, sorted(ks)
    for k, v in ks.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
