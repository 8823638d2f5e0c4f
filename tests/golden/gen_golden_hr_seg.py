"""Record the fixtures of HRVanillaTracker's label-map path from the reference, executed read-only in place (never copied).

    python tests/golden/gen_golden_hr_seg.py          # writes tests/golden/hr_seg_*.npz, hr_heatmap_*.npz

The genuine HRVanillaTracker.forward_test_backward_save_mem (vanilla_tracker.py:663-830) with its own affinity, the genuine
masked_attention_efficient_correlation (local_attention.py:883-1006: Correlation + part_unfold + top-k over K*(2R+1)^2), on CPU under
oracle/ref_import.py.  Nothing in the tracker is swapped; the two stand-ins are outside it:
  - mmcv.ops.Correlation is ref_import's stand-in (the published semantics: zero padded, sum over channels);
  - mmcv.imresize(..., interpolation='nearest', backend='pillow') is Pillow's resize (what mmcv calls on that backend).
The tracker keeps its constructor's `stride` (2) as the pad unit.  test_cfg.sstep is large (the reference reads the key; it only chunks
the queries).  Frames are float16-rounded and stored as such.  Masks: the top-two gap of the normalised values the reference's argmax saw
(f32, spied), which says which pixels are decidable.  Heat maps: each clip runs twice (coords=True: the recorded coordinates; coords=False:
the maps), gap = (5th - 6th largest) / max per (frame, joint).
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

BASE = dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=8, sstep=1 << 20, with_first=True)


def _setup():
    from PIL import Image
    from oracle import ref_import
    ref = ref_import.load()
    mmcv = sys.modules["mmcv"]

    def imresize(img, size, interpolation="bilinear", backend=None, **_):
        assert interpolation == "nearest" and backend == "pillow", (interpolation, backend)
        return np.asarray(Image.fromarray(img).resize(tuple(size), Image.NEAREST))
    mmcv.imresize = imresize
    return ref, ref_import


def _model(ref, seed, strides, cfg):
    from oracle import fgvc_oracle as O
    model = ref.builder.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=strides, out_indices=(2,),
                                                                              pool_type="none")), train_cfg=None, test_cfg=ref.ConfigDict(cfg))
    model.backbone.load_state_dict(O.seeded_resnet_state(seed, strides, "none"), strict=True)
    return model.eval()


def gen_masks(name, seed, T, h, w, objects, original_shape, extra, strides=(1, 1, 1, 4), seg_edit=None):
    import torch
    from gen_golden_vos import _ArgmaxSpy, _frames
    ref, ref_import = _setup()
    cfg = {**BASE, **extra}
    model = _model(ref, seed, strides, cfg)
    imgs16, seg0 = _frames(seed, T, h, w, objects)
    if seg_edit is not None:
        seg_edit(seg0, model)
    imgs = torch.from_numpy(imgs16.astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()   # (1, 1, 3, T, h, w)
    ref_seg = torch.from_numpy(seg0).unsqueeze(0)
    with ref_import.cuda_as_cpu(), torch.no_grad(), _ArgmaxSpy(original_shape) as spy:
        out = model.forward_test_backward_save_mem(imgs, ref_seg, [dict(original_shape=tuple(original_shape))])
    assert isinstance(out, list) and len(out) == 1
    masks = np.asarray(out[0])
    assert masks.shape == (T, *original_shape) and np.array_equal(masks, masks.astype(np.uint8)), masks.shape
    assert len(spy.gaps) == T - 1, len(spy.gaps)
    save = dict(imgs=imgs16, ref_seg_map=seg0, original_shape=np.array(original_shape), seed=seed, strides=np.array(strides),
                masks=masks.astype(np.uint8), gap=np.stack(spy.gaps).astype(np.float32), test_cfg=np.array(json.dumps(cfg)))
    outp = os.path.join(HERE, name + ".npz")
    np.savez_compressed(outp, **save)
    print(outp, masks.shape, "ids", np.unique(masks).tolist(), "undecidable", int((save["gap"] <= 1e-5).sum()), "of", save["gap"].size,
          "size", os.path.getsize(outp))


def gen_heat(name, seed, T, h, w, K, map_shape, sigma, original_shape, map_dtype, extra, points=None):
    import torch
    from gen_golden_heatmap import _gap
    from gen_golden_vos import _frames
    from fgvc_amd.datasets import pose_heatmaps
    ref, ref_import = _setup()
    cfg0 = {**BASE, **extra}
    rng = np.random.default_rng(seed)
    imgs16, _ = _frames(seed, T, h, w, 2)
    mh, mw = map_shape
    if points is None:
        points = np.stack([rng.uniform(0.15 * mw, 0.85 * mw, K), rng.uniform(0.15 * mh, 0.85 * mh, K)], 1)
    heat = pose_heatmaps(points, map_shape, sigma, (h, w)).astype(map_dtype)
    outs = {}
    for coords in (True, False):
        model = _model(ref, seed, (1, 1, 1, 4), {**cfg0, "coords": coords})
        imgs = torch.from_numpy(imgs16.astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()
        with ref_import.cuda_as_cpu(), torch.no_grad():
            out = model.forward_test_backward_save_mem(imgs, torch.from_numpy(heat).unsqueeze(0), [dict(original_shape=tuple(original_shape))])
        assert isinstance(out, list) and len(out) == 1
        outs[coords] = np.asarray(out[0])
    coords, maps = outs[True], outs[False]
    assert coords.shape == (2, K, T) and coords.dtype == np.float64, (coords.shape, coords.dtype)
    assert maps.shape == (T, K, *original_shape), maps.shape
    assert np.array_equal(model.img2coord(maps, num_poses=K), coords)
    gap = _gap(maps)
    save = dict(imgs=imgs16, ref_seg_map=heat, original_shape=np.array(original_shape), seed=seed, coords=coords, gap=gap.astype(np.float64),
                test_cfg=np.array(json.dumps(cfg0)))
    outp = os.path.join(HERE, name + ".npz")
    np.savez_compressed(outp, **save)
    print(outp, "unclear maps", int((gap <= 1e-5).sum()), "of", gap.size, "size", os.path.getsize(outp))


def _vanish(seg, model):
    """An id on one pixel that Pillow's nearest sampling to the feature grid never reads (padded 42 x 48 -> 11 x 12 under the stride-4
    encoder; the tracker's stride 2 pads 41 x 47 at the bottom and right only, so padded and unpadded coordinates agree)."""
    from fgvc_amd import ops
    rows = set(ops.pil_nearest_index(42, 11).tolist())
    cols = set(ops.pil_nearest_index(48, 12).tolist())
    y = next(r for r in range(15, 41) if r not in rows)
    x = next(c for c in range(15, 47) if c not in cols)
    seg[y, x] = seg.max() + 1


def main():
    gen_masks("hr_seg_8x62x70", 41, 8, 62, 70, 3, (62, 70), {})
    gen_masks("hr_seg_hard_8x62x70", 41, 8, 62, 70, 3, (62, 70), dict(hard_prop=True))
    gen_masks("hr_seg_vanish_5x41x47", 43, 5, 41, 47, 2, (45, 52), dict(precede_frames=3), strides=(1, 2, 1, 1), seg_edit=_vanish)
    gen_masks("hr_seg_nonorm_5x62x70", 44, 5, 62, 70, 3, (62, 70), dict(precede_frames=3, with_norm=False, temperature=200.0))
    rng = np.random.default_rng(5)
    K = 15
    pts = np.stack([rng.uniform(6, 34, K), rng.uniform(5, 25, K)], 1)       # (x, y) on a 30 x 40 video
    pts[4] = (-40.0, 12.0)                                                    # a joint off the frame: a zero map, -1 throughout
    gen_heat("hr_heatmap_jhmdb_6x48x64", 51, 6, 48, 64, K, (30, 40), 4, (30, 40), np.float64, {}, points=pts)
    gen_heat("hr_heatmap_pad_5x41x47", 53, 5, 41, 47, 6, (41, 47), 3, (45, 52), np.float32, dict(precede_frames=3))


if __name__ == "__main__":
    main()
