"""Record the fixtures of the heat-map path (soft first-frame labels, coords=True) from the reference, executed read-only in place.

    python tests/golden/gen_golden_heatmap.py          # writes tests/golden/heatmap_*.npz

The genuine HRVanillaTracker.forward_test_backward_save_mem (vanilla_tracker.py:663-830) on CPU under oracle/ref_import.py, with the
replacements gen_golden_vos.py names (VanillaTracker's affinity through the genuine masked_attention_efficient, self.stride = 2).  Each
clip runs twice: with coords=True (the recorded coordinates) and with coords=False (the full maps).  From the maps: per (frame, joint)
the gap (5th - 6th largest) / max, which says where the top 5 is decidable, and a check that the reference's own img2coord of them is
the coords=True output.  The first-frame maps are fgvc_amd.datasets.pose_heatmaps (draw_label_map + the INTER_LINEAR restatement),
stored as given to the tracker; the frames are float16-rounded and stored as such.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)


def _gap(maps: np.ndarray) -> np.ndarray:
    """maps (T, K, h0, w0) -> (T, K) (5th - 6th largest) / max (inf for a zero map)."""
    T, K = maps.shape[:2]
    s = np.sort(maps.reshape(T, K, -1).astype(np.float64), axis=-1)[..., -6:]
    mx = np.abs(s[..., -1])
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (s[..., 1] - s[..., 0]) / mx
    return np.where(mx == 0, np.inf, g)


def gen(name, seed, T, h, w, K, map_shape, sigma, original_shape, map_dtype, extra, points=None, edit=None):
    import torch
    from gen_golden_vos import _frames
    from oracle import fgvc_oracle as O
    from oracle import ref_import
    from fgvc_amd.datasets import pose_heatmaps
    ref = ref_import.load()
    vt = sys.modules["mmpt.models.trackers.vanilla_tracker"]
    cfg0 = {**dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=8, step=512, with_first=True, with_first_neighbor=True),
            **extra}

    def corr_wrapper(query_frame, key_frames, value_logits, radius=None, corr_infer=None, feat_extractor=None, temperature=1.0,
                     topk=None, sstep=None, tstep=None, normalize=True):
        def enc(x):
            f = feat_extractor(x)
            return f[0] if isinstance(f, (list, tuple)) else f
        q = enc(query_frame)
        k = torch.stack([enc(key_frames[:, :, t]) for t in range(key_frames.shape[2])], 2)
        mask = ref.spatial_neighbor(q.shape[0], *q.shape[2:], neighbor_range=cfg0["neighbor_range"], device=q.device, dtype=q.dtype,
                                    mode="circle")
        return ref.masked_attention_efficient(q, k, value_logits, mask, temperature=cfg0["temperature"], topk=cfg0["topk"],
                                              step=cfg0["step"], normalize=True, non_mask_len=0, sim_mode="dot_product")
    vt.masked_attention_efficient_correlation = corr_wrapper
    rng = np.random.default_rng(seed)
    imgs16, _ = _frames(seed, T, h, w, 2)
    mh, mw = map_shape
    if points is None:
        points = np.stack([rng.uniform(0.15 * mw, 0.85 * mw, K), rng.uniform(0.15 * mh, 0.85 * mh, K)], 1)
    heat = pose_heatmaps(points, map_shape, sigma, (h, w)).astype(map_dtype)
    if edit is not None:
        edit(heat)
    outs = {}
    for coords in (True, False):
        cfg = ref.ConfigDict({**cfg0, "coords": coords})
        model = ref.builder.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4),
                                                                                  out_indices=(2,), pool_type="none")),
                                        train_cfg=None, test_cfg=cfg)
        model.backbone.load_state_dict(O.seeded_resnet_state(seed, (1, 1, 1, 4), "none"), strict=True)
        model.eval()
        model.stride = 2
        imgs = torch.from_numpy(imgs16.astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()
        with ref_import.cuda_as_cpu(), torch.no_grad():
            out = model.forward_test_backward_save_mem(imgs, torch.from_numpy(heat).unsqueeze(0), [dict(original_shape=tuple(original_shape))])
        assert isinstance(out, list) and len(out) == 1
        outs[coords] = np.asarray(out[0])
    coords, maps = outs[True], outs[False]
    assert coords.shape == (2, K, T) and coords.dtype == np.float64, (coords.shape, coords.dtype)
    assert maps.shape == (T, K, *original_shape), maps.shape
    assert np.array_equal(model.img2coord(maps, num_poses=K), coords)      # the recorded coordinates are img2coord of the maps
    gap = _gap(maps)
    save = dict(imgs=imgs16, ref_seg_map=heat, original_shape=np.array(original_shape), seed=seed, coords=coords,
                gap=gap.astype(np.float64), maps_dtype=np.array(str(maps.dtype)), test_cfg=np.array(json.dumps(cfg0)))
    if name.startswith("heatmap_jhmdb"):
        off = np.where(~heat.reshape(K, -1).any(1))[0]
        save["off_joint"] = np.array(int(off[0]))
        assert np.all(coords[:, off[0]] == -1.0)
    outp = os.path.join(HERE, name + ".npz")
    np.savez_compressed(outp, **save)
    print(outp, "maps", maps.dtype, "unclear maps", int((gap <= 1e-5).sum()), "of", gap.size, "size", os.path.getsize(outp))


def _flat_top(heat):
    heat[1] = np.minimum(heat[1], np.float32(0.7) * heat[1].max())           # a plateau wider than 5 pixels: ties at rank 5


def main():
    rng = np.random.default_rng(5)
    K = 15
    pts = np.stack([rng.uniform(6, 34, K), rng.uniform(5, 25, K)], 1)       # (x, y) on a 30 x 40 video
    pts[4] = (-40.0, 12.0)                                                    # a joint off the frame: a zero map, -1 throughout
    gen("heatmap_jhmdb_6x48x64", 51, 6, 48, 64, K, (30, 40), 4, (30, 40), np.float64, {}, points=pts)
    gen("heatmap_badja_6x56x80", 52, 6, 56, 80, 20, (28, 40), 3, (56, 80), np.float64, dict(precede_frames=3))
    gen("heatmap_pad_5x41x47", 53, 5, 41, 47, 6, (41, 47), 3, (45, 52), np.float32, dict(precede_frames=3), edit=_flat_top)


if __name__ == "__main__":
    main()
