"""Record the fixtures of the soft-map output (soft first-frame labels WITHOUT coords: the propagated maps themselves) from the
reference, executed read-only in place.

    python tests/golden/gen_golden_softmap.py          # writes tests/golden/softmap_*.npz, hr_softmap_*.npz

The clips, seeds and set-ups are those of gen_golden_heatmap.py (dense affinity through its corr_wrapper: softmap_*) and of
gen_golden_hr_seg.py (the genuine masked_attention_efficient_correlation: hr_softmap_*), so the `coords` of those fixtures and the
`maps` of these describe the same runs.  Recorded is the reference's own coords=False return value (T, K, h0, w0): `maps0` = frame 0 in
the stack's dtype, `maps` = frames >= 1 as float32 -- np.stack widened them to the stack's dtype, and the generator asserts that widening
the stored float32 values reproduces the reference's array exactly.

Yardstick: every clip runs a second time with the model and the frames in float64 (model.double()); per frame f >= 1
`ref_noise_max[f]` = max |f32 run - f64 run| and `share_over[f]` = the share of values whose difference exceeds
atol(f) = 2 * 1e-3 * f * max|ref_seg_map| (the bound the model-call test applies).  share_over must be 0: the reference alone stays inside
the tolerance with nothing left out.  The float64 pass runs for the three dense clips only: the genuine
masked_attention_efficient_correlation cannot run in float64 (the tracker hands it the float32 label bank of :711 beside float64
features, and its product raises "expected scalar type Double but found Float"; nothing inside the tracker is swapped for these clips,
so there is no place to cast).  The two hr_softmap_* fixtures therefore carry no yardstick fields; their test uses the same derived bounds.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)

DELTA = 1e-3          # the project's score bar, logit units


def _run(model, imgs16, heat, original_shape, ref_import, double):
    import torch
    dt = torch.float64 if double else torch.float32
    if double:
        model = model.double()
    imgs = torch.from_numpy(imgs16.astype(np.float32)).to(dt).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()
    with ref_import.cuda_as_cpu(), torch.no_grad():
        out = model.forward_test_backward_save_mem(imgs, torch.from_numpy(heat).unsqueeze(0), [dict(original_shape=tuple(original_shape))])
    assert isinstance(out, list) and len(out) == 1
    return np.asarray(out[0])


def _save(name, imgs16, heat, original_shape, seed, cfg0, maps, maps64, img2coord):
    T, K = maps.shape[:2]
    # the same run as the heat-map fixture of this clip: the reference's own img2coord of these maps is that fixture's `coords`
    twin = np.load(os.path.join(HERE, name.replace("softmap", "heatmap") + ".npz"))
    assert np.array_equal(img2coord(maps, num_poses=K), twin["coords"]), name
    assert maps.shape == (T, K, *original_shape) and maps.dtype == heat.dtype, (maps.shape, maps.dtype)
    later = maps[1:].astype(np.float32)
    assert np.array_equal(later.astype(maps.dtype), maps[1:])             # frames >= 1 are float32 values, widened by np.stack
    save = dict(imgs=imgs16, ref_seg_map=heat, original_shape=np.array(original_shape), seed=seed, test_cfg=np.array(json.dumps(cfg0)),
                maps0=maps[0], maps=later)
    if maps64 is not None:
        M = float(np.abs(heat).max())
        diff = np.abs(maps[1:].astype(np.float64) - maps64[1:].astype(np.float64)).reshape(T - 1, -1)
        atol = 2 * DELTA * np.arange(1, T) * M
        noise = np.concatenate([[0.0], diff.max(1)])
        share = np.concatenate([[0.0], (diff > atol[:, None]).mean(1)])
        assert np.all(share == 0), (name, share)
        save.update(ref_noise_max=noise, share_over=share)
    outp = os.path.join(HERE, name + ".npz")
    np.savez_compressed(outp, **save)
    size = os.path.getsize(outp)
    assert size <= 1000000, (outp, size)
    print(outp, maps.dtype, maps.shape, "size", size,
          "ref_noise_max", None if maps64 is None else float(save["ref_noise_max"].max()))


def gen_dense(name, seed, T, h, w, K, map_shape, sigma, original_shape, map_dtype, extra, points=None, edit=None):
    """The set-up of gen_golden_heatmap.gen (VanillaTracker's affinity through the genuine masked_attention_efficient, self.stride = 2).
    Its corr_wrapper is a closure of that function and cannot be imported, so it is restated here with one addition for the float64 pass:
    the label bank (float32, :711) is cast to the features' dtype before the operator multiplies the two (a no-op in the float32 run that
    is recorded).  That the two set-ups are one is checked, not assumed: _save asserts that the reference's img2coord of the maps recorded
    here equals the `coords` of the heat-map fixture bit for bit."""
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
        return ref.masked_attention_efficient(q, k, value_logits.to(q.dtype), mask, temperature=cfg0["temperature"], topk=cfg0["topk"],
                                              step=cfg0["step"], normalize=True, non_mask_len=0, sim_mode="dot_product")
    genuine = vt.masked_attention_efficient_correlation
    vt.masked_attention_efficient_correlation = corr_wrapper
    rng = np.random.default_rng(seed)
    imgs16, _ = _frames(seed, T, h, w, 2)
    mh, mw = map_shape
    if points is None:
        points = np.stack([rng.uniform(0.15 * mw, 0.85 * mw, K), rng.uniform(0.15 * mh, 0.85 * mh, K)], 1)
    heat = pose_heatmaps(points, map_shape, sigma, (h, w)).astype(map_dtype)
    if edit is not None:
        edit(heat)
    outs = []
    for double in (False, True):
        model = ref.builder.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4),
                                                                                  out_indices=(2,), pool_type="none")),
                                        train_cfg=None, test_cfg=ref.ConfigDict({**cfg0, "coords": False}))
        model.backbone.load_state_dict(O.seeded_resnet_state(seed, (1, 1, 1, 4), "none"), strict=True)
        model.eval()
        model.stride = 2
        outs.append(_run(model, imgs16, heat, original_shape, ref_import, double))
    vt.masked_attention_efficient_correlation = genuine                  # gen_local runs the tracker's own operator
    _save(name, imgs16, heat, original_shape, seed, cfg0, outs[0], outs[1], model.img2coord)


def gen_local(name, seed, T, h, w, K, map_shape, sigma, original_shape, map_dtype, extra, points=None):
    """The set-up of gen_golden_hr_seg.gen_heat: nothing in the tracker swapped.  Float32 run only (module docstring)."""
    from gen_golden_hr_seg import BASE, _model, _setup
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
    model = _model(ref, seed, (1, 1, 1, 4), {**cfg0, "coords": False})
    _save(name, imgs16, heat, original_shape, seed, cfg0, _run(model, imgs16, heat, original_shape, ref_import, False), None, model.img2coord)


def main():
    from gen_golden_heatmap import _flat_top
    rng = np.random.default_rng(5)
    K = 15
    pts = np.stack([rng.uniform(6, 34, K), rng.uniform(5, 25, K)], 1)       # (x, y) on a 30 x 40 video
    pts[4] = (-40.0, 12.0)                                                    # a joint off the frame: a zero map throughout
    gen_dense("softmap_jhmdb_6x48x64", 51, 6, 48, 64, K, (30, 40), 4, (30, 40), np.float64, {}, points=pts)
    gen_dense("softmap_badja_6x56x80", 52, 6, 56, 80, 20, (28, 40), 3, (56, 80), np.float64, dict(precede_frames=3))
    gen_dense("softmap_pad_5x41x47", 53, 5, 41, 47, 6, (41, 47), 3, (45, 52), np.float32, dict(precede_frames=3), edit=_flat_top)
    gen_local("hr_softmap_jhmdb_6x48x64", 51, 6, 48, 64, K, (30, 40), 4, (30, 40), np.float64, {}, points=pts)
    gen_local("hr_softmap_pad_5x41x47", 53, 5, 41, 47, 6, (41, 47), 3, (45, 52), np.float32, dict(precede_frames=3))


if __name__ == "__main__":
    main()
