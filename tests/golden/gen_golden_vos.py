"""Record the fixtures of the mask path (semi-supervised VOS) from the reference, executed read-only in place (never copied).

    python tests/golden/gen_golden_vos.py          # writes tests/golden/vos_*.npz

Tracker fixtures (vos_8x62x70, vos_hard_8x62x70, vos_vanish_5x41x47): the genuine HRVanillaTracker.forward_test_backward_save_mem
(vanilla_tracker.py:663-830) on CPU under oracle/ref_import.py, with these replacements:
  - affinity: `masked_attention_efficient_correlation` in the tracker module's namespace becomes a wrapper that encodes the query and
    key frames with the genuine backbone and calls the genuine `masked_attention_efficient` with the genuine `spatial_neighbor` mask and
    VanillaTracker's keys (vanilla_tracker.py:330-378: temperature, topk, step, with_norm, non_mask_len from with_first_neighbor);
  - mmcv.imresize(..., interpolation='nearest', backend='pillow') is Pillow's resize (what mmcv calls on that backend);
    mmcv.ops.Correlation is ref_import's stand-in (constructed, never called here);
  - self.stride = 2: the output stride of the res18_d1 encoder (stem stride 2, strides 1, 1, 1 up to layer 3), the padding unit the
    product uses (VanillaTracker.output_stride).
Frames are float16-rounded (stored as such) so the fixture is exactly the reference's input.  Also stored per output pixel: the gap
between the top two normalised channel values the reference's argmax saw (f32, spied), which says which pixels are decidable.

J&F fixture (vos_jf.npz): the reference's metric functions (mmpt/core/evaluation/metrics.py).  PINNED UNDER STAND-INS: the metric module imports cv2, mmcv and skimage, none of which is installed here.  cv2.dilate(b, k) is
scipy.ndimage.binary_dilation(b, structure=k) as uint8 (a symmetric kernel and a zero border make them the same operation);
skimage.morphology.disk(r) is the footprint x^2 + y^2 <= r^2 as uint8 (skimage's definition); mmcv is an empty module; numpy 2 lost
`np.bool`, so np.bool = bool for the duration.  The recorded values are the genuine functions' arithmetic under those stand-ins.
"""
from __future__ import annotations

import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_import import REF_ROOT  # noqa: E402


def _standins():
    from scipy.ndimage import binary_dilation
    cv2 = types.ModuleType("cv2")
    cv2.dilate = lambda b, k: binary_dilation(b.astype(bool), structure=k.astype(bool)).astype(np.uint8) if b.any() else b.astype(np.uint8)
    sk = types.ModuleType("skimage")
    morph = types.ModuleType("skimage.morphology")

    def disk(r):
        r = int(r)
        y, x = np.mgrid[-r:r + 1, -r:r + 1]
        return ((x * x + y * y) <= r * r).astype(np.uint8)
    morph.disk = disk
    sk.morphology = morph
    return {"cv2": cv2, "mmcv": types.ModuleType("mmcv"), "skimage": sk, "skimage.morphology": morph}


def load_reference_metrics():
    """The genuine module with the stand-ins installed in sys.modules (f_measure imports skimage at call time: they stay for the run)."""
    sys.modules.update(_standins())
    np.bool = bool
    spec = importlib.util.spec_from_file_location("ref_vos_metrics", os.path.join(REF_ROOT, "mmpt/core/evaluation/metrics.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def cases(seed: int = 0):
    """(objects, T, h, w) ground truth and prediction: moving discs, the prediction shifted and eroded by a few pixels, one object the
    prediction loses halfway, one frame with an empty annotation."""
    rng = np.random.default_rng(seed)
    O, T, h, w = 3, 9, 60, 84
    yy, xx = np.mgrid[0:h, 0:w]
    gt = np.zeros((O, T, h, w), bool)
    pr = np.zeros_like(gt)
    for o in range(O):
        c = rng.uniform([15, 15], [45, 69])
        v = rng.uniform(-2, 2, 2)
        r = rng.uniform(6, 14)
        for t in range(T):
            cy, cx = c + t * v
            gt[o, t] = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
            dy, dx = rng.integers(-3, 4, 2)
            pr[o, t] = (yy - cy - dy) ** 2 + (xx - cx - dx) ** 2 <= (r - rng.uniform(0, 3)) ** 2
    pr[2, 5:] = False
    gt[1, 4] = False
    return gt, pr


def _frames(seed, T, h, w, objects):
    """Moving textured ellipses on a smooth random texture, (1, T, 3, h, w) float16 in about [-1, 1], and the frame-0 id map."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]

    def tex():
        base = rng.random((h // 4 + 2, w // 4 + 2, 3))
        return np.kron(base, np.ones((4, 4, 1)))[:h, :w] * 1.2 - 0.6 + 0.1 * rng.standard_normal((h, w, 3))
    bg = tex()
    obj = [dict(c=rng.uniform([0.3 * h, 0.2 * w], [0.7 * h, 0.8 * w]), v=rng.uniform(-1.2, 1.2, 2),
                r=rng.uniform([0.12 * h, 0.1 * w], [0.22 * h, 0.18 * w]), col=rng.uniform(-0.8, 0.8, 3), tex=tex() * 0.4)
           for _ in range(objects)]
    imgs = np.zeros((T, 3, h, w), np.float32)
    seg0 = np.zeros((h, w), np.uint8)
    for t in range(T):
        img = bg.copy()
        for k, o in enumerate(obj):
            c = o["c"] + t * o["v"]
            inside = ((yy - c[0]) / o["r"][0]) ** 2 + ((xx - c[1]) / o["r"][1]) ** 2 <= 1.0
            img[inside] = o["col"] + o["tex"][inside]
            if t == 0:
                seg0[inside] = k + 1
        imgs[t] = img.transpose(2, 0, 1)
    return imgs.astype(np.float16)[None], seg0


class _ArgmaxSpy:
    """Records the top-two gap of every (B, C, h0, w0) tensor the reference takes an argmax over dim 1 of (the read-out's)."""

    def __init__(self, out_hw):
        self.out_hw, self.gaps = tuple(out_hw), []

    def __enter__(self):
        import torch
        self._orig = torch.Tensor.argmax
        spy = self

        def argmax(t, *a, **k):
            if t.ndim == 4 and tuple(t.shape[-2:]) == spy.out_hw and (a[:1] == (1,) or k.get("dim") == 1):
                v = t.double().topk(min(2, t.shape[1]), dim=1).values
                spy.gaps.append((v[0, 0] - v[0, 1]).numpy() if t.shape[1] > 1 else np.full(spy.out_hw, np.inf))
            return spy._orig(t, *a, **k)
        torch.Tensor.argmax = argmax
        return self

    def __exit__(self, *exc):
        import torch
        torch.Tensor.argmax = self._orig
        return False


def gen_tracker(name, seed, T, h, w, objects, original_shape, extra, seg_edit=None):
    import torch
    from PIL import Image
    from oracle import fgvc_oracle as O
    from oracle import ref_import
    ref = ref_import.load()
    vt = sys.modules["mmpt.models.trackers.vanilla_tracker"]
    mmcv = sys.modules["mmcv"]

    def imresize(img, size, interpolation="bilinear", backend=None, **_):
        assert interpolation == "nearest" and backend == "pillow", (interpolation, backend)
        return np.asarray(Image.fromarray(img).resize(tuple(size), Image.NEAREST))
    mmcv.imresize = imresize
    cfg = ref.ConfigDict({**dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=8, step=512, with_first=True,
                                 with_first_neighbor=True), **extra})

    def corr_wrapper(query_frame, key_frames, value_logits, radius=None, corr_infer=None, feat_extractor=None, temperature=1.0,
                     topk=None, sstep=None, tstep=None, normalize=True):
        def enc(x):
            f = feat_extractor(x)
            return f[0] if isinstance(f, (list, tuple)) else f
        q = enc(query_frame)
        Tk = key_frames.shape[2]
        k = torch.stack([enc(key_frames[:, :, t]) for t in range(Tk)], 2)
        mask = ref.spatial_neighbor(q.shape[0], *q.shape[2:], neighbor_range=cfg.neighbor_range, device=q.device, dtype=q.dtype,
                                    mode=cfg.get("mask_mode", "circle"))
        return ref.masked_attention_efficient(q, k, value_logits, mask, temperature=cfg.temperature, topk=cfg.topk,
                                              step=cfg.get("step", 32), normalize=cfg.get("with_norm", True),
                                              non_mask_len=0 if cfg.get("with_first_neighbor", True) else 1,
                                              sim_mode=cfg.get("sim_mode", "dot_product"))
    vt.masked_attention_efficient_correlation = corr_wrapper
    model = ref.builder.build_model(dict(type="HRVanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4),
                                                                              out_indices=(2,), pool_type="none")),
                                    train_cfg=None, test_cfg=cfg)
    model.backbone.load_state_dict(O.seeded_resnet_state(seed, (1, 1, 1, 4), "none"), strict=True)
    model.eval()
    model.stride = 2
    imgs16, seg0 = _frames(seed, T, h, w, objects)
    if seg_edit is not None:
        seg_edit(seg0)
    imgs = torch.from_numpy(imgs16.astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()   # (1, 1, 3, T, h, w)
    ref_seg = torch.from_numpy(seg0).unsqueeze(0)          # uint8, as the mask pipelines load it (Image.fromarray needs it)
    with ref_import.cuda_as_cpu(), torch.no_grad(), _ArgmaxSpy(original_shape) as spy:
        out = model.forward_test_backward_save_mem(imgs, ref_seg, [dict(original_shape=tuple(original_shape))])
    assert isinstance(out, list) and len(out) == 1
    masks = np.asarray(out[0])
    assert masks.shape == (T, *original_shape), masks.shape
    assert len(spy.gaps) == T - 1, len(spy.gaps)
    save = dict(imgs=imgs16, ref_seg_map=seg0, original_shape=np.array(original_shape), seed=seed,
                out_dtype=str(masks.dtype), masks=masks.astype(np.uint8), gap=np.stack(spy.gaps).astype(np.float32),
                test_cfg=np.array(json.dumps(dict(cfg))))
    assert np.array_equal(masks, masks.astype(np.uint8))
    outp = os.path.join(HERE, name + ".npz")
    np.savez_compressed(outp, **save)
    print(outp, masks.shape, "ids", np.unique(masks).tolist(), "undecidable", int((save["gap"] <= 1e-5).sum()))


def _vanish(seg):
    seg[30, 32] = seg.max() + 1            # even row and column: Pillow's nearest sample to half size reads the odd ones


def main():
    gen_tracker("vos_8x62x70", 41, 8, 62, 70, 3, (62, 70), {})
    gen_tracker("vos_hard_8x62x70", 41, 8, 62, 70, 3, (62, 70), dict(hard_prop=True))
    gen_tracker("vos_vanish_5x41x47", 43, 5, 41, 47, 2, (45, 52), dict(precede_frames=3), seg_edit=_vanish)
    m = load_reference_metrics()
    gt, pr = cases()
    saved = {"gt": gt, "pred": pr}
    for o in range(gt.shape[0]):
        saved[f"iou_{o}"] = np.asarray(m.db_eval_iou(gt[o], pr[o]), dtype=np.float64)
        saved[f"f_{o}"] = np.asarray(m.db_eval_boundary(gt[o], pr[o]), dtype=np.float64)
    jfm = m.JFM(gt, pr, gt.shape[0])
    for k, v in jfm.items():
        saved["JFM_" + k] = np.asarray(v, dtype=np.float64)
    out = os.path.join(HERE, "vos_jf.npz")
    np.savez_compressed(out, **saved)
    print(out, {k: np.round(v, 4).tolist() for k, v in saved.items() if k.startswith("JFM_")})


if __name__ == "__main__":
    main()
