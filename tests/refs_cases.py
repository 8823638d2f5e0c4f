"""Shared by test_refs_host.py and test_gpu_refs.py: the float64 restatements the annotations-at-any-frame path (test_cfg.refs) is held to,
the label recipe of the confidence read-out's cases with its error budget, the late-object clip, and a writer of synthetic clips in the
YouTube-VOS layout.  Everything here runs on the CPU."""
import json
import os
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

DECIDE = 1e-5          # test_gpu_vos.py's: a pixel is decidable when its float64 top-two values differ by more than this
U = 2.0 ** -24         # unit roundoff of f32


def pil_nearest(a: np.ndarray, Hf: int, Wf: int) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((Wf, Hf), Image.NEAREST))


# ---- float64 restatement of the read-out (test_gpu_vos.py's readout_f64, with the field itself returned too) -----------------------------
def field_f64(labels, Hf, Wf, pad_shape, pad, out_shape, norm=True):
    """labels (n, HfWf, C) -> the (normalised) field (n, C, h0, w0) in float64 with torch's own operators, and the smallest denominator
    max - min + 1e-12 of a normalised channel (1.0 when none is)."""
    n, _, C = labels.shape
    x = labels.double().reshape(n, Hf, Wf, C).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=pad_shape, mode="bilinear", align_corners=False)
    lw, uw, lh, uh = pad
    x = x[:, :, lh:pad_shape[0] - uh, lw:pad_shape[1] - uw]
    x = F.interpolate(x, size=out_shape, mode="bilinear", align_corners=False)
    den_min = 1.0
    if norm:
        mn = x.flatten(2).min(-1)[0][..., None, None]
        mx = x.flatten(2).max(-1)[0][..., None, None]
        den = mx - mn + 1e-12
        if bool((mx > 0).any()):
            den_min = float(den[mx > 0].min())
        x = torch.where(mx > 0, (x - mn) / den, x)
    return x, den_min


def readout_f64(labels, Hf, Wf, pad_shape, pad, out_shape, norm=True):
    """labels (n, HfWf, C) -> (argmax (n, h0, w0) int64, top-two gap (n, h0, w0)) in float64."""
    x, _ = field_f64(labels, Hf, Wf, pad_shape, pad, out_shape, norm)
    C = x.shape[1]
    top2 = x.topk(min(2, C), dim=1).values
    gap = (top2[:, 0] - top2[:, 1]) if C > 1 else torch.full_like(top2[:, 0], float("inf"))
    return x.argmax(1), gap


def conf_f64(labels, Hf, Wf, pad_shape, pad, out_shape, norm=True):
    """255 * clamp(best - second, 0, 1) in float64 (n, h0, w0) (C == 1: 255), and field_f64's smallest denominator."""
    x, den_min = field_f64(labels, Hf, Wf, pad_shape, pad, out_shape, norm)
    C = x.shape[1]
    if C == 1:
        return torch.full_like(x[:, 0], 255.0), den_min
    top2 = x.topk(2, dim=1).values
    return 255.0 * (top2[:, 0] - top2[:, 1]).clamp(0.0, 1.0), den_min


# test_gpu_vos.py's READOUT_CASES without the 480p one: (n, Hf, Wf, C, pad_shape, pad (l, r, t, b), out_shape).  93 x 61 = 5673 pixels a
# frame: no multiple of 4, so the second frame's rows start unaligned and the last lane of a frame holds a partial word.
CONF_CASES = [
    (2, 16, 18, 3, (64, 72), (1, 1, 1, 1), (62, 70)),
    (2, 16, 18, 3, (64, 72), (1, 1, 1, 1), (50, 90)),
    (2, 31, 35, 1, (62, 70), (0, 0, 0, 0), (62, 70)),
    (2, 20, 19, 2, (80, 76), (1, 2, 0, 1), (93, 61)),
]
CONF_EXCLUDED_MAX = 0.05


def conf_labels(n, Hf, Wf, C, seed):
    """The label recipe of the confidence cases: what a propagated bank looks like.  Every cell is the one-hot row of a region map (a left /
    right split with a rectangle of the last regular id on top), then 3 % of the cells get a random peaked row (rand ** 3), so that soft
    values, near-ties and every level of the confidence byte occur.  With C > 2 the last channel is negative everywhere: its maximum is
    <= 0, it is not normalised and never wins.  All values lie in [-1, 1]."""
    g = torch.Generator().manual_seed(seed)
    ids = max(C - 1, 1) if C > 2 else C
    ys, xs = torch.meshgrid(torch.arange(Hf), torch.arange(Wf), indexing="ij")
    region = (xs >= Wf // 2).long() % ids
    region[Hf // 4:Hf // 2, Wf // 3:2 * Wf // 3] = ids - 1
    lab = F.one_hot(region.reshape(-1), C).double()[None].repeat(n, 1, 1)
    soft = torch.rand(n, Hf * Wf, generator=g) < 0.03
    rows = torch.rand(n, Hf * Wf, C, generator=g, dtype=torch.float64) ** 3
    lab[soft] = rows[soft]
    if C > 2:
        lab[..., -1] = -0.25 - 0.5 * torch.rand(n, Hf * Wf, generator=g, dtype=torch.float64)
    return lab.float()


def conf_delta(case, norm, den_min):
    """The error budget of 255 * gap between the kernel's f32 chain and float64, in levels of the confidence byte.  Every rounded f32
    operation adds at most U relative to its result; values are at most 1 in magnitude.
      source coordinates   s = scale * (d + 0.5) - 0.5: the scale's division, the product and the subtraction, 3 roundings on a value below
                           the source size S, so an interpolation weight is off by at most 3 U S; it multiplies a difference of two values
                           (at most 1, weights sum to 1).  One such term per axis and per resize: stage 1 reads the feature grid (Hf, Wf),
                           the second resize (only where the output size differs from the unpadded one) the unpadded frame (h, w);
      weights and sums     per resize and axis the weight pair costs 2 roundings and a product of two weights 1; the field is 4 (composed:
                           16) fused multiply-adds and as many row folds: 32 roundings bound either form;
      normalisation        (v - min) / (max - min + 1e-12): v, min and max each carry the error above, so the quotient carries 4 e / den
                           (den >= den_min, from the float64 restatement) plus 3 roundings of its own;
      the gap              two such values, one subtraction, one product with 255."""
    n, Hf, Wf, C, pad_shape, pad, out_shape = case
    lw, uw, lh, uh = pad
    h, w = pad_shape[0] - lh - uh, pad_shape[1] - lw - uw
    composed = (h, w) != tuple(out_shape)
    coord = 3 * (Hf + Wf) + (3 * (h + w) if composed else 0)
    e_v = U * (32 + coord)
    e_n = (4 * e_v / den_min + 3 * U) if norm else e_v
    return 255.0 * (2 * e_n + 2 * U)


def conf_verdict(got: torch.Tensor, want64: torch.Tensor, delta: float):
    """(largest level difference, mismatches among the pixels that must be equal, excluded share): a pixel must be equal when the float64
    value is farther than delta from a half-integer."""
    target = torch.round(want64)                                   # (ties to even: a tie is excluded below anyway)
    diff = (got.double() - target).abs()
    frac = want64 - torch.floor(want64)
    must = (frac - 0.5).abs() > delta
    return float(diff.max()), int(((diff != 0) & must).sum()), float((~must).double().mean())


# ---- the late-object clip ------------------------------------------------------------------------------------------------------------------
def clip_chw(T, C_feat, Hf, Wf, seed):
    """test_gpu_vos.py's _clip recipe before normalisation: (T, C, Hf, Wf) float32 on the host."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, C_feat, Hf, Wf, generator=g)
    return torch.cat([torch.roll(base, shifts=(t, t), dims=(2, 3)) + 0.3 * torch.randn(1, C_feat, Hf, Wf, generator=g) for t in range(T)])


LATE_T, LATE_H, LATE_W, LATE_D, LATE_SEED = 8, 62, 70, 2, 11
LATE_KW = dict(neighbor_range=8, precede_frames=3)


def late_maps():
    """{0: three objects, 3: object 2 re-drawn elsewhere and a new id 4} at 62 x 70."""
    a = np.zeros((LATE_H, LATE_W), np.uint8)
    a[10:30, 8:30], a[35:55, 20:45], a[5:25, 40:66] = 1, 2, 3
    b = np.zeros((LATE_H, LATE_W), np.uint8)
    b[38:58, 24:50] = 2
    b[28:44, 50:68] = 4
    return {0: a, 3: b}


def oracle_lists(feats_chw: torch.Tensor, cfg) -> SimpleNamespace:
    """A LabelSweep's tensors for the clip feats_chw (n, C, Hf, Wf) from the oracle's float64 dense affinity: per frame j >= 1 the top-k of
    its key slots' masked correlation (every slot masked: with_first_neighbor) and their softmax."""
    from fgvc_amd import engine
    from oracle import fgvc_oracle as O
    n, _, Hf, Wf = feats_chw.shape
    HW = Hf * Wf
    t_max = cfg.precede_frames + 1
    sf, idx, wgt = [], [], []
    for j in range(1, n):
        ks = engine.key_slots(j, 0, cfg.precede_frames, cfg.with_first)
        dense = O.corr_volume(feats_chw[j].double(), feats_chw[ks].transpose(0, 1).double(), cfg.temperature)
        m = O.mask_slab(Hf, Wf, Hf, Wf, len(ks), torch.arange(HW), cfg.neighbor_range, cfg.mask_mode)
        val, ix = O.topk_canonical(dense.masked_fill(~m, float("-inf")), cfg.topk)
        sf.append(ks + [0] * (t_max - len(ks)))
        idx.append(ix.t().contiguous())
        wgt.append(torch.softmax(val.t(), dim=1))
    return SimpleNamespace(slot_frame=torch.tensor(sf), idx=torch.stack(idx), weight=torch.stack(wgt), window_L=0)


def restated_masks(small, T, fw, bw, direction, override, hard, Hf, Wf, pad_shape, pad, out_shape, norm=True):
    """engine.sweep_refs_host on the given lists, read out in float64: (argmax (T, h0, w0), gap (T, h0, w0))."""
    from fgvc_amd import engine
    soft = engine.sweep_refs_host(small, T, fw=fw, bw=bw, direction=direction, override=override, hard_prop=hard)
    return readout_f64(soft, Hf, Wf, pad_shape, pad, out_shape, norm)


# ---- synthetic clips in the YouTube-VOS layout ----------------------------------------------------------------------------------------------
def write_fake_ytvos(root, videos=2, frames=6, size=(48, 64), seed=0, full_gt=False, step=5):
    """JPEGImages/<video>/<frame>.jpg, Annotations/<video>/<frame>.png (palette PNGs at the frames where objects first appear; every frame
    with full_gt) and meta.json.  Frame names are 5-digit numbers `step` apart, as the dataset's.  Object 1 is there from the first frame,
    object 2 enters at the third.  Returns {video: (frame names, {frame index: map}, all maps (T, h, w))}."""
    from PIL import Image
    from fgvc_amd.viz import davis_palette
    rng = np.random.default_rng(seed)
    h, w = size
    out, meta = {}, {"videos": {}}
    for v in range(videos):
        name = f"vid{v:02d}"
        os.makedirs(os.path.join(root, "JPEGImages", name))
        os.makedirs(os.path.join(root, "Annotations", name))
        names = [f"{step * i:05d}" for i in range(frames)]
        back = rng.integers(0, 255, (h, w, 3), dtype=np.uint8)
        maps = np.zeros((frames, h, w), np.uint8)
        for i in range(frames):
            maps[i, 5 + i:20 + i, 6 + 2 * i:26 + 2 * i] = 1
            if i >= 2:
                maps[i, 26:40, 30 + i:50 + i] = 2
            img = back.copy()
            img[maps[i] == 1] = (220, 40, 40)
            img[maps[i] == 2] = (40, 40, 220)
            Image.fromarray(img).save(os.path.join(root, "JPEGImages", name, names[i] + ".jpg"), quality=95)
        refs = {0: maps[0].copy(), 2: np.where(maps[2] == 2, 2, 0).astype(np.uint8)}
        for i in range(frames):
            if full_gt or i in refs:
                im = Image.fromarray(maps[i] if full_gt else refs[i], mode="P")
                im.putpalette(davis_palette().tobytes())
                im.save(os.path.join(root, "Annotations", name, names[i] + ".png"))
        meta["videos"][name] = {"objects": {"1": {"category": "a", "frames": names}, "2": {"category": "b", "frames": names[2:]}}}
        out[name] = (names, refs, maps)
    with open(os.path.join(root, "meta.json"), "w") as f:
        json.dump(meta, f)
    return out
