"""Shapes, seeded inputs and float64 restatements shared by tests/test_gpu_post_ops.py (the HIP kernels of csrc/post.hip) and
tests/test_post_reference_share.py (the reference alone, on the CPU: which read-out maps the coordinate check holds, and that the
restatements below reproduce the oracle).  No GPU code here: everything is a plain torch / numpy evaluation on the CPU.

Read-out.  A map is CHECKABLE when its float64 ranks 5 and 6 are separated by more than CLEAR of the maximum (the top five are the same
set under any rounding), when they tie STRUCTURALLY (exactly equal in float64 and the two pixels are border replicas of each other: the
bilinear upsample repeats the rows whose source coordinate clamps to 0 and those with i0 == in_size - 1, so the pick is decided by the
canonical rule "the higher flat index stays", never by rounding), or when its f32 sum is 0 (the answer is -1 whichever pixels rank).
"""
import numpy as np
import torch
import torch.nn.functional as F

TEMP = 0.07
CLEAR = 1e-5              # tests/test_gpu_heatmap.py::CLEAR
MIN_SHARE = 0.95          # a read-out case may leave at most 5 % of its maps out of the coordinate check
TOL_PX, TOL_F32_ULPS = 1e-5, 4
F32_MIN_NORMAL = 2.0 ** -126


def readout_tol(h, w):
    """tests/test_gpu_heatmap.py::_tol(False, (h, w)), restated (that module is GPU-only): 1e-5 px + 4 ulps of the largest coordinate
    for the one f32 rounding of the top-5 sum.  tests/test_post_reference_share.py ties it to the reference's own f32 pipeline."""
    return TOL_PX + TOL_F32_ULPS * 2.0 ** -24 * max(h, w)


# name, T, Hf, Wf, P, h, w
READOUT = [("base", 3, 30, 54, 17, 120, 216), ("ragged", 2, 30, 54, 5, 119, 213), ("scale8", 2, 16, 20, 3, 128, 160),
           ("identity", 2, 24, 32, 4, 24, 32), ("down2", 2, 24, 32, 4, 12, 16), ("odd", 2, 11, 12, 7, 41, 47), ("tiny", 1, 3, 5, 1, 9, 17),
           ("scale1.5", 2, 20, 27, 6, 30, 40), ("bumps04", 2, 30, 54, 9, 120, 216),
           # bumps centred on the four borders and the four corners, an all-zero channel, a channel with negative values
           ("special_x4", 2, 12, 16, 10, 48, 64)]
# power-of-two scales of labels quantised to multiples of 2^-8: every product and sum of the interpolation is exact in f32
EXACT = [("noise_x2", 16, 20, 2), ("noise_x4", 16, 20, 4), ("noise_x8", 16, 20, 8), ("plateau_x4", 16, 20, 4), ("corners_x4", 16, 20, 4)]
# (Hf, Wf, stride, P, sigma)
GAUSS = [(30, 54, 4, 17, 6.0), (12, 16, 2, 2, 6.0), (7, 9, 8, 1, 3.0), (33, 70, 1, 5, 1.0)]
# (n, C, H, W); the last is an addition of this module: padding channels 40 -> 64
NORMALIZE = [(1, 512, 5, 7), (2, 1, 3, 3), (1, 371, 1, 1), (1, 64, 1, 33), (2, 40, 3, 13)]
MERGE_T = [1, 2, 7, 20]
MERGE_HWQ = [1, 255, 257, 1000]
MERGE_HWK = 37
PROP_P = [1, 3, 17, 40]
PROP_TOPK = [1, 5, 10, 16]
PROP_GRIDS = [(5, 33), (17, 23)]
PROP_SLOTS = [[0, 3, 3, 5], [4, 1, 5, 0, 2], [2]]          # the engine's shape (a frame twice), a permutation, one slot


def case_id(c):
    return c[0] if isinstance(c[0], str) else "x".join(str(v) for v in c)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ----------------------------------------------------------------------------------------------------------------------
# read-out
# ----------------------------------------------------------------------------------------------------------------------
def _bump(Hf, Wf, cy, cx, sy, sx, amp=1.0):
    yy, xx = np.mgrid[0:Hf, 0:Wf]
    return amp * np.exp(-((yy - cy) ** 2 / (2 * sy * sy) + (xx - cx) ** 2 / (2 * sx * sx)))


def readout_labels(case):
    """(T, HfWf, P) f32 propagated-like labels of one READOUT case: one seeded bump per (frame, channel)."""
    name, T, Hf, Wf, P, h, w = case
    rng = np.random.default_rng(11 + 7 * Hf + 13 * Wf + 31 * h + P)
    b = np.zeros((T, Hf, Wf, P))
    for t in range(T):
        if name.startswith("special"):
            cyr, cxr = rng.uniform(2.2, Hf - 3.2), rng.uniform(2.2, Wf - 3.2)
            centres = [(0, cxr), (Hf - 1, cxr), (cyr, 0), (cyr, Wf - 1), (0, 0), (0, Wf - 1), (Hf - 1, 0), (Hf - 1, Wf - 1)]
            for k, (cy, cx) in enumerate(centres):           # anisotropic: a corner bump is not symmetric under x <-> y
                b[t, :, :, k] = _bump(Hf, Wf, cy, cx, 2.0, 2.7, rng.uniform(0.3, 1.0))
            b[t, :, :, 9] = _bump(Hf, Wf, cyr, cxr, 2.0, 2.7) - 0.3          # negative values; channel 8 stays all zero
            continue
        for k in range(P):
            s = 0.4 if name == "bumps04" else rng.uniform(1.5, 4.0)
            b[t, :, :, k] = _bump(Hf, Wf, rng.uniform(0, Hf - 1), rng.uniform(0, Wf - 1), s, s, rng.uniform(0.3, 1.0))
    return torch.from_numpy(b.reshape(T, Hf * Wf, P)).float()


def exact_labels(case):
    """(1, HfWf, P) f32 labels whose x2 / x4 / x8 bilinear field is exact in f32: multiples of 2^-8 in [0, 1]."""
    name, Hf, Wf, scale = case
    g = _gen(500 + scale + len(name))
    if name.startswith("noise"):
        lab = torch.randint(0, 257, (1, Hf, Wf, 4), generator=g).float() / 256
    elif name.startswith("plateau"):                         # a 1.0 plateau wider than five pixels on a quantised slope
        lab = torch.randint(0, 129, (1, Hf, Wf, 3), generator=g).float() / 256
        lab[0, 4:9, 6:13, 0] = 1.0
        lab[0, 0:3, :, 1] = 1.0                              # touching the top border
        lab[0, :, Wf - 2:, 2] = 1.0                          # touching the right border
    else:                                                    # one hot cell in each corner, one channel per corner
        lab = torch.zeros(1, Hf, Wf, 4)
        for k, (y, x) in enumerate([(0, 0), (0, Wf - 1), (Hf - 1, 0), (Hf - 1, Wf - 1)]):
            lab[0, y, x, k] = 1.0
    return lab.reshape(1, Hf * Wf, -1).contiguous()


def field(labels, Hf, Wf, h, w, dtype=torch.float64):
    """(T, P, h, w): F.interpolate(bilinear, align_corners=False) of (T, HfWf, P) labels, evaluated in `dtype`."""
    T, _, P = labels.shape
    x = labels.to(dtype).reshape(T, Hf, Wf, P).permute(0, 3, 1, 2)
    return F.interpolate(x, size=(h, w), mode="bilinear", align_corners=False)


def gauss_frame(points, h, w, sigma, stride=1):
    """(P, h, w) float64: exp(-((x - cx)^2 + (y - cy)^2) / (2 sigma^2)) at (x * stride, y * stride), from the f32-ROUNDED points (the
    kernels' operands).  Also returns arg = d^2 / (2 sigma^2)."""
    p = points.float().double()
    xs = (torch.arange(w, dtype=torch.float64) * stride).view(1, 1, w)
    ys = (torch.arange(h, dtype=torch.float64) * stride).view(1, h, 1)
    arg = ((xs - p[:, 0].view(-1, 1, 1)) ** 2 + (ys - p[:, 1].view(-1, 1, 1)) ** 2) / (2.0 * sigma * sigma)
    return torch.exp(-arg), arg


def axis_class(n_in, n_out):
    """(n_out,) replica class of every output coordinate of one axis: -1 where the source coordinate clamps to 0, -2 where
    i0 == n_in - 1 (i1 == i0: one source row), else the coordinate itself (a class of its own)."""
    d = torch.arange(n_out, dtype=torch.float64)
    raw = (n_in / n_out) * (d + 0.5) - 0.5
    i0 = raw.clamp_min(0).floor().long().clamp_max(n_in - 1)
    cls = torch.arange(n_out)
    cls = torch.where(i0 == n_in - 1, torch.full_like(cls, -2), cls)
    return torch.where(raw <= 0, torch.full_like(cls, -1), cls)


def readout_picks(maps, cls_y=None, cls_x=None):
    """img2coord (vanilla_tracker.py:172-191) of (T, P, h, w) float64 maps as tests/test_gpu_heatmap.py::img2coord_restated states it for
    an f32 stack: stable ascending sort (the higher flat index last), the last five, float32 normalisation, -1 where the f32 sum is 0.
    Returns dict(coords (T, P, 2) = (x, y) float64, gap (T, P) = (5th - 6th) / max in float64, tie = ranks 5 and 6 equal in float64,
    structural = tie between border replicas (cls_y / cls_x = axis_class of the two axes; None: no replicas), zero, checkable)."""
    T, P, h, w = maps.shape
    flat = maps.reshape(T, P, -1)
    s64, i64 = torch.sort(flat, dim=-1, stable=True)
    gap = (s64[..., -5] - s64[..., -6]) / s64[..., -1].abs().clamp_min(1e-300)
    tie = s64[..., -5] == s64[..., -6]
    a, b = i64[..., -5], i64[..., -6]
    cls_y = torch.arange(h) if cls_y is None else cls_y
    cls_x = torch.arange(w) if cls_x is None else cls_x
    structural = tie & (cls_y[a // w] == cls_y[b // w]) & (cls_x[a % w] == cls_x[b % w])
    work = flat.float()
    s32, i32 = torch.sort(work, dim=-1, stable=True)
    top_i, top_v = i32[..., -5:].numpy(), s32[..., -5:].numpy()
    v = top_v / (np.sum(top_v, axis=-1, keepdims=True) + 1e-9)                     # stays float32
    coords = np.stack([np.sum((top_i % w) * v, axis=-1), np.sum((top_i // w) * v, axis=-1)], -1)
    zero = (work.sum(-1) == 0)
    coords[zero.numpy()] = -1
    return dict(coords=coords, gap=gap, tie=tie, structural=structural, zero=zero, checkable=(gap > CLEAR) | structural | zero)


def readout_points(h, w):
    """First-frame centres for the analytic frame 0 of a read-out: (points (P, 2) f32, exact (P,) bool, far (P,) bool).
    exact: both coordinates are multiples of 0.5, so every squared distance is exact in f32 and in f64, equal distances give equal
    values in either arithmetic, and a tie at rank 5 is decided by the canonical rule (the higher flat index stays), not by rounding.
    far: the label underflows to 0 on the whole image, the read-out is exactly -1."""
    pts = [(w * 0.37 + 0.21, h * 0.61 + 0.13, 0), (w * 0.8 - 0.37, h * 0.2 + 0.41, 0),            # inside
           (20.5, 30.5, 1), (w - 1.5, 0.5, 1),                                                  # x.5, y.5: four-way exact ties at the top
           (0.0, h // 2, 1), (w // 3, h - 1.0, 1), (0.0, 0.0, 1), (w - 1.0, h - 1.0, 1),        # on the border, in the corners
           (-3.0, h // 2, 1), (w // 2, h + 2.0, 1), (-3.0, -3.0, 1),                            # 3 px outside
           (w + 1000.0, h / 2, 2), (-1e4, -1e4, 2)]                                             # far outside
    t = torch.tensor(pts, dtype=torch.float64)
    return t[:, :2].float(), t[:, 2] >= 1, t[:, 2] == 2


def first_frame_want(points, exact, h, w, sigma=6.0):
    """readout_picks of the analytic first frame; structural = an exact tie of a centre with exact distances."""
    want = readout_picks(gauss_frame(points, h, w, sigma)[0][None])
    want["structural"] = want["tie"] & exact.view(1, -1)
    want["checkable"] = (want["gap"] > CLEAR) | want["structural"] | want["zero"]
    return want


def readout_want(case, labels):
    name, T, Hf, Wf, P, h, w = case
    return readout_picks(field(labels, Hf, Wf, h, w), axis_class(Hf, h), axis_class(Wf, w))


# ----------------------------------------------------------------------------------------------------------------------
# merge
# ----------------------------------------------------------------------------------------------------------------------
def merge_lists(n_pairs, HWq, HWk, topk, seed):
    """Synthetic per-pair lists as fgvc_pair_topk_f32 writes them: (n_pairs, HWq, topk) int32 ids / f32 scores in (score desc, id asc)
    order, distinct ids within a list, a -1 / -inf tail after a random length 0..topk (half of the lists are full).  Scores are
    cosines in [-0.55, 0.55], so that every logit at temperature 0.07 is below 8 in size and half an ulp of it is at most 2^-22 (the
    softmax bound of tests/test_gpu_post_ops.py is derived for that); a third of the rows hold multiples of 1/8 only, so scores tie within
    a list and across lists."""
    g = _gen(3000 + seed)
    score = (torch.rand(n_pairs, HWq, topk, generator=g) * 2 - 1) * 0.55
    quant = torch.rand(1, HWq, 1, generator=g) < 0.33
    score = torch.where(quant, (score * 8).round() / 8, score)
    ids = torch.rand(n_pairs, HWq, HWk, generator=g).argsort(-1)[..., :topk]
    o = torch.sort(ids, dim=-1, stable=True)[1]
    ids, score = ids.gather(-1, o), score.gather(-1, o)
    o = torch.sort(score, dim=-1, descending=True, stable=True)[1]
    ids, score = ids.gather(-1, o), score.gather(-1, o)
    length = torch.randint(0, topk + 1, (n_pairs, HWq, 1), generator=g)
    length = torch.where(torch.rand(n_pairs, HWq, 1, generator=g) < 0.5, torch.full_like(length, topk), length)
    tail = torch.arange(topk).view(1, 1, topk) >= length
    return ids.masked_fill(tail, -1).int(), score.masked_fill(tail, float("-inf")).float()


def merge_slot_pairs(n_out, T, n_pairs, seed):
    """(n_out, T) int32: row 0 random pairs with a -1 slot and a pair held twice (T >= 3); row 1 every slot holds the same pair (every
    score ties across slots: the lower gid first); row 2 a single used slot (fewer than topk candidates wherever its list is short)."""
    g = _gen(4000 + seed)
    sp = torch.randint(0, n_pairs, (n_out, T), generator=g)
    if T >= 2:
        sp[0, T - 1] = sp[0, 0]
    if T >= 3:
        sp[0, 1] = -1
    if n_out > 1:
        sp[1, :] = sp[1, 0]
    if n_out > 2:
        sp[2, :] = -1
        sp[2, T // 2] = n_pairs - 1
    return sp.int()


def merge_restated(pair_idx, pair_score, slot_pair, HWk, topk, temperature=TEMP):
    """Pool every valid (score, gid = slot * HWk + id) of an output row, sort by (score desc, gid asc), take topk.
    Returns idx (n_out, HWq, topk) int64 (-1: no candidate), logit = score / temperature, the softmax over the valid entries and
    clamp(min=0)**2, all float64, and the valid mask."""
    n_out, T = slot_pair.shape
    sp = slot_pair.long()
    pi = pair_idx.long()[sp.clamp_min(0)]                                           # (n_out, T, HWq, k)
    ps = pair_score.double()[sp.clamp_min(0)]
    ok = (pi >= 0) & (sp >= 0).view(n_out, T, 1, 1)
    gid = torch.arange(T).view(1, T, 1, 1) * HWk + pi
    gid = torch.where(ok, gid, torch.full_like(gid, T * HWk))
    ps = torch.where(ok, ps, torch.full_like(ps, float("-inf")))
    HWq = pi.shape[2]
    gid, ps = gid.permute(0, 2, 1, 3).reshape(n_out, HWq, -1), ps.permute(0, 2, 1, 3).reshape(n_out, HWq, -1)
    o = torch.sort(gid, dim=-1, stable=True)[1]
    gid, ps = gid.gather(-1, o), ps.gather(-1, o)
    o = torch.sort(ps, dim=-1, descending=True, stable=True)[1]
    gid, ps = gid.gather(-1, o)[..., :topk], ps.gather(-1, o)[..., :topk]
    valid = ps > float("-inf")
    idx = torch.where(valid, gid, torch.full_like(gid, -1))
    logit = ps / temperature
    e = torch.where(valid, torch.exp(logit - logit[..., :1]), torch.zeros_like(logit))
    soft = e / e.sum(-1, keepdim=True)
    return dict(idx=idx, logit=logit, softmax=soft, cosine=logit.clamp(min=0) ** 2, valid=valid)


def merge_dense(pair_idx, pair_score, slot_row, HWk):
    """(T * HWk, HWq) float64 slab of one output row built from the same lists: -inf where no list holds the candidate."""
    T, HWq = slot_row.numel(), pair_idx.shape[1]
    dense = torch.full((T * HWk, HWq), float("-inf"), dtype=torch.float64)
    q = torch.arange(HWq).view(HWq, 1).expand(HWq, pair_idx.shape[2])
    for t, p in enumerate(slot_row.tolist()):
        if p < 0:
            continue
        ok = pair_idx[p] >= 0
        dense[(t * HWk + pair_idx[p].long())[ok], q[ok]] = pair_score[p].double()[ok]
    return dense


# ----------------------------------------------------------------------------------------------------------------------
# propagate
# ----------------------------------------------------------------------------------------------------------------------
def propagate_inputs(P, topk, Hq, Wq, Hk, Wk, slot_frame, window_L, seed, n_frames=6, empty=0.15):
    """labels (n_frames, HkWk, P) f32 with both signs, idx (HqWq, topk) int32 over slot * span + pixel-or-tap with a share of -1, weight
    (HqWq, topk) f32 in [0, 1]."""
    g = _gen(5000 + seed + P + 7 * topk + 13 * Hq + window_L)
    labels = torch.rand(n_frames, Hk * Wk, P, generator=g) - 0.3
    span = window_L * window_L if window_L > 0 else Hk * Wk
    idx = torch.randint(0, len(slot_frame) * span, (Hq * Wq, topk), generator=g)
    idx = idx.masked_fill(torch.rand(Hq * Wq, topk, generator=g) < empty, -1)
    if window_L > 0:
        # Random taps alone miss a border now and then (topk 1 on the 5 x 33 grid leaves about 25 live taps per side column), so
        # the four corner queries each get their window's outermost corner tap, in the first and the last slot: every case then
        # has a live tap above, below, left and right of the image whatever the seed.
        last, L = (len(slot_frame) - 1) * span, window_L
        idx[0, 0], idx[Wq - 1, 0] = 0, last + L - 1
        idx[(Hq - 1) * Wq, 0], idx[Hq * Wq - 1, 0] = L * (L - 1), last + span - 1
    weight = torch.rand(Hq * Wq, topk, generator=g)
    return labels, idx.int(), weight


def propagate_restated(labels, slot_frame, idx, weight, Hq, Wq, Hk, Wk, window_L=0):
    """Plain float64 gather-sum out[q][p] = sum_r w[q][r] * labels[slot_frame[slot]][pixel][p]; for window_L > 0 the candidate is a tap
    of local_attention's window (tests/window_cases.py::coord_of_lists has the same arithmetic): pixel (qy + tap // L - R,
    qx + tap % L - R), contributing 0 outside the image (F.unfold zero padding).  Returns (out (HqWq, P), sum_r |w v| (HqWq, P))."""
    S, k = idx.shape
    span = window_L * window_L if window_L > 0 else Hk * Wk
    id_ = idx.long().clamp_min(0)
    slot, pix = id_ // span, id_ % span
    ok = idx >= 0
    if window_L > 0:
        R = window_L // 2
        q = torch.arange(S).view(S, 1)
        ky, kx = q // Wq + pix // window_L - R, q % Wq + pix % window_L - R
        ok = ok & (ky >= 0) & (ky < Hk) & (kx >= 0) & (kx < Wk)
        pix = (ky * Wk + kx).clamp(0, Hk * Wk - 1)
    frame = torch.as_tensor(slot_frame).long()[slot]
    v = labels.double()[frame, pix]                                                 # (S, k, P)
    wv = torch.where(ok, weight.double(), torch.zeros_like(weight, dtype=torch.float64)).unsqueeze(-1) * v
    return wv.sum(1), wv.abs().sum(1)


# ----------------------------------------------------------------------------------------------------------------------
# Gaussian labels, normalise, BN
# ----------------------------------------------------------------------------------------------------------------------
def gauss_points(case, seed=0):
    """(P, 2) f32 points of one GAUSS case on the image grid (Hf * stride x Wf * stride): inside, outside the image, and (from the second
    point on, cyclically) at least 40 sigma away, where the label underflows to a subnormal or to 0."""
    Hf, Wf, stride, P, sigma = case
    g = _gen(6000 + seed + Hf + P)
    h, w = Hf * stride, Wf * stride
    pts = torch.rand(P, 2, generator=g) * torch.tensor([w - 1.0, h - 1.0])
    if P >= 2:
        pts[1] = torch.tensor([w + 40.0 * sigma + 3.3, h * 0.5])                  # >= 40 sigma from every pixel: arg >= 800, the label is 0
    if P >= 3:
        pts[2] = torch.tensor([-7.25, h * 0.3])                                   # outside
    if P >= 4:
        pts[3] = torch.tensor([w * 0.4, -13.0 * sigma])                           # arg >= 84.5: the far rows are subnormal (exp(-87.3) = 2^-126)
    if P == 1:
        pts[0] = torch.tensor([-2.5, h + 2.0])                                    # one point: outside; the far rows subnormal, then 0
    return pts.float()


def normalize_input(case):
    """(n, C, H, W) f32 with, where the shape has the pixels: pixel 0 all zero, pixel 1 of 1e-20-sized values (norm below eps: divided
    by eps), pixel 2 of 1e-9-sized values (norm above eps)."""
    n, C, H, W = case
    g = _gen(7000 + C + H * W)
    x = torch.randn(n, C, H * W, generator=g)
    if H * W >= 3:
        x[:, :, 0] = 0.0
        x[:, :, 1] *= 1e-20
        x[:, :, 2] *= 1e-9
    return x.reshape(n, C, H, W).contiguous()


def normalize_restated(x, Cout=None):
    """(n, HW, Cout) float64: x / max(||x||, 1e-12) over the channels, channels last, zero padding channels."""
    n, C = x.shape[:2]
    xd = x.double().reshape(n, C, -1)
    y = (xd / xd.norm(dim=1, keepdim=True).clamp_min(1e-12)).permute(0, 2, 1)
    return y if Cout in (None, C) else F.pad(y, (0, Cout - C))


def bn_inputs(shape, seed=0):
    N, C, H, W = shape
    g = _gen(8000 + seed + C + H)
    x, res = torch.randn(N, C, H, W, generator=g), torch.randn(N, C, H, W, generator=g)
    mean, var = torch.randn(C, generator=g) * 0.5, torch.rand(C, generator=g) * 1.5 + 0.5
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    return x, res, mean, var, gamma, beta


def bn_restated(x, res, mean, var, gamma, beta, eps, relu):
    """y = (x - mean[c]) * rsqrt(var[c] + eps) * gamma[c] + beta[c] [+ residual] [max(., 0)] in float64 (csrc/post.hip), and the
    magnitude |x - m| * inv * |g| + |b| + |res| its bound is stated in."""
    v = lambda t: t.double().view(1, -1, 1, 1)
    inv = 1.0 / torch.sqrt(v(var) + eps)
    y = (x.double() - v(mean)) * inv * v(gamma) + v(beta)
    mag = (x.double() - v(mean)).abs() * inv * v(gamma).abs() + v(beta).abs()
    if res is not None:
        y, mag = y + res.double(), mag + res.double().abs()
    return (y.clamp_min(0) if relu else y), mag
