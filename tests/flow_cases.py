"""Contracts of the dense-flow kernels (fgvc_amd/csrc/flow.hip): float64 restatements in numpy and generators of the
synthetic window lists they are tested on.  No GPU, no torch.

The three restatements:
  * flow_from_lists_ref   fgvc_flow_from_lists_f32, every sum, quotient and interpolation in float64, with the error bound of the f32
                          kernel per pixel (docs/LAB_NOTES.md has the derivation);
  * warp_ref              fgvc_warp_f32 = the reference's Warp.forward (warp.py:55-82);
  * consistency_ref       fgvc_flow_consistency_f32 = the reference's occlusion_estimation (occlusion_estimation.py:95-177), with every
                          pixel's margin to its threshold.
Sampling coordinates are the one thing kept in float32: the reference computes them in float32 (warp.py:22-24, then grid_sample's
unnormalisation), IEEE single operations without contraction are reproducible, and numpy's float32 arrays perform exactly those.  The taps
are then weighted and summed in float64, so the kernel's distance from the restatement is the rounding of its products and sums alone.
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -24
MARGIN = 1e-4          # a threshold comparison closer than this in float64 is undecided
MASK_MARGIN = 1e-5     # |grid_sample(ones) - 0.9999| below this: the warp mask is undecided
F32 = np.float32


# ---- window lists -> flow ---------------------------------------------------------------------------------------------------------------
def synthetic_lists(rows, Hf, Wf, R, k, seed):
    """idx (rows, Hf*Wf, k) int32 and weight (rows, Hf*Wf, k) float32 in run_local_affinity's single-slot form.  Weights are positive and
    sum to 1 over a cell's k entries (a softmax's), so S <= 1 once taps drop out.  Every row holds: empty entries (-1, about one in seven),
    out-of-image taps (every border cell has some at R >= 1), cell 0 with only out-of-image taps when R >= 1 (S == 0), cell 1 all empty
    (S == 0), and the middle cell with one tap repeated k times."""
    rng = np.random.default_rng(seed)
    HW, L2 = Hf * Wf, (2 * R + 1) ** 2
    idx = rng.integers(0, L2, (rows, HW, k)).astype(np.int32)
    w = rng.random((rows, HW, k)) + 0.05
    weight = (w / w.sum(-1, keepdims=True)).astype(F32)
    idx[rng.random((rows, HW, k)) < 0.15] = -1
    idx[:, 0] = 0 if R >= 1 else -1                                   # tap (dy, dx) = (-R, -R) of the corner cell: outside
    idx[:, 1] = -1
    idx[:, HW // 2] = min(L2 - 1, L2 // 2 + 1)                        # a duplicate tap, k times
    return idx, weight


def flow_from_lists_ref(idx, weight, Hf, Wf, R, scale, size, pad=(0, 0), renorm=True):
    """-> flow (rows, 2, h, w) float64, valid (rows, h, w) uint8, bound (rows, h, w) float64 = 32 * 2^-24 * (A + P): A the largest
    sum |w_r coord_r| / S among the pixel's four cells, P the magnitude of the pixel's own (padded) coordinate."""
    rows, HW, k = idx.shape
    (h, w), (left, top) = size, pad
    L = 2 * R + 1
    q = np.arange(HW)
    qy, qx = (q // Wf)[None, :, None], (q % Wf)[None, :, None]
    tap = np.where(idx >= 0, idx, 0) % (L * L)
    ky, kx = qy + tap // L - R, qx + tap % L - R
    ok = (idx >= 0) & (ky >= 0) & (ky < Hf) & (kx >= 0) & (kx < Wf)
    wv = np.where(ok, weight.astype(np.float64), 0.0)
    S = wv.sum(-1)
    C = np.stack([(wv * kx * scale).sum(-1), (wv * ky * scale).sum(-1)], -1)                  # (rows, HW, 2)
    A = np.hypot((np.abs(wv) * np.abs(kx * scale)).sum(-1), (np.abs(wv) * np.abs(ky * scale)).sum(-1))
    valid = S != 0
    Ss = np.where(valid, S, 1.0)
    own = np.stack([qx[..., 0] * scale, qy[..., 0] * scale], -1).astype(np.float64)           # (1, HW, 2)
    disp = np.where(valid[..., None], (C / Ss[..., None] if renorm else C) - own, 0.0)
    A = np.where(valid, A / Ss, 0.0)
    X, Y = np.arange(w) + left, np.arange(h) + top
    cx0, cy0 = np.minimum(X // scale, Wf - 1), np.minimum(Y // scale, Hf - 1)
    cx1, cy1 = np.minimum(cx0 + 1, Wf - 1), np.minimum(cy0 + 1, Hf - 1)                        # the upper neighbour is clamped
    fx, fy = ((X - cx0 * scale) / scale)[None, None, :, None], ((Y - cy0 * scale) / scale)[None, :, None, None]
    cell = lambda cy, cx: cy[:, None] * Wf + cx[None, :]                                       # (h, w) cell index
    i00, i01, i10, i11 = cell(cy0, cx0), cell(cy0, cx1), cell(cy1, cx0), cell(cy1, cx1)
    t = disp[:, i00] + fx * (disp[:, i01] - disp[:, i00])
    b = disp[:, i10] + fx * (disp[:, i11] - disp[:, i10])
    flow = (t + fy * (b - t)).transpose(0, 3, 1, 2)
    v = (valid[:, i00] & valid[:, i01] & valid[:, i10] & valid[:, i11]).astype(np.uint8)
    Amax = np.maximum(np.maximum(A[:, i00], A[:, i01]), np.maximum(A[:, i10], A[:, i11]))
    P = np.hypot(X[None, :], Y[:, None])[None]
    return flow, v, 32 * EPS * (Amax + P)


# ---- warp and the forward-backward check ------------------------------------------------------------------------------------------------------
def _taps(flow, align_corners):
    """The reference's sampling of output pixel (x, y) with flow (u, v), coordinates in float32 as it computes them.  flow (N, 2, H, W)
    float32 -> weights (N, 4, H, W) float64 (nw, ne, sw, se), flat tap indices (N, 4, H, W) int64 and in-plane flags (N, 4, H, W)."""
    flow = np.asarray(flow)
    assert flow.dtype == F32
    N, _, H, W = flow.shape
    xs, ys = np.arange(W, dtype=F32)[None, None, :], np.arange(H, dtype=F32)[None, :, None]
    dw, dh = F32(max(W - 1, 1)), F32(max(H - 1, 1))
    gx = (xs + flow[:, 0]) * F32(2) / dw - F32(1)                         # warp.py:22-24
    gy = (ys + flow[:, 1]) * F32(2) / dh - F32(1)
    if align_corners:                                                     # grid_sample's unnormalisation
        ix, iy = (gx + F32(1)) / F32(2) * F32(W - 1), (gy + F32(1)) / F32(2) * F32(H - 1)
    else:
        ix, iy = ((gx + F32(1)) * F32(W) - F32(1)) / F32(2), ((gy + F32(1)) * F32(H) - F32(1)) / F32(2)
    assert ix.dtype == F32 and iy.dtype == F32
    xa, ya = np.floor(ix), np.floor(iy)
    ix, iy, xa, ya = (a.astype(np.float64) for a in (ix, iy, xa, ya))
    xb, yb = xa + 1, ya + 1
    wts = np.stack([(xb - ix) * (yb - iy), (ix - xa) * (yb - iy), (xb - ix) * (iy - ya), (ix - xa) * (iy - ya)], 1)
    tx, ty = np.stack([xa, xb, xa, xb], 1), np.stack([ya, ya, yb, yb], 1)
    inside = (tx >= 0) & (tx <= W - 1) & (ty >= 0) & (ty <= H - 1)
    at = np.where(inside, ty * W + tx, 0).astype(np.int64)
    return wts, at, inside


def warp_ref(feat, flow, align_corners=False, use_mask=True):
    """-> out (N, C, H, W) float64, ones (N, H, W) float64 = grid_sample of a plane of ones (the mask is ones > 0.9999), mag (N, C, H, W)
    float64 = sum_i |v_i w_i| over the in-plane taps: the f32 kernel stays within 7 * 2^-24 * mag of `out` (a weight product, a tap
    product and three sums; the mask multiplies by 1 or 0) wherever the mask is decided."""
    feat = np.asarray(feat, np.float64)
    N, C, H, W = feat.shape
    wts, at, inside = _taps(flow, align_corners)
    wts = np.where(inside, wts, 0.0)
    planes = feat.reshape(N, C, H * W)
    v = np.stack([np.take_along_axis(planes, np.broadcast_to(at[:, i].reshape(N, 1, H * W), (N, C, H * W)), 2) for i in range(4)], 2)
    v = v.reshape(N, C, 4, H, W)
    out, mag = (v * wts[:, None]).sum(2), np.abs(v * wts[:, None]).sum(2)
    ones = wts.sum(1)
    mask = (ones > 0.9999) if use_mask else np.ones_like(ones, bool)
    return out * mask[:, None], ones, mag


def consistency_ref(flow_fw, flow_bw, mode="consistency", diff=1.5):
    """One direction (own = flow_fw, other = flow_bw): occ (N, 1, H, W) float64 in {0, 1} and decided (N, 1, H, W) bool -- False where the
    float64 margin to the threshold is below MARGIN or the warp mask's below MASK_MARGIN.  Quirks of the reference kept
    (occlusion_estimation.py): Warp() with align_corners=False whatever warp_cfg says (:108, :135); sum_sq = sum(own * 2 + warped^2), a
    product by two (:114-115)."""
    own = np.asarray(flow_fw, np.float64)
    warped, ones, _ = warp_ref(flow_bw, flow_fw, False, True)
    sq = ((own + warped) ** 2).sum(1, keepdims=True)
    if mode == "consistency":
        rhs = (own * 2 + warped ** 2).sum(1, keepdims=True) * 0.01 + 0.5
        lhs = sq
    elif mode == "fb_abs":
        lhs, rhs = np.sqrt(sq), np.full_like(sq, float(diff))
    else:
        raise ValueError(mode)
    decided = (np.abs(lhs - rhs) >= MARGIN) & (np.abs(ones[:, None] - 0.9999) >= MASK_MARGIN)
    return (lhs < rhs).astype(np.float64), decided


def consistency_both_ref(flow_fw, flow_bw, mode="consistency", diff=1.5):
    """Both directions, as the kernel returns them: occ_fw, occ_bw, decided_fw, decided_bw."""
    of, df = consistency_ref(flow_fw, flow_bw, mode, diff)
    ob, db = consistency_ref(flow_bw, flow_fw, mode, diff)
    return of, ob, df, db


def smooth_field(shape_nchw, seed, amp, coarse=5):
    """(N, C, H, W) float32: bicubic-like smooth field -- a coarse normal grid of amplitude `amp` upsampled with separable cubic
    (Catmull-Rom) interpolation in float64."""
    N, C, H, W = shape_nchw
    rng = np.random.default_rng(seed)
    g = rng.standard_normal((N, C, coarse + 3, coarse + 3)) * amp

    def up(a, n, axis):
        t = np.linspace(1.0, a.shape[axis] - 2.0 - 1e-9, n)
        i, f = np.floor(t).astype(int), t - np.floor(t)
        p = [np.take(a, i + d, axis) for d in (-1, 0, 1, 2)]
        sh = [1] * a.ndim
        sh[axis] = n
        f = f.reshape(sh)
        return 0.5 * (2 * p[1] + (p[2] - p[0]) * f + (2 * p[0] - 5 * p[1] + 4 * p[2] - p[3]) * f * f + (3 * p[1] - p[0] - 3 * p[2] + p[3]) * f ** 3)

    return up(up(g, H, 2), W, 3).astype(F32)


# ---- a synthetic feature bank with a known shift ----------------------------------------------------------------------------------------------
def shifted_bank(T, Hf, Wf, C, seed, shift=(2, -1)):
    """(T, Hf*Wf, C) float32: frame 0 holds unit-norm random rows; frame t is frame 0 moved by t * shift = (dx, dy) cells, fresh unit-norm
    random rows filling in what moved into view."""
    rng = np.random.default_rng(seed)

    def rows(n):
        a = rng.standard_normal((n, C))
        return a / np.linalg.norm(a, axis=1, keepdims=True)

    f0 = rows(Hf * Wf).reshape(Hf, Wf, C)
    out = [f0]
    ys, xs = np.mgrid[0:Hf, 0:Wf]
    for t in range(1, T):
        f = rows(Hf * Wf).reshape(Hf, Wf, C)
        sy, sx = ys - shift[1] * t, xs - shift[0] * t
        ok = (sy >= 0) & (sy < Hf) & (sx >= 0) & (sx < Wf)
        f[ok] = f0[sy[ok], sx[ok]]
        out.append(f)
    return np.stack(out).reshape(T, Hf * Wf, C).astype(F32)


def largest_off_match_cosine(bank, Hf, Wf, R, step, shift=(2, -1)):
    """The largest cosine, in float64, between a query row and any row of its window in the paired frame other than its true match, over
    every forward and backward pair `step` apart and every query."""
    b = bank.astype(np.float64)
    q = np.arange(Hf * Wf)
    qy, qx = q // Wf, q % Wf
    win = (np.abs(qy[:, None] - qy[None]) <= R) & (np.abs(qx[:, None] - qx[None]) <= R)
    c = -1.0
    for g in range(b.shape[0] - step):
        for a, k, s in ((g, g + step, 1), (g + step, g, -1)):
            cos = b[a] @ b[k].T
            my, mx = qy + s * shift[1] * step, qx + s * shift[0] * step
            match = (qy[None] == my[:, None]) & (qx[None] == mx[:, None])
            c = max(c, float(cos[win & ~match].max()))
    return c
