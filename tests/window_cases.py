"""Shapes, seeded inputs and float64 restatements shared by tests/test_gpu_window_ops.py (the HIP kernels of csrc/local.hip) and
tests/test_window_reference_share.py (the reference alone, on the CPU: how many queries of every case the strict list check holds
to the exact list).  No GPU code here: everything is a plain torch evaluation on the CPU.

Candidate ids: local window = slot * (2R+1)^2 + tap; c2f fine stage = t * (2Rf+1)^2 + tap.  A tap outside the image scores exactly 0
in the reference (F.unfold zero padding): tie class 1.  The same tap of one key frame held in two slots scores bit for bit the same:
tie class 2 + (frame, tap).  O.check_topk(structural=classes) then demands canonical order (score desc, id asc) among such ties.
"""
import torch
import torch.nn.functional as F

from oracle import fgvc_oracle as O

TEMP = 0.07
GAP = 1e-5
MIN_SHARE = 0.95          # a case may leave at most 5 % of its queries out of the exact list check

# (C, K, H, W, R, topk)
LOCAL_F32 = [(64, 1, 5, 33, 1, 5), (16, 1, 3, 4, 6, 16), (256, 2, 17, 23, 2, 10), (32, 3, 10, 12, 3, 6), (40, 4, 9, 7, 5, 16),
             (256, 7, 12, 20, 12, 10), (32, 2, 8, 8, 0, 1)]
LOCAL_F16X3 = [(256, 2, 17, 23, 2, 10), (256, 7, 12, 20, 12, 10)]
LOCAL_TIES = [(64, 2, 7, 9, 3, 10), (256, 2, 9, 11, 2, 10)]                 # the second also runs on the f16x3 route
# Key rows that are all zero (a dead pixel after the ReLU) score exactly 0 INSIDE the image and reach local_merge_slot with the pair list,
# i.e. BEFORE the padded taps -- the one place in local.hip where the id clause of TopK::accepts decides (everywhere else equal scores
# arrive in ascending id order).  Built so that the canonical answer is unambiguous: no live key scores above 0 (query >= 0, keys <= 0), and
# with H = R = 3 the whole first window row of every query is padding, so the canonical top-k is the padded taps 0..k-1 whichever dead
# pixels the pair kernel listed (among in-image exact ties it keeps arrival order, as common.hpp documents for TopKF).
LOCAL_ZERO_ROWS = [(32, 2, 3, 9, 3, 1), (32, 2, 3, 9, 3, 5)]
PLAN_SHAPE = (32, 3, 9, 11, 3)                                               # C, key frames (= pairs), H, W, R
PLAN_ROWS = [[0, 1, 2], [0, -1, 2], [0, 7, 1], [1, 1, 0], [2, -1, -1]]       # -1 slot, pair id >= n_pairs, a pair twice, a single slot
PLAN_TOPK = [1, 5, 10, 16]
# (C, H, W, R, topk, scale): border-heavy windows (R >= min(H, W)); the last: fewer candidates than topk, the list ends in -1
COORD = [(32, 5, 7, 5, 6, 1), (16, 3, 4, 6, 16, 4), (32, 4, 9, 4, 5, 8), (32, 6, 6, 0, 3, 4)]

# (Cf, T, H, W, scale, Rf, topk)
C2F_SWEEP = [(48, 1, 6, 9, 4, 1, 5), (512, 2, 5, 7, 2, 2, 16), (16, 1, 9, 13, 4, 1, 9), (256, 2, 5, 7, 4, 3, 10), (12, 2, 9, 13, 4, 3, 5),
             (24, 3, 7, 11, 2, 2, 10), (4, 3, 9, 13, 4, 6, 16), (8, 2, 9, 13, 3, 3, 1), (16, 1, 9, 13, 4, 0, 1)]
# name -> ((Cf, T, H, W, scale, Rf, topk), P, forced coarse cells)
C2F_EXTRA = {"scale1": ((16, 2, 9, 13, 1, 2, 5), 3, False), "P70_second_pl_trip": ((32, 2, 6, 9, 2, 2, 5), 70, False),
             "forced_corner_edge_rowcoop": ((16, 2, 7, 9, 2, 10, 10), 3, True), "forced_corner_edge_fallback": ((24, 2, 7, 9, 2, 10, 10), 3, True)}
C2F_TIES = {"rowcoop_Cf16": (16, 2, 7, 9, 4, 2, 10), "fallback_Cf12": (12, 2, 7, 9, 4, 2, 10), "rowcoop_Cf256": (256, 2, 5, 6, 2, 1, 5)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def case_id(shape):
    return "x".join(str(v) for v in shape)


# ----------------------------------------------------------------------------------------------------------------------
# local window
# ----------------------------------------------------------------------------------------------------------------------
def local_inputs(shape, seed=0, P=3, twin=False, zero_rows=False):
    """query (C,H,W), keys (K,C,H,W), values (K,P,H,W); twin: every key slot holds key frame 0; zero_rows: query >= 0, keys <= 0, 40 % of
    the pixels of key frame 0 and every pixel of the later frames have all-zero features."""
    C, K, H, W, R, topk = shape
    g = _gen(1000 + seed + C + 7 * H + 13 * W)
    q = torch.randn(C, H, W, generator=g)
    keys = torch.randn(K, C, H, W, generator=g)
    vals = torch.rand(K, P, H, W, generator=g)
    if twin:
        keys = keys[:1].expand(K, -1, -1, -1).contiguous()
    if zero_rows:
        q, keys = q.abs(), -keys.abs() * (torch.rand(1, 1, H, W, generator=g) < 0.6)
        keys[1:] = 0.0
    return q, keys, vals


def window_outside(H, W, R):
    """((2R+1)^2, HW) bool: tap of query lies outside the image."""
    L = 2 * R + 1
    return F.unfold(torch.ones(1, 1, H, W), kernel_size=L, padding=R).reshape(L * L, H * W) == 0


def local_slab(q, keys, R, temperature=TEMP, frames=None):
    """float64 logits (K*(2R+1)^2, HW) of the local window and their tie classes.  frames[s] = the key frame slot s holds (None: all
    different; -1: an empty slot, every candidate -inf).
    Tie class 1 = the out-of-image taps AND the in-image taps of all-zero key rows (both score exactly 0 in the reference).  CAVEAT for
    the second kind: fgvc_pair_topk_f32 keeps exact in-image ties in arrival order, not id order, so when more of them tie than a slot's
    pair list holds, the kernel's list is legitimate but not canonical.  Mark-as-class-1 is safe only for inputs whose canonical answer
    never depends on WHICH in-image zeros are listed (LOCAL_ZERO_ROWS is built that way); any other case with dead key pixels must
    not expect the exact list on those queries."""
    K, C, H, W = keys.shape
    LL = (2 * R + 1) ** 2
    corr = O.local_corr(q.double(), keys.double(), R).reshape(K, LL, H * W) / temperature
    out = window_outside(H, W, R)
    L = 2 * R + 1
    dead = (keys.abs().sum(1, keepdim=True) == 0).float()                                     # (K,1,H,W) all-zero key rows: score exactly 0 too
    dead = F.unfold(dead, kernel_size=L, padding=R).reshape(K, LL, H * W) == 1
    if frames is None:
        frames = list(range(K))
        dense = corr
    else:
        dense = torch.stack([corr[f] if f >= 0 else torch.full_like(corr[0], O.NEG_INF) for f in frames], 0)
    tap = torch.arange(LL).view(LL, 1).expand(LL, H * W)
    cls = []
    for f in frames:
        c = torch.where(out | dead[f], torch.ones_like(tap), 2 + f * LL + tap) if f >= 0 else torch.zeros_like(tap)
        cls.append(c)
    return dense.reshape(len(frames) * LL, H * W), torch.stack(cls, 0).reshape(len(frames) * LL, H * W)


def plan_frames(row, n_pairs):
    return [p if 0 <= p < n_pairs else -1 for p in row]


def coord_of_lists(idx, weight, H, W, R, scale):
    """float64 restatement of get_coord's last step (vanilla_tracker.py:479-485) for GIVEN lists: idx (S,k) window candidates of one
    slot (-1: none), weight (S,k) -> (S,2) = sum_r w * (x, y) * scale of the tap's pixel, (0,0) for a tap outside the image."""
    L = 2 * R + 1
    S = H * W
    qy, qx = (torch.arange(S) // W).view(S, 1), (torch.arange(S) % W).view(S, 1)
    tap = idx.clamp_min(0) % (L * L)
    ky, kx = qy + tap // L - R, qx + tap % L - R
    ok = (idx >= 0) & (ky >= 0) & (ky < H) & (kx >= 0) & (kx < W)
    w = torch.where(ok, weight.double(), torch.zeros_like(weight, dtype=torch.float64))
    return torch.stack([(w * (kx * scale).double()).sum(1), (w * (ky * scale).double()).sum(1)], 1)


# ----------------------------------------------------------------------------------------------------------------------
# coarse-to-fine fine stage
# ----------------------------------------------------------------------------------------------------------------------
def c2f_inputs(shape, seed=0, P=3, twin=False):
    """coarse query (16,H,W) / key (16,T,H,W); UNIT-NORM f32 fine rows qfine (Cf,sH,sW) / kfine (Cf,T,sH,sW) (the kernel's operands:
    the float64 side takes these very numbers); value (P,T,sH,sW)."""
    Cf, T, H, W, scale, Rf, topk = shape
    g = _gen(2000 + seed + Cf + 7 * H + 13 * W + 31 * Rf)
    q = O.l2_normalize(torch.randn(16, H, W, generator=g), 0)
    key = O.l2_normalize(torch.randn(16, T, H, W, generator=g), 0)
    qfine = O.l2_normalize(torch.randn(Cf, H * scale, W * scale, generator=g), 0)
    kfine = O.l2_normalize(torch.randn(Cf, T, H * scale, W * scale, generator=g), 0)
    v = torch.rand(P, T, H * scale, W * scale, generator=g)
    if twin:
        key = key[:, :1].expand(-1, T, -1, -1).contiguous()
        kfine = kfine[:, :1].expand(-1, T, -1, -1).contiguous()
    return q, key, qfine, kfine, v


def border_cells(H, W):
    """the four corner cells first, then every other edge cell"""
    corners = [0, W - 1, (H - 1) * W, H * W - 1]
    edge = [y * W + x for y in range(H) for x in range(W) if (y in (0, H - 1) or x in (0, W - 1)) and y * W + x not in corners]
    return corners + edge


def forced_arg(T, H, W):
    cells = torch.tensor(border_cells(H, W))
    q = torch.arange(H * W)
    return torch.stack([cells[(q + 3 * t) % len(cells)] for t in range(T)], 0)


def c2f_slab(qfine, kfine, arg, H, W, scale, Rf, temperature=TEMP, twin=False):
    """float64 fine logits (T*(2Rf+1)^2, HW) for GIVEN coarse cells arg (T,HW) (local_attention.py:785-847), their tie classes, and the
    index (T, LL, HW) of every candidate's fine pixel (-1 outside the map)."""
    Cf, T = kfine.shape[:2]
    L = 2 * Rf + 1
    LL, HW = L * L, H * W
    sH, sW = H * scale, W * scale
    qf = qfine.double()[:, ::scale, ::scale].reshape(Cf, HW)
    tap = torch.arange(LL)
    cy, cx = (arg // W) * scale, (arg % W) * scale                                             # (T,HW)
    fy = cy.view(T, 1, HW) + (tap // L - Rf).view(1, LL, 1)
    fx = cx.view(T, 1, HW) + (tap % L - Rf).view(1, LL, 1)
    inside = (fy >= 0) & (fy < sH) & (fx >= 0) & (fx < sW)
    pix = torch.where(inside, fy * sW + fx, torch.full_like(fy, -1))                           # (T,LL,HW)
    kf = kfine.double().reshape(Cf, T, sH * sW)
    dense = torch.zeros(T, LL, HW, dtype=torch.float64)
    for t in range(T):
        rows = kf[:, t, pix[t].clamp_min(0).reshape(-1)].reshape(Cf, LL, HW)
        dense[t] = torch.where(inside[t], (rows * qf.view(Cf, 1, HW)).sum(0), torch.zeros(LL, HW, dtype=torch.float64)) / temperature
    frame = torch.zeros(T, dtype=torch.long) if twin else torch.arange(T)
    cls = torch.where(inside, 2 + frame.view(T, 1, 1) * LL + tap.view(1, LL, 1), torch.ones_like(pix))
    return dense.reshape(T * LL, HW), cls.reshape(T * LL, HW), pix


def c2f_out(dense, pix, v, topk, mode):
    """float64 output (P,HW) of the fine stage from its slab (local_attention.py:858-870)."""
    P, T = v.shape[:2]
    val, idx = O.topk_canonical(dense, topk)                                                   # (k,HW)
    w = val.softmax(0) if mode == "softmax" else val.clamp(min=0) ** 2
    LL = pix.shape[1]
    p = pix.reshape(T * LL, -1).gather(0, idx)                                                 # (k,HW) fine pixel or -1
    t = idx // LL
    vv = v.double().reshape(P, T, -1)
    g = vv[:, t.reshape(-1), p.clamp_min(0).reshape(-1)].reshape(P, *idx.shape)
    g = torch.where((p >= 0).unsqueeze(0), g, torch.zeros_like(g))
    return (g * w.unsqueeze(0)).sum(1), idx.t().contiguous(), val.t().contiguous()


def c2f_case(shape, P=3, forced=False, twin=False):
    """inputs + coarse cells (the oracle's own arg-max unless forced) + the float64 slab of one c2f case"""
    Cf, T, H, W, scale, Rf, topk = shape
    q, key, qfine, kfine, v = c2f_inputs(shape, P=P, twin=twin)
    if forced:
        arg = forced_arg(T, H, W)
    else:
        aff = O.corr_volume(q.double(), key.double(), TEMP, normalize=False).reshape(T, H * W, H * W)      # (:804-806), no mask
        arg = aff.argmax(1)                                                                     # (:837)
    dense, cls, pix = c2f_slab(qfine, kfine, arg, H, W, scale, Rf, twin=twin)
    return dict(q=q, key=key, qfine=qfine, kfine=kfine, v=v, arg=arg, dense=dense, cls=cls, pix=pix)


def share(dense, topk, cls):
    m = O.checkable_queries(dense, topk, GAP, cls)
    return float(m.float().mean())
