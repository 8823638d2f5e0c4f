"""Case builder, `delta` patterns and a plain restatement of the refining merge's rule (csrc/refine.hip: fgvc_merge_refine_topk_f32),
shared by tests/test_gpu_refine_ops.py (the entry point on these lists) and tests/test_refine_reference_share.py (the restatement
against the oracle, on the CPU).  No GPU code here: numpy / torch on the CPU.

The kernel's correctness is a proof (header of refine.hip) from ONE assumption, |approximate - exact| <= eps for every candidate.
tests/test_gpu_refine.py feeds the merge the real f16 + FP6 pair kernel, whose error is a third of eps: nothing there comes near the
boundary the proof is about.  Here the pair lists are built on the host, with the approximate scores pushed to the boundary on purpose.

A case: f32 rows (frames, HW, 256); dot64 = float64 product of every (query, key) under the mask; s32 = float32(dot64) is the EXACT
score the kernel is specified to produce (products and sums in f64, one rounding); the approximate score is a = float32(s32 + delta);
a slot's list is the top-kin by (a desc, pixel asc) of the candidates under the mask, its tail -1 / -inf.  Two slots fed by the same
key frame read ONE list (one pair): twins.

The margin.  `delta` is limited to |delta| <= eps - MARGIN, eps = the f32 the kernel is handed.  Two roundings stand between that and
the proof's real-number statements, both for scores below 2 in size (asserted), where half a unit of an f32 is at most 2^-24:
  * a = f32(s32 + delta):  |a - s32| <= eps - MARGIN + 2^-24 (<= eps: the contract the builder asserts on every candidate);
  * thr = f32(t_k - 2 eps): at most 2^-24 above the real t_k - 2 eps (2 eps itself is exact in f32, so a fused t_k - 2 eps rounds the same).
  A candidate the kernel leaves outside the window has a < thr <= t_k - 2 eps + 2^-24, so its exact score is
  s <= a + eps - MARGIN + 2^-24 < t_k - eps - MARGIN + 2^-23, while each of the k entries at or above t_k has
  s_j >= t_k - (eps - MARGIN + 2^-24).  The first stays strictly below the second when 2 MARGIN >= 2^-23 + 2^-24, i.e. MARGIN >= 0.75 * 2^-23.
  * The cluster test f32(a_j - a_j+1) <= 2 eps needs no margin of its own: rounding is monotone and 2 eps is an f32, so the rounded
  difference exceeds 2 eps exactly when the real one does; then s_j - s_j+1 > 2 eps - 2 (eps - MARGIN + 2^-24) = 2 MARGIN - 2^-23 >= 0
  needs MARGIN >= 2^-24 for a strict order.
MARGIN = 2^-23 covers both.  The dyadic cases have no rounding anywhere (every dot product, every a, every difference is exact in f32):
their margin is 0 and `delta` reaches +-eps itself; an excluded candidate is then a < thr strictly, s <= a + eps < t_k - eps <= s_j.

Masks are written as the kernel takes them (r2max, ry, rx): keep <=> dy^2 + dx^2 <= r2max and |dy| <= ry and |dx| <= rx.  R2_NR30 = 224
is the product's disc (neighbor_range 30: sqrt(d2) < 15 in f32), R2_NR12 = 35 (sqrt(d2) < 6).
"""
import functools
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch

TEMP = 0.07
NO_LIMIT = 0x3FFFFFFF
PAIR_MASKED = 1
KX = 16                   # RF_KX: merged candidates kept per query
KMAX = 10                 # RF_KMAX
MARGIN = 2.0 ** -23
MIN_SHARE = 0.95
GUARD = 4096              # elements in front of and behind every output view
R2_NR30, R2_NR12 = 224, 35
PATHS = ("final", "rescored", "scratch_some", "scratch_all")
NINF = float("-inf")
DYADIC_CH, DYADIC_NZ, DYADIC_TOP = 16, 6, 8      # dyadic rows: non-zero channels among the first DYADIC_CH, values up to DYADIC_TOP / 16


@dataclass(frozen=True)
class Case:
    name: str
    grid: Tuple[int, int]                       # query grid (Hq, Wq)
    rows: Tuple[Tuple[int, ...], ...]           # per output row: the key frame of every slot (-1: unused); the query frame is frame n_key + row
    mask: Tuple[int, int, int]                  # (r2max, ry, rx)
    k: int
    kind: str                                   # gauss | neartie | smooth | dyadic | ladder
    eps: float
    pattern: str                                # zero | rand | alt | edge
    seed: int = 0
    kgrid: Optional[Tuple[int, int]] = None     # key grid when it differs (unmasked pairs only)
    masked: bool = True
    floors: Tuple[Tuple[str, int], ...] = ()    # (path, least number of queries the case must send down it)


def _disc(r2):
    return (r2, NO_LIMIT, NO_LIMIT)


def _square(nr):
    return (NO_LIMIT, nr // 2, nr // 2)


# Floors: well below the counts measured on the CPU (tests/test_refine_reference_share.py prints them; docs/LAB_NOTES.md has the table).
CASES = [
    Case("c01_gauss_alt", (9, 11), ((0, 1),), _disc(R2_NR30), 10, "gauss", 2e-5, "alt", 1, floors=(("final", 50),)),
    Case("c02_neartie_alt_some_open", (9, 11), ((0, 1),), _disc(R2_NR30), 10, "neartie", 2e-5, "alt", 28,
         floors=(("rescored", 30), ("scratch_some", 10))),
    Case("c03_twins_neartie_edge", (9, 11), ((0, 0, 1),), _disc(R2_NR30), 10, "neartie", 2e-5, "edge", 33,
         floors=(("rescored", 30), ("scratch_some", 5), ("scratch_all", 1))),
    Case("c03_triple_twins", (9, 11), ((0, 0, 0, 1),), _disc(R2_NR30), 10, "neartie", 2e-5, "edge", 35,
         floors=(("rescored", 30), ("scratch_some", 5), ("scratch_all", 8))),
    Case("c04_wide_eps_over16_in_window", (9, 11), ((0, 1, 2),), _disc(R2_NR30), 10, "gauss", 5e-3, "alt", 4,
         floors=(("scratch_all", 2), ("rescored", 30))),
    Case("c05_all_from_scratch", (9, 11), ((0, 1, 2, 3),), _disc(R2_NR30), 10, "gauss", 2e-2, "rand", 5, floors=(("scratch_all", 99),)),
    Case("c06_k5_insertion_square", (9, 11), ((0, 1, 2),), _square(4), 5, "gauss", 2e-3, "edge", 6,
         floors=(("final", 3), ("rescored", 30), ("scratch_some", 2))),
    Case("c07_k7", (9, 11), ((0, 1, 2),), _disc(8), 7, "neartie", 2e-5, "rand", 7, floors=(("rescored", 30), ("scratch_some", 8))),
    Case("c08_short_lists_ragged_workgroup", (5, 33), ((0, 0, 1, 2),), _disc(2), 10, "neartie", 2e-5, "edge", 8, floors=(("rescored", 60), ("scratch_all", 3))),
    Case("c09_one_candidate_k10", (3, 4), ((0,),), _disc(0), 10, "gauss", 2e-5, "rand", 9, floors=(("final", 12),)),
    Case("c09_one_candidate_k1", (3, 4), ((0,),), _disc(0), 1, "gauss", 2e-5, "rand", 9, floors=(("scratch_all", 12),)),
    Case("c10_product_layout_two_rows", (17, 23), ((0, 0, 1, 2, 3, 4), (0, 1, 2, 3, 4, -1)), _disc(R2_NR12), 10, "neartie", 2e-5, "alt", 10,
         floors=(("rescored", 300), ("scratch_some", 12), ("scratch_all", 1))),
    Case("c11_dyadic_alt", (9, 11), ((0, 0, 1, 2),), _disc(R2_NR30), 10, "dyadic", 2.0 ** -6, "alt", 11,
         floors=(("rescored", 15), ("scratch_all", 15))),
    Case("c11_dyadic_edge", (9, 11), ((0, 0, 1, 2),), _disc(8), 10, "dyadic", 2.0 ** -6, "edge", 12,
         floors=(("rescored", 15), ("scratch_all", 15))),
    Case("c11_dyadic_rand_k7", (9, 11), ((0, 1),), _disc(R2_NR30), 7, "dyadic", 2.0 ** -6, "rand", 13,
         floors=(("rescored", 15), ("scratch_some", 15), ("scratch_all", 2))),
    # two DIFFERENT key frames whose scores at one pixel are exactly 2 eps apart, the lower slot's below: `alt` makes their approximate
    # scores equal, every such pair stands alone (8 eps to the next), k = 5 cuts one in two.  Same pixel, equal score, NOT twins.
    Case("c11_ladder_equal_scores_not_twins", (9, 11), ((0, 1),), _disc(2), 5, "ladder", 2.0 ** -6, "alt", 0, floors=(("rescored", 99),)),
    Case("c12_eps_zero_twins", (9, 11), ((0, 0, 1),), _disc(R2_NR30), 10, "gauss", 0.0, "zero", 14, floors=(("final", 90),)),
    Case("c13_mostly_final_sampled", (34, 32), ((0, 0, 1),), _disc(R2_NR12), 10, "gauss", 2e-5, "rand", 19, floors=(("final", 1001),)),
    Case("c15_unmasked_unequal_grids", (5, 7), ((0, 1, 1),), (NO_LIMIT, NO_LIMIT, NO_LIMIT), 10, "neartie", 2e-5, "alt", 15,
         kgrid=(6, 9), masked=False, floors=(("rescored", 10), ("scratch_some", 4))),
    Case("c15_unmasked_all_open", (5, 7), ((0, 1),), (NO_LIMIT, NO_LIMIT, NO_LIMIT), 10, "gauss", 2e-2, "rand", 16,
         kgrid=(6, 9), masked=False, floors=(("scratch_all", 35),)),
]
# 66 x 64 = 4224 queries against a scan queue of 4096: 128 from-scratch items recomputed inside the refine kernel (RF_INLINE), every one
# with two slots.  Square 2 is a 3 x 3 window (4 candidates in a corner); k = 4 makes every list full -- a corner's list holds ALL its
# candidates and is full at once -- so with eps far above the scores' spread every slot's own last entry is inside the window.
OVERFLOW = Case("c16_beyond_the_scan_queue", (66, 64), ((0, 1),), _square(2), 4, "gauss", 0.5, "rand", 17, floors=(("scratch_all", 4224),))
# CPU only: smooth rows reach logits of 14, outside the range the post module's weight bound is derived for
CPU_ONLY = [Case("smooth_alt", (9, 11), ((0, 1, 2),), _disc(R2_NR30), 10, "smooth", 2e-5, "alt", 18, floors=(("final", 1),))]
BY_NAME = {c.name: c for c in CASES + [OVERFLOW] + CPU_ONLY}


def case_id(c):
    return c.name if isinstance(c, Case) else str(c)


# ----------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------
def feats(kind, n, H, W, seed):
    """(n, H * W, 256) f32 rows.  gauss / neartie / smooth as _feats of tests/test_gpu_refine.py, unit norm (normalised in f64, rounded
    once); dyadic: six non-zero channels of the first sixteen per row, multiples of 2^-4 up to 8 * 2^-4 in size, NOT normalised;
    ladder: channel 0 only -- every query row is 1, key frame 0 holds 2^-3 (1 + 3 (y mod 3) + x mod 3) (distinct inside any 3 x 3 window),
    key frame f the same + f 2^-5: a score IS the key's value."""
    g = torch.Generator().manual_seed(seed)
    if kind == "ladder":
        x = np.zeros((n, H * W, 256), np.float32)
        yy, xx = np.divmod(np.arange(H * W), W)
        for f in range(n - 1):
            x[f, :, 0] = (1 + 3 * (yy % 3) + xx % 3) / 8.0 + f / 32.0
        x[n - 1, :, 0] = 1.0
        return x
    if kind == "dyadic":
        r = np.random.default_rng(seed)
        x = np.zeros((n, H * W, 256), np.float32)
        for f in range(n):
            for p in range(H * W):
                ch = r.choice(DYADIC_CH, DYADIC_NZ, replace=False)
                x[f, p, ch] = r.integers(1, DYADIC_TOP + 1, DYADIC_NZ) * r.choice([-1.0, 1.0], DYADIC_NZ) / 16.0
        return x
    x = torch.randn(n, 256, H, W, generator=g)
    if kind == "smooth":
        x = torch.nn.functional.avg_pool2d(torch.randn(n, 256, H + 6, W + 6, generator=g), 7, 1) + 0.05 * x
    elif kind == "neartie":
        base = torch.randn(n, 256, (H + 1) // 2, (W + 1) // 2, generator=g)
        x = base.repeat_interleave(2, 2).repeat_interleave(2, 3)[:, :, :H, :W] + 2e-5 * x
    elif kind != "gauss":
        raise ValueError(kind)
    x = x.double()
    x = x / x.norm(dim=1, keepdim=True)
    return x.flatten(2).permute(0, 2, 1).contiguous().float().numpy()


def mask_matrix(Hq, Wq, Hk, Wk, mask, masked):
    """(HWk, HWq) bool: the kernel's predicate on offsets key - query; all true for an unmasked pair"""
    if not masked:
        return np.ones((Hk * Wk, Hq * Wq), bool)
    assert (Hq, Wq) == (Hk, Wk)
    r2max, ry, rx = mask
    ky, kx = np.divmod(np.arange(Hk * Wk), Wk)
    qy, qx = np.divmod(np.arange(Hq * Wq), Wq)
    dy, dx = ky[:, None] - qy[None, :], kx[:, None] - qx[None, :]
    return (dy * dy + dx * dx <= r2max) & (np.abs(dy) <= ry) & (np.abs(dx) <= rx)


def near_f32_midpoint(x, tol=1e-12):
    """x (f64 array): within `tol` of the midpoint of two neighbouring f32 -- where the f32 rounding of an f64 sum depends on its last bits"""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(np.where(x == 0, 1.0, x))
    ulp = np.ldexp(1.0, np.maximum(e - 24, -149))
    r = x / ulp
    return np.abs(r - np.floor(r) - 0.5) * ulp < tol


# ----------------------------------------------------------------------------------------------------------------------
# the case builder
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    case: Case
    eps: float                    # the f32 the kernel is handed, as a Python float
    q_rows: np.ndarray            # (frames, HWq, 256) f32; the same array as k_rows on equal grids
    k_rows: np.ndarray
    pairs: np.ndarray             # (n_pairs, 4) int32: query frame, key frame, flags, 0
    slot_pair: np.ndarray         # (n_out, T) int32
    pair_idx: np.ndarray          # (n_pairs, HWq, k) int32
    pair_score: np.ndarray        # (n_pairs, HWq, k) f32
    s32: np.ndarray               # (n_pairs, HWk, HWq) f32: the exact scores
    a: np.ndarray                 # (n_pairs, HWk, HWq) f32: the approximate ones
    dot64: np.ndarray
    ok: np.ndarray                # (n_pairs, HWk, HWq) bool
    held: np.ndarray = field(default=None)       # (n_out, HWq) bool


def check_contract(b: "Built"):
    """|a - s32| <= eps on EVERY candidate under the mask: what the proof in refine.hip assumes"""
    err = np.abs(b.a.astype(np.float64) - b.s32.astype(np.float64))[b.ok]
    assert err.size and float(err.max()) <= b.eps, (b.case.name, float(err.max()), b.eps)
    return float(err.max())


def build(case: Case, delta_scale: float = 1.0) -> Built:
    Hq, Wq = case.grid
    Hk, Wk = case.kgrid or case.grid
    HWq, HWk, k = Hq * Wq, Hk * Wk, case.k
    n_out, T = len(case.rows), len(case.rows[0])
    assert all(len(r) == T for r in case.rows) and 1 <= k <= KMAX and T <= 16
    n_key = 1 + max(max(r) for r in case.rows)
    if case.kgrid is None:
        k_rows = q_rows = feats(case.kind, n_key + n_out, Hq, Wq, case.seed)
        qf_of = [n_key + r for r in range(n_out)]
    else:
        k_rows, q_rows = feats(case.kind, n_key, Hk, Wk, case.seed), feats(case.kind, n_out, Hq, Wq, case.seed + 1000)
        qf_of = list(range(n_out))
    pairs, slot_pair, where = [], np.full((n_out, T), -1, np.int32), {}
    for r, slots in enumerate(case.rows):
        for t, kf in enumerate(slots):
            if kf < 0:
                continue
            if (r, kf) not in where:
                where[(r, kf)] = len(pairs)
                pairs.append((qf_of[r], kf, PAIR_MASKED if case.masked else 0, 0))
            slot_pair[r, t] = where[(r, kf)]
    pairs = np.array(pairs, np.int32)
    n_pairs = len(pairs)
    ok1 = mask_matrix(Hq, Wq, Hk, Wk, case.mask, case.masked)
    dot64 = np.stack([k_rows[kf].astype(np.float64) @ q_rows[qf].astype(np.float64).T for qf, kf, _, _ in pairs])     # (n_pairs, HWk, HWq)
    s32 = dot64.astype(np.float32)
    ok = np.broadcast_to(ok1, dot64.shape)
    eps = float(np.float32(case.eps))
    dyadic = case.kind in ("dyadic", "ladder")                    # exact arithmetic
    lim = eps if dyadic else max(eps - MARGIN, 0.0)
    # exact ranks in the merged order (s32 desc, gid = slot * HWk + pixel asc) of each output row; a pair in two slots takes its first slot's
    delta = np.zeros(dot64.shape)
    rng = np.random.default_rng(case.seed + 77)
    for r in range(n_out):
        sl = [t for t in range(T) if slot_pair[r, t] >= 0]
        slab = np.concatenate([np.where(ok1, s32[slot_pair[r, t]], -np.inf) for t in sl], 0)                          # (len(sl) * HWk, HWq)
        order = np.argsort(-slab, axis=0, kind="stable")
        rank = np.empty_like(order)
        np.put_along_axis(rank, order, np.broadcast_to(np.arange(slab.shape[0])[:, None], slab.shape), 0)
        seen = set()
        for i, t in enumerate(sl):
            pid = int(slot_pair[r, t])
            if pid in seen:
                continue
            seen.add(pid)
            rk = rank[i * HWk:(i + 1) * HWk]
            if case.pattern == "zero":
                d = np.zeros(rk.shape)
            elif case.pattern == "rand":
                d = np.round(rng.uniform(-1, 1, rk.shape) * 16) / 16 * lim if dyadic else rng.uniform(-lim, lim, rk.shape)
            elif case.pattern == "alt":
                d = np.where(rk % 2 == 0, -lim, lim)
            elif case.pattern == "edge":
                d = np.where(rk < k, -lim, lim)
            else:
                raise ValueError(case.pattern)
            delta[pid] = d
    a = (s32.astype(np.float64) + delta_scale * delta).astype(np.float32)
    if dyadic:      # exact arithmetic: nothing was rounded
        assert np.array_equal(s32.astype(np.float64), dot64) and np.array_equal(a.astype(np.float64), s32.astype(np.float64) + delta_scale * delta)
        assert eps == 2.0 ** -6 and np.array_equal(delta * 1024, np.round(delta * 1024))
    else:
        assert float(np.abs(a[ok]).max()) < 2.0 and float(np.abs(s32[ok]).max()) < 2.0               # the margin's derivation assumes it
    # the lists: per pair the top-k by (a desc, pixel asc) under the mask
    am = np.where(ok, a, -np.inf)
    order = np.argsort(-am, axis=1, kind="stable")[:, :k]                                            # (n_pairs, k, HWq)
    sc = np.take_along_axis(am, order, 1)
    if order.shape[1] < k:
        pad = k - order.shape[1]
        order = np.concatenate([order, np.zeros((n_pairs, pad, HWq), order.dtype)], 1)
        sc = np.concatenate([sc, np.full((n_pairs, pad, HWq), -np.inf, sc.dtype)], 1)
    pair_idx = np.where(np.isfinite(sc), order, -1).astype(np.int32).transpose(0, 2, 1).copy()
    pair_score = sc.astype(np.float32).transpose(0, 2, 1).copy()
    b = Built(case, eps, q_rows, k_rows, pairs, slot_pair, pair_idx, pair_score, s32, a, dot64, ok)
    check_contract(b)
    # held: none of the first k + 1 float64 dot products (merged order) within 1e-12 of an f32 rounding midpoint
    held = np.ones((n_out, HWq), bool)
    for r in range(n_out):
        sl = [t for t in range(T) if slot_pair[r, t] >= 0]
        slab = np.concatenate([np.where(ok1, dot64[slot_pair[r, t]], -np.inf) for t in sl], 0)
        top = -np.sort(-slab, axis=0)[:k + 1]
        fin = np.isfinite(top)
        held[r] = ~(near_f32_midpoint(np.where(fin, top, 0.0)) & fin).any(0)
    b.held = held
    return b


@functools.lru_cache(maxsize=None)
def built(name: str) -> Built:
    """a case, built once and shared: the tests do not change it"""
    return build(BY_NAME[name])


def slab64(b: Built, r: int) -> torch.Tensor:
    """(T' * HWk, HWq) float64 slab of output row r holding s32 (the exact score the kernel is specified to produce), -inf outside
    the mask; the slots with a pair only (they come first in every case), a key frame in two slots twice"""
    sl = [t for t in range(b.slot_pair.shape[1]) if b.slot_pair[r, t] >= 0]
    assert sl == list(range(len(sl)))
    return torch.from_numpy(np.concatenate([np.where(b.ok[b.slot_pair[r, t]], b.s32[b.slot_pair[r, t]].astype(np.float64), -np.inf) for t in sl], 0))


# ----------------------------------------------------------------------------------------------------------------------
# the rule of refine.hip, restated
# ----------------------------------------------------------------------------------------------------------------------
def sample_hash(q: int, f: int) -> bool:
    """merge_mark_kernel's pseudo-random 1/64 of the queries (32-bit unsigned arithmetic)"""
    h = ((q * 2654435761) & 0xFFFFFFFF) ^ ((f * 0x9E3779B1) & 0xFFFFFFFF)
    return ((h >> 11) & 63) == 0


def restate_query(b: Built, f: int, q: int) -> dict:
    """One query of output row f by the header of refine.hip.  Scores are np.float32 wherever the kernel's f32 arithmetic decides."""
    k, HWk, sp = b.case.k, b.s32.shape[1], b.slot_pair[f]
    two_eps = np.float32(2.0) * np.float32(b.eps)                                # exact in f32
    listed, tau = [], {}                                                         # (a, gid) of every listed candidate; a full list's last entry per slot
    for t, pid in enumerate(sp):
        if pid < 0:
            continue
        ids, sc = b.pair_idx[pid, q], b.pair_score[pid, q]
        n = int((ids >= 0).sum())
        if n == k:
            tau[t] = float(sc[k - 1])                                            # nothing the pair kernel did not list scores above it
        listed += [(float(sc[j]), t * HWk + int(ids[j])) for j in range(n)]
    listed.sort(key=lambda e: (-e[0], e[1]))
    top = listed[:KX]                                                            # the 16 best listed by a
    drop_max = listed[KX][0] if len(listed) > KX else NINF                       # best listed candidate that is not among them
    t_k = top[k - 1][0] if len(top) >= k else NINF
    thr = float(np.float32(t_k) - two_eps)                                       # f32(t_k - f32(2 eps)); -inf stays -inf
    m = sum(1 for s, _ in top if s >= thr)                                       # the window: a prefix of the 16
    all_open = drop_max > NINF and drop_max >= thr                               # more listed candidates inside the window than the 16 kept
    open_slots = sorted(t for t, v in tau.items() if v >= thr)
    brute = all_open or bool(open_slots)
    s32_of = lambda gid: float(b.s32[sp[gid // HWk], gid % HWk, q])
    twin = [j + 1 < m and top[j][0] == top[j + 1][0] and top[j][1] % HWk == top[j + 1][1] % HWk and
            sp[top[j][1] // HWk] == sp[top[j + 1][1] // HWk] for j in range(KX - 1)]
    mask = set()
    for j in range(KX - 1):
        if j + 1 < m and not twin[j] and np.float32(top[j][0]) - np.float32(top[j + 1][0]) <= two_eps:
            mask |= {j, j + 1}
    for sweep in (range(KX - 1), range(KX - 2, -1, -1)):                          # a re-scored entry takes its twin along, both ways
        for j in sweep:
            if twin[j] and (j in mask or j + 1 in mask):
                mask |= {j, j + 1}
    out = dict(m=m, n_listed16=len(top), rescored=[], brute=brute, n_mask=0)
    if not brute and not mask:
        out["path"], ent = "final", [(s, g, False) for s, g in top[:k]]          # the order is proven as it stands
        out["sampled"] = sample_hash(q, f) and len(top) > 0
        out["sample_err"] = max([abs(s - s32_of(g)) for s, g in top] + [0.0])
    elif not brute:
        out["path"], out["n_mask"] = "rescored", len(mask)
        ent = [((s32_of(g), g, True) if j in mask else (s, g, False)) for j, (s, g) in enumerate(top[:m])]
        out["rescored"] = [(top[j][1], abs(top[j][0] - s32_of(top[j][1]))) for j in sorted(mask)]
    else:
        valid = [t for t, pid in enumerate(sp) if pid >= 0]
        if all_open:
            open_slots = valid
        out["path"] = "scratch_all" if all_open or open_slots == valid else "scratch_some"
        cand = {}
        for t in open_slots:                                                     # every candidate of an open slot under the mask
            for pix in np.nonzero(b.ok[sp[t], :, q])[0]:
                cand[t * HWk + int(pix)] = True
        for s, g in top[:m]:                                                     # the closed slots' contenders are among the 16, inside the window
            if g // HWk not in open_slots:
                cand[g] = True
        ent = [(s32_of(g), g, True) for g in cand]
    ent.sort(key=lambda e: (-e[0], e[1]))
    ent = ent[:k]
    out["gid"] = [g for _, g, _ in ent] + [-1] * (k - len(ent))
    out["score"] = [s for s, _, _ in ent] + [NINF] * (k - len(ent))
    out["exact"] = [x for _, _, x in ent] + [False] * (k - len(ent))
    return out


def scan_cap(n_out: int, HWq: int) -> int:
    return max(4096, (n_out * HWq + 31) // 32)


@functools.lru_cache(maxsize=None)
def restated(name: str) -> dict:
    """Every query of a case: idx (n_out, HWq, k) int64, score (the f32 score each final entry carries: s32 where re-scored or from
    scratch, a otherwise) and exact (which), path (index into PATHS), the statistics words the kernel reports, the largest
    |a - s32| over the re-scored entries (word 4), over the sampled queries' listed entries (word 5) and over all listed entries."""
    b = built(name)
    n_out, HWq, k = b.slot_pair.shape[0], b.pair_idx.shape[1], b.case.k
    idx = np.full((n_out, HWq, k), -1, np.int64)
    score = np.full((n_out, HWq, k), -np.inf, np.float32)
    exact = np.zeros((n_out, HWq, k), bool)
    path = np.zeros((n_out, HWq), np.int64)
    flagged = n_brute = n_cand = smp_q = smp_n = 0
    err_resc = err_smp = 0.0
    for f in range(n_out):
        for q in range(HWq):
            r = restate_query(b, f, q)
            idx[f, q], score[f, q], exact[f, q], path[f, q] = r["gid"], r["score"], r["exact"], PATHS.index(r["path"])
            flagged += r["path"] != "final"
            n_brute += r["brute"]
            n_cand += r["n_mask"]
            err_resc = max([err_resc] + [e for _, e in r["rescored"]])
            if r["path"] == "final" and r["sampled"]:
                smp_q, smp_n, err_smp = smp_q + 1, smp_n + r["n_listed16"], max(err_smp, r["sample_err"])
    listed = b.pair_idx >= 0
    gather = np.take_along_axis(b.s32.transpose(0, 2, 1), np.maximum(b.pair_idx, 0).astype(np.int64), 2)
    err_listed = float(np.abs(b.pair_score.astype(np.float64) - gather.astype(np.float64))[listed].max())
    counts = {p: int((path == i).sum()) for i, p in enumerate(PATHS)}
    return dict(idx=idx, score=score, exact=exact, path=path, counts=counts, err_rescored=err_resc, err_sampled=err_smp, err_listed=err_listed,
                words={0: flagged, 1: n_brute, 2: n_cand, 3: max(0, n_brute - scan_cap(n_out, HWq)), 6: smp_n, 7: smp_q},
                unflagged=int((path == 0).sum()))
