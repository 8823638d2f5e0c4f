"""Case tables, planted feature rows, float64 slabs and the list checker shared by tests/test_gpu_pair_ops.py (the four pair top-k
kernels: csrc/pair_topk.hip, pair_topk_v5.hip, pair_topk_v7.hpp, pair_topk_v8.hpp) and tests/test_pair_reference_share.py (the same
statements on the CPU, from the rows and the oracle alone).  No GPU code here.

The rows are PLANTED so that every dot product is exact in every arithmetic the kernels use -- the f32 chains, the f16 (h, l) split
with l = 0, the f16 + FP6 rows with h exact and both residual forms 0 -- so no comparison below needs a tolerance:
    codebook  each pixel draws one of a few dozen unit rows with 4^m non-zeros of +-2^-m (m = 1..4) or a zero row: scores are multiples
              of 2^-8, exact ties everywhere (also across the k-th place); a key frame equal to the query frame (self scores exactly
              1), one equal to minus it (self scores exactly -1) and an all-zero one (every score 0).
    graded    query rows +-e_c for two channels c; key rows carry +-a / 2048 on those channels, a a permutation of 1..HWk (HWk <= 1447,
              so that a^2 + b^2 < 2^22), and four more entries w / 2048 with w^2 + x^2 + y^2 + z^2 = 2^22 - a^2 - b^2: norm exactly 1,
              and within any window all finite scores are distinct -- the full index list is determined for every kernel.
    smallint  (fgvc_pair_topk_f32 only) un-normalised integer rows, |entries| <= 3: dots exact far beyond 1.
    gauss     real-valued unit rows for the tolerance variant of the checker (the bars the kernels' existing tests use).

check_lists states the contract the kernels document (score descending, index ascending), see its docstring.
"""
import functools
import math
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from oracle import fgvc_oracle as O

NO_LIMIT = 0x3FFFFFFF
TAU = 0.07
NEG_INF = float("-inf")
V8 = 4194304                      # pair_f16_debug bit: pair_topk_kernel_v8 takes the launch
QBH, QBW = 4, 8


@dataclass(frozen=True)
class Case:
    name: str
    family: str                   # codebook | graded | smallint | gauss
    C: int
    qgrid: Tuple[int, int]
    kgrid: Tuple[int, int]
    T: int                        # frames of the bank (equal grids) / key frames (unequal grids: two query frames)
    mask: Tuple[int, int, int]    # (r2max, ry, rx), NO_LIMIT = off
    k32: int                      # top-k asked of fgvc_pair_topk_f32
    ksplit: int                   # top-k asked of the split kernels
    dense: str = ""               # "" | bern | reject | lastrc: a dense user mask of that kind (f32 only)
    seed: int = 0
    mix: bool = True              # some rows without PAIR_MASKED (f32 and f16x3; the f16 + FP6 kernels get every row masked)

    @property
    def equal(self):
        return self.qgrid == self.kgrid

    @property
    def has_mask(self):
        return min(self.mask) < NO_LIMIT

    @property
    def split_ok(self):
        """what fgvc_pair_topk_f16x3 documents: 256 channels, normalised rows, k <= 10, analytic mask or none"""
        return self.C == 256 and self.family != "smallint" and not self.dense and 1 <= self.ksplit <= 10


def case_id(c):
    return c.name


# ----------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------
GRIDS = [(1, 1), (1, 9), (9, 1), (4, 8), (5, 9), (7, 15), (8, 16), (9, 17), (12, 24), (17, 23), (33, 41)]
MASKS = [("r0", (0, NO_LIMIT, NO_LIMIT)), ("r1", (1, NO_LIMIT, NO_LIMIT)), ("r2", (2, NO_LIMIT, NO_LIMIT)),
         ("r4", (4, NO_LIMIT, NO_LIMIT)), ("r5", (5, NO_LIMIT, NO_LIMIT)),
         ("liney", (NO_LIMIT, 0, 6)), ("linex", (NO_LIMIT, 6, 0)),
         ("rect3x7", (NO_LIMIT, 3, 7)), ("rect4x8", (NO_LIMIT, 4, 8)), ("rect5x9", (NO_LIMIT, 5, 9)), ("rect9x3", (NO_LIMIT, 9, 3)),
         ("disc20cut3x4", (20, 3, 4)), ("disc5000", (5000, NO_LIMIT, NO_LIMIT)), ("nomask", (NO_LIMIT, NO_LIMIT, NO_LIMIT))]
K32 = [1, 2, 5, 6, 10, 11, 16]
KSPLIT = [1, 3, 5, 6, 10]


def _planted_equal():
    out, n = [], 0
    for gi, grid in enumerate(GRIDS):
        for mi, (mname, mask) in enumerate(MASKS):
            if (gi + mi) % 2:                           # half of the grid x mask table: every grid meets 7 masks, every mask 5 or 6 grids
                continue
            for fam in ("codebook", "graded"):
                out.append(Case(f"{fam}-{grid[0]}x{grid[1]}-{mname}-k{K32[n % 7]}-{KSPLIT[n % 5]}", fam, 256, grid, grid, 2 + n % 3, mask,
                                K32[n % 7], KSPLIT[n % 5], seed=n))
                n += 1
    return out


PLANTED_EQUAL = _planted_equal()

# unequal grids, no mask: fgvc_pair_topk_f32 and fgvc_pair_topk_f16x3
NOMASK = (NO_LIMIT, NO_LIMIT, NO_LIMIT)
UNEQUAL = [Case(f"{fam}-q{q[0]}x{q[1]}-k{kg[0]}x{kg[1]}-k{k32}-{ks}", fam, 256, q, kg, 3, NOMASK, k32, ks, seed=100 + i, mix=False)
           for i, (fam, q, kg, k32, ks) in enumerate([("codebook", (8, 16), (9, 17), 16, 10), ("graded", (8, 16), (12, 40), 11, 5),
                                                      ("codebook", (5, 9), (12, 40), 6, 6), ("graded", (5, 9), (9, 17), 2, 3)])]

# dense user masks: fgvc_pair_topk_f32 only
DENSE = [Case(f"dense-{kind}-{fam}-C{C}-q{q[0]}x{q[1]}-k{kg[0]}x{kg[1]}-k{k32}", fam, C, q, kg, 3, NOMASK, k32, 0, dense=kind, seed=200 + i)
         for i, (kind, fam, C, q, kg, k32) in enumerate([
             ("bern", "codebook", 256, (9, 17), (9, 17), 10), ("bern", "graded", 32, (5, 9), (9, 17), 5),
             ("bern", "codebook", 32, (5, 9), (9, 17), 16), ("reject", "codebook", 256, (5, 9), (9, 17), 6),
             ("reject", "graded", 32, (9, 17), (9, 17), 11), ("reject", "graded", 256, (5, 9), (9, 17), 2),
             ("lastrc", "codebook", 32, (9, 17), (9, 17), 10), ("lastrc", "graded", 256, (5, 9), (9, 17), 16),
             ("bern", "graded", 256, (17, 23), (17, 23), 1)])]

# fgvc_pair_topk_f32 only: narrower rows, and un-normalised small integers
F32_ONLY = ([Case(f"codebook-C{C}-{g[0]}x{g[1]}-{mn}-k{k}", "codebook", C, g, g, 3, dict(MASKS)[mn], k, 0, seed=300 + i)
             for i, (C, g, mn, k) in enumerate([(32, (9, 17), "r2", 5), (64, (7, 15), "rect3x7", 11), (128, (12, 24), "disc20cut3x4", 16),
                                                (64, (5, 9), "nomask", 2), (128, (9, 17), "r0", 6), (32, (17, 23), "rect5x9", 10)])] +
            [Case(f"graded-C{C}-{g[0]}x{g[1]}-{mn}-k{k}", "graded", C, g, g, 3, dict(MASKS)[mn], k, 0, seed=320 + i)
             for i, (C, g, mn, k) in enumerate([(32, (9, 17), "r5", 6), (64, (12, 24), "rect4x8", 16), (128, (7, 15), "nomask", 11)])] +
            [Case(f"smallint-C{C}-{g[0]}x{g[1]}-{mn}-k{k}", "smallint", C, g, g, 3, dict(MASKS)[mn], k, 0, seed=340 + i)
             for i, (C, g, mn, k) in enumerate([(256, (9, 17), "r4", 10), (64, (17, 23), "rect3x7", 16), (32, (5, 9), "nomask", 5),
                                                (128, (8, 16), "linex", 1), (256, (12, 24), "disc5000", 11)])])

# real-valued rows at the short-window shapes: the tolerance variant
GAUSS = [Case(f"gauss-{g[0]}x{g[1]}-{mn}-k{k32}-{ks}", "gauss", 256, g, g, 3, dict(MASKS)[mn], k32, ks, seed=400 + i)
         for i, (g, mn, k32, ks) in enumerate([((5, 9), "r1", 10, 10), ((9, 17), "r4", 16, 6), ((7, 15), "liney", 11, 5),
                                               ((17, 23), "rect4x8", 6, 10), ((4, 8), "nomask", 16, 10), ((1, 9), "r0", 5, 3)])]

# list-size boundaries of fgvc_pair_topk_f16x3: one unmasked pair, a one-tile query grid, codebook rows.  (key grid, key blocks, what)
BIG = [((128, 512), 2048, "three_role_limit"), ((128, 520), 2080, "two_role"), ((256, 512), 4096, "still_accepted")]
BIG_REFUSED = (256, 520)                                # 64 x 65 = 4160 blocks: one block column more
BIG_Q = (8, 16)
BIG_K = 10

ALL_PLANTED = PLANTED_EQUAL + UNEQUAL + DENSE + F32_ONLY


# ----------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def codebook(C):
    """(n, C) f32: ten rows each with 4^m non-zeros of +-2^-m (norm exactly 1) for every m with 4^m <= C, drawn from the first 4^(m+1)
    channels so that supports overlap, plus two zero rows"""
    rng = np.random.default_rng(1000 + C)
    rows = []
    m = 1
    while 4 ** m <= C and m <= 4:
        nz, pool = 4 ** m, min(C, 4 ** (m + 1))
        for _ in range(10):
            v = np.zeros(C, np.float32)
            v[rng.choice(pool, nz, replace=False)] = rng.choice([-1.0, 1.0], nz) * 2.0 ** -m
            rows.append(v)
        m += 1
    rows += [np.zeros(C, np.float32)] * 2
    return np.stack(rows)


@functools.lru_cache(maxsize=1)
def _two_squares():
    n = 40000
    tab = np.full((n, 2), -1, np.int64)
    for y in range(200):
        for z in range(y + 1):
            if y * y + z * z < n and tab[y * y + z * z, 0] < 0:
                tab[y * y + z * z] = (y, z)
    return tab


def four_squares(n):
    """n >= 0 -> (w, x, y, z), w^2 + x^2 + y^2 + z^2 = n (Lagrange), w the largest"""
    if n and n % 4 == 0:                                 # n = 0 mod 4: halve (every solution of n = 0 mod 8 is all even anyway)
        return tuple(2 * v for v in four_squares(n // 4))
    tab = _two_squares()                                 # n = 1, 2, 3 mod 4: n - w^2 = 1 or 2 mod 4, a sum of three squares, for w or w - 1
    w = math.isqrt(n)
    while w >= 0:
        rem = n - w * w
        if rem < len(tab):
            x = math.isqrt(rem)
            while x >= 0:
                y, z = tab[rem - x * x]
                if y >= 0:
                    return w, x, int(y), int(z)
                x -= 1
        w -= 1
    raise AssertionError(n)


def graded_channels(C):
    """(the two channels a query row may select, the four channels that complete a key row to norm 1)"""
    return (3, C - 7), (1, C // 2, C // 2 + 5, C - 1)


def graded_key_frame(HW, C, rng):
    assert HW <= 1447, "a^2 + b^2 must stay below 2^22"
    (c0, c1), fill = graded_channels(C)
    a, b = rng.permutation(HW) + 1, rng.permutation(HW) + 1
    rows = np.zeros((HW, C), np.float64)
    rows[:, c0] = a * rng.choice([-1, 1], HW)
    rows[:, c1] = b * rng.choice([-1, 1], HW)
    for j in range(HW):
        sq = four_squares((1 << 22) - int(a[j]) ** 2 - int(b[j]) ** 2)
        rows[j, list(fill)] = np.array(sq) * rng.choice([-1, 1], 4)
    return (rows / 2048.0).astype(np.float32)


def graded_query_frame(HW, C, rng):
    (c0, c1), _ = graded_channels(C)
    rows = np.zeros((HW, C), np.float32)
    rows[np.arange(HW), np.where(rng.integers(0, 2, HW) == 0, c0, c1)] = rng.choice([-1.0, 1.0], HW)
    return rows


def _rows_equal(T, variant, mix):
    """pair rows over one bank of T frames: q == k first, runs of 1 to 3 pairs, a row without PAIR_MASKED here and there"""
    rows = []
    for q in range(T):
        for j in range(1 + (q + variant) % 3):
            rows.append((q, (q + j) % T, not (mix and (q + j + variant) % 3 == 2)))
    return rows


@dataclass
class Built:
    case: Case
    qfeat: torch.Tensor           # (nq, HWq, C) f32
    kfeat: torch.Tensor           # (nk, HWk, C) f32; the same tensor as qfeat on equal grids
    rows: list                    # (q, k, masked)
    dense_mask: Optional[torch.Tensor]      # (HWk, HWq) bool
    scale: float                  # slab * scale is integral (0: not planted)
    kinds: list                   # what each key frame is

    def rows_for(self, all_masked):
        return [(q, k, True) for q, k, _ in self.rows] if all_masked else self.rows


@functools.lru_cache(maxsize=None)
def built(name):
    case = {c.name: c for c in ALL_PLANTED + GAUSS}[name]
    rng = np.random.default_rng(77 + case.seed)
    HWq, HWk, C, T = case.qgrid[0] * case.qgrid[1], case.kgrid[0] * case.kgrid[1], case.C, case.T
    mix = case.mix and case.has_mask or bool(case.dense)
    if case.family == "graded":
        nq = 1 if T == 2 else 2
        if case.equal:
            frames = [graded_query_frame(HWq, C, rng) for _ in range(nq)] + [graded_key_frame(HWk, C, rng) for _ in range(T - nq)]
            kinds = ["query"] * nq + ["key"] * (T - nq)
            qf = kf = np.stack(frames)
            rows = [(q, k, not (mix and (q + k) % 3 == 2)) for q in range(nq) for k in range(nq, T)]
        else:
            qf = np.stack([graded_query_frame(HWq, C, rng) for _ in range(2)])
            kf = np.stack([graded_key_frame(HWk, C, rng) for _ in range(T)])
            kinds = ["key"] * T
            rows = [(0, 0, True), (0, 1, True), (1, 1, not mix), (1, 2, True)]
        scale = 2.0 ** 22
    else:
        if case.family == "codebook":
            book = codebook(C)
            draw = lambda hw: book[rng.integers(0, len(book), hw)]
            scale = 2.0 ** 8
        elif case.family == "smallint":
            draw = lambda hw: (rng.integers(-3, 4, (hw, C)) * (rng.random((hw, C)) < 0.5)).astype(np.float32)
            scale = 1.0
        else:
            draw = lambda hw: torch.nn.functional.normalize(torch.from_numpy(rng.standard_normal((hw, C)).astype(np.float32)), dim=1).numpy()
            scale = 0.0
        if case.equal:
            frames, kinds = [draw(HWq)], ["draw"]
            special = {2: ["neg0"], 3: ["draw", "zero"], 4: ["draw", "neg0", "zero"]}[T]
            if case.family == "gauss":
                special = ["draw"] * (T - 1)
            for s in special:
                frames.append({"draw": lambda: draw(HWq), "neg0": lambda: -frames[0], "zero": lambda: np.zeros((HWq, C), np.float32)}[s]())
                kinds.append(s)
            qf = kf = np.stack(frames)
            rows = _rows_equal(T, case.seed, mix)
        else:
            qf = np.stack([draw(HWq) for _ in range(2)])
            kf = np.stack([draw(HWk) for _ in range(T - 1)] + [np.zeros((HWk, C), np.float32)])
            kinds = ["draw"] * (T - 1) + ["zero"]
            rows = [(0, 0, True), (0, 1, True), (1, 1, not mix), (1, 2, True), (1, 0, True)][:T + 2]
    if not case.has_mask and not case.dense:
        rows = [(q, k, False) for q, k, _ in rows]
    qt = torch.from_numpy(np.ascontiguousarray(qf, np.float32))
    kt = qt if kf is qf else torch.from_numpy(np.ascontiguousarray(kf, np.float32))
    b = Built(case, qt, kt, rows, None, scale, kinds)
    if case.dense:
        b.dense_mask = _dense_mask(b, rng)
    return b


def _dense_mask(b, rng):
    """(HWk, HWq) bool.  bern: Bernoulli(0.3), the first three columns all false, column 3 admitting exactly k - 1 keys and column 4
    exactly k; reject: everything but each query's own unmasked top k (of the first masked pair): the kernel's lazy byte gather, taken
    only for candidates that could still enter the list, runs for exactly the candidates that must go; lastrc: true only on the last row
    and the last column of the (ragged) key grid."""
    c = b.case
    HWq, HWk, k = c.qgrid[0] * c.qgrid[1], c.kgrid[0] * c.kgrid[1], c.k32
    if c.dense == "bern":
        m = torch.from_numpy(rng.random((HWk, HWq)) < 0.3)
        m[:, :3] = False
        for col, n in ((3, k - 1), (4, k)):
            m[:, col] = False
            m[torch.from_numpy(rng.choice(HWk, n, replace=False)), col] = True
        return m
    if c.dense == "reject":
        q, kk, _ = next(r for r in b.rows if r[2])
        raw = b.kfeat[kk].double() @ b.qfeat[q].double().t()
        _, di = O.topk_canonical(raw, k)
        m = torch.ones(HWk, HWq, dtype=torch.bool)
        m.scatter_(0, di, False)
        return m
    assert c.dense == "lastrc"
    ky, kx = torch.arange(HWk) // c.kgrid[1], torch.arange(HWk) % c.kgrid[1]
    return ((ky == c.kgrid[0] - 1) | (kx == c.kgrid[1] - 1)).view(-1, 1).expand(HWk, HWq).clone()


# ----------------------------------------------------------------------------------------------------------------------
# the float64 slab
# ----------------------------------------------------------------------------------------------------------------------
def analytic_admit(grid, mask):
    """(HW, HW) bool [key, query]: dy^2 + dx^2 <= r2max, |dy| <= ry, |dx| <= rx with (dy, dx) = key - query, in integers"""
    H, W = grid
    y, x = torch.arange(H * W) // W, torch.arange(H * W) % W
    dy, dx = y.view(-1, 1) - y.view(1, -1), x.view(-1, 1) - x.view(1, -1)
    return (dy * dy + dx * dx <= mask[0]) & (dy.abs() <= mask[1]) & (dx.abs() <= mask[2])


def admitted(b, masked):
    """(HWk, HWq) bool or None (everything admitted) for a pair with / without PAIR_MASKED"""
    if not masked:
        return None
    if b.dense_mask is not None:
        return b.dense_mask
    if b.case.has_mask:
        assert b.case.equal
        return analytic_admit(b.case.kgrid, b.case.mask)
    return None


def raw64(b, q, k):
    return b.kfeat[k].double() @ b.qfeat[q].double().t()


def slab64(b, row):
    """float64 (HWk, HWq) of pair row (q, k, masked): the exact dot products, -inf where the pair's mask rejects"""
    q, k, masked = row
    s = raw64(b, q, k)
    adm = admitted(b, masked)
    return s if adm is None else s.masked_fill(~adm, NEG_INF)


def window_size(mask):
    """offsets the analytic predicate admits on an unbounded grid (capped at 129 x 129)"""
    d = torch.arange(-64, 65)
    dy, dx = d.view(-1, 1), d.view(1, -1)
    return int(((dy * dy + dx * dx <= mask[0]) & (dy.abs() <= mask[1]) & (dx.abs() <= mask[2])).sum())


# ----------------------------------------------------------------------------------------------------------------------
# the checker
# ----------------------------------------------------------------------------------------------------------------------
def canonical_lists(slab, k):
    """(idx (S, k) int64, score (S, k) float64) of O.topk_canonical, padded with (-1, -inf) where the window holds fewer than k"""
    M, S = slab.shape
    kk = min(k, M)
    cv, ci = O.topk_canonical(slab, kk)
    idx = torch.full((S, k), -1, dtype=torch.int64)
    val = torch.full((S, k), NEG_INF, dtype=torch.float64)
    val[:, :kk] = cv.t()
    idx[:, :kk] = torch.where(torch.isfinite(cv.t()), ci.t(), torch.full_like(ci.t(), -1))
    return idx, val


def check_lists(slab, idx, score, k, canonical=False, tol=0.0):
    """Hold (idx, score) (S, k) to the float64 slab (M, S) of one (pair, query grid), -inf = not admitted.  Raises AssertionError naming
    the rule; returns counts.
      scores      the k scores equal the canonical top-k score list (as numbers: -0 == +0); every idx >= 0 is in bounds, admitted, and
                  its slab value equals its score
      distinct    the indices of a list are pairwise distinct
      order       score descending, index ascending among equal scores
      empties     exactly max(0, k - |window|) entries are (-1, -inf), all at the tail
      membership  every candidate strictly above the k-th score is listed; among candidates tied at the k-th score any choice passes
      canonical   (canonical=True) the indices equal O.topk_canonical's
    tol > 0 (real-valued rows): distinct, admission, empties and order (in the kernel's own scores) stay exact; a score may differ from
    its slab value and from the canonical list's by tol; every listed candidate lies within 2 tol of the k-th canonical score and every
    candidate more than 2 tol above it is listed (a candidate's kernel score is within tol of its slab value, so fewer than k candidates
    can have a kernel score above kth + tol, and the kernel's k-th score is at least kth - tol)."""
    M, S = slab.shape
    idx, score = idx.long(), score.double()
    assert idx.shape == score.shape == (S, k), (idx.shape, score.shape, (S, k))
    ci, cv = canonical_lists(slab, k)
    nwin = torch.isfinite(slab).sum(0)
    n_empty = (k - nwin).clamp_min(0)
    emp = idx < 0
    want_emp = torch.arange(k).view(1, k) >= (k - n_empty).view(S, 1)
    assert torch.equal(emp, want_emp), f"empties: {int((emp != want_emp).any(1).sum())} queries do not hold exactly max(0, k - |window|) empties at the tail"
    assert bool((idx[emp] == -1).all()) and bool((score[emp] == NEG_INF).all()), "empties: an empty entry is not (-1, -inf)"
    assert bool((idx[~emp] < M).all()), "scores: index out of bounds"
    got = slab.t().gather(1, idx.clamp_min(0))
    assert bool(torch.isfinite(got[~emp]).all()), f"scores: {int((~torch.isfinite(got) & ~emp).sum())} listed indices are not admitted by the mask"
    srt = torch.sort(torch.where(emp, -1 - torch.arange(k).view(1, k).expand(S, k), idx), dim=1).values
    assert bool((srt[:, 1:] != srt[:, :-1]).all()), f"distinct: {int((srt[:, 1:] == srt[:, :-1]).any(1).sum())} lists name an index twice"
    live2 = ~emp[:, 1:]
    assert bool((score[:, :-1] >= score[:, 1:])[live2].all()), "order: scores ascend somewhere"
    tie = (score[:, :-1] == score[:, 1:]) & live2
    assert bool((idx[:, :-1] < idx[:, 1:])[tie].all()), f"order: {int(((idx[:, :-1] > idx[:, 1:]) & tie).any(1).sum())} lists hold equal scores out of index order"
    err = torch.where(emp, torch.zeros_like(got), (got - score).abs())
    lerr = torch.where(emp, torch.zeros_like(got), (cv - score).abs())
    assert float(err.max()) <= tol, f"scores: a score is {float(err.max())} from its slab value"
    assert float(lerr.max()) <= tol, f"scores: the score list is {float(lerr.max())} from the canonical top-k scores"
    kth = cv[:, k - 1]                                                    # -inf where the window is short: then everything admitted is above it
    listed = torch.zeros(M + 1, S, dtype=torch.bool)
    listed.scatter_(0, torch.where(emp, torch.full_like(idx, M), idx).t().contiguous(), True)
    missing = (slab > (kth + 2 * tol).view(1, S)) & ~listed[:M]
    assert not bool(missing.any()), f"membership: {int(missing.any(0).sum())} lists lack a candidate strictly above the k-th score"
    low = torch.where(emp, torch.zeros_like(got, dtype=torch.bool), got < (kth - 2 * tol).view(S, 1))
    assert not bool(low.any()), "membership: a listed candidate is below the k-th score"
    exact = (idx == ci).all(1)
    if canonical:
        assert bool(exact.all()), f"canonical: {int((~exact).sum())} lists differ from O.topk_canonical"
    return dict(queries=S, canonical=int(exact.sum()), short=int((n_empty > 0).sum()), max_err=float(err.max()))


def edge_counts(slab, k):
    """what one (pair, k) slab exercises: queries with a short window, tied across the k-th place, whose list holds a score of exactly
    -1 / 0 / +1, fully rejected; and whether any two finite scores of one window tie"""
    M, S = slab.shape
    ci, cv = canonical_lists(slab, k)
    nwin = torch.isfinite(slab).sum(0)
    kth = cv[:, k - 1]
    tied = torch.isfinite(kth) & ((slab == kth.view(1, S)).sum(0) > 1) & ((slab >= kth.view(1, S)).sum(0) > k)
    srt = torch.sort(slab, dim=0, descending=True).values
    any_tie = bool(((srt[1:] == srt[:-1]) & torch.isfinite(srt[1:])).any()) if M > 1 else False
    return dict(short=int(((nwin < k) & (nwin > 0)).sum()), tied_kth=int(tied.sum()), minus1=int((cv == -1).any(1).sum()),
                zero=int((cv == 0).any(1).sum()), plus1=int((cv == 1).any(1).sum()), rejected=int((nwin == 0).sum()), any_tie=any_tie)


# ----------------------------------------------------------------------------------------------------------------------
# key blocks an interior query tile reaches, by brute force over pixels (ops.pair_blocks_reached / pair_v7_blocks_reached restate it
# as block-to-block distances)
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blocks_reached_brute(r2max, ry, rx):
    """distinct 4 x 8 key blocks holding at least one pixel that some pixel of an 8 x 16 block-aligned query tile admits"""
    rr = math.isqrt(r2max) if r2max < NO_LIMIT else NO_LIMIT
    Ry, Rx = min(ry, rr), min(rx, rr)
    assert Ry <= 64 and Rx <= 64
    dy, dx = np.arange(-Ry, Ry + 1).reshape(-1, 1), np.arange(-Rx, Rx + 1).reshape(1, -1)
    D = (dy * dy + dx * dx <= r2max) & (np.abs(dy) <= ry) & (np.abs(dx) <= rx)
    oy, ox = (Ry // QBH + 1) * QBH, (Rx // QBW + 1) * QBW               # the tile's origin: block aligned, further than the reach from the corner
    hit = np.zeros((oy + 2 * QBH + Ry + QBH, ox + 2 * QBW + Rx + QBW), bool)
    for qy in range(2 * QBH):
        for qx in range(2 * QBW):
            hit[oy + qy - Ry: oy + qy + Ry + 1, ox + qx - Rx: ox + qx + Rx + 1] |= D
    H, W = hit.shape[0] // QBH * QBH, hit.shape[1] // QBW * QBW
    assert not hit[H:].any() and not hit[:, W:].any()
    return int(hit[:H, :W].reshape(H // QBH, QBH, W // QBW, QBW).any((1, 3)).sum())


def sweep_masks():
    """the masks the CPU sweep covers: discs r2max 0..700, rectangles ry, rx in 0..20, discs cut by rectangles"""
    out = [(r2, NO_LIMIT, NO_LIMIT) for r2 in range(701)]
    out += [(NO_LIMIT, ry, rx) for ry in range(21) for rx in range(21)]
    out += [(r2, ry, rx) for r2 in (5, 20, 50, 101, 224, 400, 577) for ry in (0, 2, 3, 7, 11, 15, 20) for rx in (0, 3, 4, 8, 12, 17, 20)]
    return out


@functools.lru_cache(maxsize=1)
def limit_masks():
    """(masks at the limit, the smallest masks above it) from the brute-force count over the sweep.  At: the rectangles of exactly 64
    blocks whose every neighbour one pixel smaller or larger in one reach has another count or is also 64 -- the corners of the region
    -- the cut discs of exactly 64, and the largest disc still inside (no disc has exactly 64: the count steps from 60 to 68).  Above:
    the masks over 64 that fall to 64 or below when any one parameter shrinks by one."""
    n_of = lambda m: blocks_reached_brute(*m)
    at = [m for m in sweep_masks() if n_of(m) == 64 and m[0] < NO_LIMIT]
    rect64 = [(ry, rx) for ry in range(21) for rx in range(21) if n_of((NO_LIMIT, ry, rx)) == 64]
    ys, xs = sorted({r[0] for r in rect64}), sorted({r[1] for r in rect64})
    at += [(NO_LIMIT, ry, rx) for ry in (ys[0], ys[-1]) for rx in (xs[0], xs[-1]) if (ry, rx) in rect64]
    first_over = min(r2 for r2 in range(701) if n_of((r2, NO_LIMIT, NO_LIMIT)) > 64)
    at.append((first_over - 1, NO_LIMIT, NO_LIMIT))
    above = [(first_over, NO_LIMIT, NO_LIMIT)]
    above += [(NO_LIMIT, ry, rx) for ry in range(1, 21) for rx in range(1, 21) if n_of((NO_LIMIT, ry, rx)) > 64
              and n_of((NO_LIMIT, ry - 1, rx)) <= 64 and n_of((NO_LIMIT, ry, rx - 1)) <= 64]
    return at, above


# ----------------------------------------------------------------------------------------------------------------------
# the big key grids
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)                        # a key frame is up to 128 MiB, its slab as much again: keep one
def big_rows(kgrid):
    """codebook rows for one unmasked pair: query (1, 128, 256) on the 8 x 16 tile, key (1, HWk, 256), and the float64 slab through
    the codebook's Gram matrix (every entry is one of its 42 x 42 exact values)"""
    rng = np.random.default_rng(9000 + kgrid[0] + kgrid[1])
    book = codebook(256)
    qc, kc = rng.integers(0, len(book), BIG_Q[0] * BIG_Q[1]), rng.integers(0, len(book), kgrid[0] * kgrid[1])
    gram = torch.from_numpy(book).double() @ torch.from_numpy(book).double().t()
    slab = gram[torch.from_numpy(kc)][:, torch.from_numpy(qc)].contiguous()
    return torch.from_numpy(book[qc]).unsqueeze(0), torch.from_numpy(book[kc]).unsqueeze(0), slab
