"""Shared by test_fuse_host.py and test_gpu_fuse.py: the float64 restatement of ops.seg_fuse_rows with its error budget, the annotation sets
and rolled complete maps of the late-object clip (tests/refs_cases.py), and the two passes of engine.fuse_refs_host kept apart so that a
test can tell which cells either pass leaves undecided.  Everything here runs on the CPU."""
import functools

import numpy as np
import torch

from tests import refs_cases as R

U = R.U
DECIDE = R.DECIDE

# ---- the kernel alone ---------------------------------------------------------------------------------------------------------------------
# (Hf, Wf) per HW of the kernel cases: 1, 63, 64, 65 straddle one wave's worth of cells (a workgroup takes 256 / G cells per iteration, G =
# the lanes per row), 1085 = 31 x 35 takes more than one workgroup for every C >= 2 and more than one iteration of none
FUSE_GRIDS = {1: (1, 1), 63: (7, 9), 64: (8, 8), 65: (5, 13), 1085: (31, 35)}
FUSE_CHANNELS = (1, 2, 3, 256)
# stacks larger than the item list, items at non-adjacent frames in no particular order: (n_fw, n_bw, n_out), then per item count the
# (fw frame, bw frame, out frame) triples
FUSE_STACKS = (7, 6, 5)
FUSE_ITEMS = {1: [(5, 4, 3)], 3: [(5, 0, 3), (1, 4, 0), (3, 2, 2)]}

# The error budget of one fused element against float64, next to refs_cases.conf_delta.  The kernel computes
#     fl( w32 * x + fl( fl(1 - w32) * y ) )          (one fused multiply-add around one product)
# from the f32 inputs x, y with |x|, |y| <= 1 and the weight 0 <= w <= 1 given as a host double and rounded to f32.  Roundings, each at most
# U relative to its own result, and what each contributes to the element in absolute terms:
#   w32 = w (1 + d0)                     |w32 x - w x| <= U |x|                               <= U
#   1 - w32 against 1 - w                the same d0: U w |y|                                 <= U
#   v = fl(1 - w32)                      U (1 - w32) |y|                                      <= U
#   p = fl(v y)                          U |v y|                                              <= U
#   the fused multiply-add's rounding    U |result|, the result a convex combination          <= U
# FUSE_ROUNDINGS = 5 such terms; the products of two of them are bounded by 4 U^2 each, 10 pairs.
FUSE_ROUNDINGS = 5


def fuse_delta() -> float:
    """The largest |kernel - float64| of one fused element for inputs of magnitude at most 1 (see above)."""
    return FUSE_ROUNDINGS * U + 40 * U * U


def fuse_rows_f64(fw, bw, items, weights):
    """ops.seg_fuse_rows in float64: fw (n_fw, HW, C), bw (n_bw, HW, C) (any float dtype; their values are taken as they are), items
    [(fw frame, bw frame, out frame)], weights host doubles -> ([rows (HW, C) float64 per item], counts (n,) int64)."""
    rows, counts = [], []
    for (fi, bi, _), w in zip(items, weights):
        x, y = fw[fi].double(), bw[bi].double()
        rows.append(w * x + (1.0 - w) * y)
        counts.append(int((x.argmax(-1) != y.argmax(-1)).sum()))               # torch.argmax: the first maximum
    return rows, torch.tensor(counts, dtype=torch.int64)


def dyadic_stack(n, HW, C, seed):
    """(n, HW, C) float32 with every value a multiple of 2^-8 in [0, 1]: with w in {0.25, 0.5, 0.75} every product and the sum are exact in
    f32.  Planted per block: cell 0 an all-zero row, cell 1 (where there is one) a row whose maximum stands at every channel (ties: the
    first wins), cell 2 a row whose maximum stands at its last two channels."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 257, (n, HW, C), generator=g).float() / 256.0
    x[:, 0] = 0.0
    if HW > 1:
        x[:, 1] = 0.5
    if HW > 2 and C > 1:
        x[:, 2] = 0.25
        x[:, 2, -2:] = 0.75
    return x


# ---- the late-object clip with complete maps ------------------------------------------------------------------------------------------------
FUSE_SETS = [(0, 3, 6), (1, 4), (0, 4)]


def rolled_maps(frames):
    """{t: refs_cases.late_maps()[0] rolled by (2t, 2t) pixels}: complete maps (every object in every map), moving with the clip."""
    base = R.late_maps()[0]
    return {t: np.roll(base, (2 * t, 2 * t), axis=(0, 1)) for t in frames}


def late_geometry():
    """(T, h, w, (hp, wp), pad, Hf, Wf) of the late-object clip."""
    from fgvc_amd import engine
    T, h, w, d = R.LATE_T, R.LATE_H, R.LATE_W, R.LATE_D
    (hp, wp), pad = engine.pad_divide_by(h, w, d)
    return T, h, w, (hp, wp), pad, hp // d, wp // d


def small_maps(frames, pad, Hf, Wf):
    """-> ({t: padded map (hp, wp) uint8 ndarray}, {t: (HW,) int64 ids on the feature grid})"""
    padded = {t: np.pad(m, ((pad[2], pad[3]), (pad[0], pad[1]))) for t, m in rolled_maps(frames).items()}
    return padded, {t: torch.from_numpy(R.pil_nearest(m, Hf, Wf).astype(np.int64)).reshape(-1) for t, m in padded.items()}


@functools.lru_cache(maxsize=None)
def oracle_sweep(start, direction):
    """The oracle's float64 lists of the late-object clip's forward sub-clip start .. T-1 ('fw') or reversed sub-clip start .. 0 ('bw')."""
    from fgvc_amd import engine
    T, _, _, _, _, Hf, Wf = late_geometry()
    feats = R.clip_chw(T, 64, Hf, Wf, R.LATE_SEED)
    sub = feats[start:] if direction == "fw" else feats[:start + 1].flip(0)
    return R.oracle_lists(sub.contiguous(), engine.TrackerConfig(**R.LATE_KW))


def passes_f64(small, T, fw, bw, hard):
    """The two passes engine.fuse_refs_host blends, kept apart: F (T, HW, C) and B (s_m + 1, HW, C) in clip frame order, float64."""
    from fgvc_amd import engine
    frames = sorted(small)
    sm = frames[-1]
    F = engine.sweep_refs_host(small, T, fw=fw, direction="forward", override="all", hard_prop=hard)
    B = engine.sweep_refs_host({sm - t: small[t] for t in frames}, sm + 1, fw=bw, direction="forward", override="all", hard_prop=hard).flip(0)
    return F, B


def row_gap(rows):
    """rows (..., C) -> the top-two gap of every row (inf where C == 1)."""
    if rows.shape[-1] == 1:
        return torch.full(rows.shape[:-1], float("inf"), dtype=torch.float64)
    top = rows.double().topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def between(frames):
    """The frames strictly between two annotated ones."""
    return [t for a, b in zip(frames[:-1], frames[1:]) for t in range(a + 1, b)]


def disagree_bounds(F, B, frames, T):
    """Per frame (lo, hi) (T,) int64: the float64 disagreement count over the cells both passes decide (top-two gap above DECIDE), and that
    count plus the number of cells either pass leaves undecided; zeros outside the between-annotation frames."""
    lo, hi = torch.zeros(T, dtype=torch.int64), torch.zeros(T, dtype=torch.int64)
    for t in between(frames):
        decided = (row_gap(F[t]) > DECIDE) & (row_gap(B[t]) > DECIDE)
        lo[t] = int(((F[t].argmax(-1) != B[t].argmax(-1)) & decided).sum())
        hi[t] = lo[t] + int((~decided).sum())
    return lo, hi
