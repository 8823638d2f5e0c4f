"""Shared cases of the pose renderer (fgvc_render_pose_u8) and what it is held to: viz.render(skeleton=..., heat=...,
backend='host').

A case is the keyword arguments of viz.render (numpy arrays) plus, optionally, dots=False (then it goes through viz.paint_pose, which has no
overlay).  The shapes are the smallest at which the kernel can go wrong: a workgroup owns TILE = (8 rows, 256 columns), so 3 x 20 x 300
frames have two column tiles and three row bands, and limbs cross x = 255 / 256 and y = 7 / 8, 15 / 16, lie in one tile, span all of them
and end off the frame on every side; the limb list is filled 256 candidates at a time, so one case keeps 300 limbs in ONE tile; every way
a limb is refused (NaN, the infinities, 1e30, +/-2^20, an invisible end) sits next to limbs that are drawn; and the heat maps hold every
kind of value the rule names."""
import functools

import numpy as np

from fgvc_amd import viz
from tests import render_cases as RC

TILE = RC.TILE


def _still(points, T, rng, step=0.75):
    """(P, T, 2): every point jittered by up to `step` px a frame round where it stands (frame 0 is the point itself)."""
    p = np.asarray(points, np.float64)
    j = rng.uniform(-step, step, (p.shape[0], T, 2))
    j[:, 0] = 0.0
    return p[:, None, :] + j


def _tiles(limb_width):
    T, H, W = 3, 20, 300
    rng = np.random.default_rng(31)
    joints = [
        (250.0, 3.0), (261.5, 5.0),         # 0-1 over x = 255 / 256
        (100.0, 5.0), (101.0, 10.5),        # 2-3 over y = 7 / 8
        (140.5, 13.0), (139.0, 18.0),       # 4-5 over y = 15 / 16
        (20.0, 1.5), (40.0, 5.5),           # 6-7 inside the first tile
        (270.0, 17.0), (290.0, 18.5),       # 8-9 inside the last tile
        (2.0, 1.0), (297.0, 18.0),          # 10-11 through every tile
        (-9.0, 6.0), (6.0, 9.0),            # 12-13 from off the left
        (310.0, 4.0), (292.0, 12.0),        # 14-15 from off the right
        (60.0, -7.0), (66.0, 4.0),          # 16-17 from above
        (200.0, 27.0), (190.0, 15.0),       # 18-19 from below
        (255.5, 7.5), (256.0, 15.5),        # 20-21 ends on the tile corners
        (-30.0, -30.0), (330.0, 50.0),      # 22-23 both ends off the frame, through it
    ]
    tracks = _still(joints, T, rng)
    P = tracks.shape[0]
    skeleton = np.array([(2 * i, 2 * i + 1) for i in range(P // 2)] + [(1, 20), (21, 9), (3, 4)], np.int32)
    return dict(frames=RC.frames_u8(rng, T, H, W), tracks=tracks, visibles=rng.random((P, T)) > 0.05,
                colors=rng.integers(0, 256, (P, 3)).astype(np.uint8), radius=1, skeleton=skeleton,
                limb_colors=rng.integers(0, 256, (skeleton.shape[0], 3)).astype(np.uint8), limb_width=limb_width)


def _degenerate():
    T, H, W = 2, 12, 24
    rng = np.random.default_rng(32)
    n, i, big, lim = np.nan, np.inf, 1e30, 2.0 ** 20
    ends = [(n, 4.0), (5.0, n), (i, 3.0), (3.0, -i), (big, 6.0), (6.0, -big), (lim, 5.0), (7.0, -lim), (lim - 1.0, 8.0)]
    anchors = [(3.0 + 2.0 * k, 2.0 + k) for k in range(len(ends))]
    joints = ends + anchors + [(12.0, 6.0), (18.0, 9.0), (15.5, 3.5), (15.5, 3.5), (20.0, 2.0)]
    E0 = len(ends)
    tracks = np.repeat(np.asarray(joints, np.float64)[:, None, :], T, 1)
    P = tracks.shape[0]
    skeleton = [(k, E0 + k) for k in range(E0)]                         # a refused end against a good one (the last: just below 2^20, drawn)
    skeleton += [(2 * E0, 2 * E0 + 1), (2 * E0 + 1, 2 * E0 + 4)]        # drawn; one end invisible on frame 1
    skeleton += [(2 * E0 + 2, 2 * E0 + 3)]                              # two joints at one place: zero length, a disc
    skeleton += [(2 * E0 + 4, 2 * E0 + 4)]                              # a == b, a disc
    skeleton += [(2 * E0 + 1, 2 * E0)]                                  # an edge drawn twice, the other way round
    vis = np.ones((P, T), bool)
    vis[2 * E0 + 4, 1] = False
    return dict(frames=RC.frames_u8(rng, T, H, W), tracks=tracks, visibles=vis, colors=rng.integers(0, 256, (P, 3)).astype(np.uint8), radius=1,
                skeleton=np.asarray(skeleton, np.int32), limb_width=2.0)


def _rounds():
    T, H, W, P, E = 2, 20, 40, 25, 300
    rng = np.random.default_rng(33)
    tracks = _still(np.stack([rng.uniform(4.0, 36.0, P), rng.uniform(9.0, 14.0, P)], -1), T, rng, 0.5)   # every limb meets the tile of rows 8 .. 15
    pairs = [(a, b) for a in range(P) for b in range(P) if a != b]
    skeleton = np.asarray([pairs[k] for k in rng.permutation(len(pairs))[:E]], np.int32)
    return dict(frames=RC.frames_u8(rng, T, H, W), tracks=tracks, colors=rng.integers(0, 256, (P, 3)).astype(np.uint8), radius=1,
                skeleton=skeleton, limb_colors=rng.integers(0, 256, (E, 3)).astype(np.uint8), limb_width=1.0, limb_alpha=0.5)


def heat_values(rng, T, K, H, W, dtype):
    """(T, K, H, W): smooth bumps in [0, 1.6] with every special value of the rule planted: negative, above 1 / gain, NaN, +/-inf, denormal."""
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros((T, K, H, W), np.float64)
    for t in range(T):
        for k in range(K):
            cy, cx, s = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(2.0, 6.0)
            out[t, k] = 1.6 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) - 0.05
    out = out.astype(dtype)
    tiny = np.finfo(dtype).smallest_subnormal
    special = [-0.75, 3.0, np.nan, np.inf, -np.inf, tiny, -tiny, 0.0, 1.0, 0.5]
    flat = out.reshape(T, K, -1)
    for t in range(T):
        for k in range(K):
            at = rng.choice(H * W, len(special), replace=False)
            flat[t, k, at] = special
    return out


def _heat(K, dtype, T=2, H=11, W=261, **kw):
    rng = np.random.default_rng(34 + K)
    return dict(frames=RC.frames_u8(rng, T, H, W), heat=heat_values(rng, T, K, H, W, dtype),
                heat_colors=rng.integers(0, 256, (K, 3)).astype(np.uint8), **kw)


def _all():
    m = RC._mixed(36, 3, 35, 57)
    rng = np.random.default_rng(37)
    P = m["tracks"].shape[0]
    skeleton = np.stack([np.arange(P - 1), np.arange(1, P)], -1).astype(np.int32)
    return dict(m, visibles=rng.random((P, 3)) > 0.1, skeleton=skeleton, limb_width=2.5, limb_alpha=0.75,
                heat=heat_values(rng, 3, 3, 35, 57, np.float32), heat_gain=1.5, heat_alpha=0.6)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for lw in (1.0, 2.0, 16.0):
        c[f"tiles_3x20x300_w{lw:g}"] = _tiles(lw)
    d = _degenerate()
    for la in (0.0, 0.5, 1.0):
        c[f"degenerate_2x12x24_a{la:g}"] = dict(d, limb_alpha=la)         # the default limb colour: joint b's
    r = _rounds()
    c["rounds_2x20x40"] = r
    c["rounds_2x20x40_reversed"] = dict(r, skeleton=r["skeleton"][::-1].copy(), limb_colors=r["limb_colors"][::-1].copy())
    c["rounds_2x20x40_e0"] = dict(r, skeleton=np.zeros((0, 2), np.int32), limb_colors=None)
    c["rounds_2x20x40_p0"] = dict(r, tracks=np.zeros((0, 2, 2)), colors=np.zeros((0, 3), np.uint8), skeleton=np.zeros((0, 2), np.int32),
                                  limb_colors=None)
    for K in (1, 3, 17):
        for dt in (np.float32, np.float64):
            c[f"heat_2x11x261_k{K}_{np.dtype(dt).name}"] = _heat(K, dt, heat_gain=2.0 if K == 3 else 1.0)
    c["heat_2x11x261_k3_alpha0"] = _heat(3, np.float32, heat_alpha=0.0)
    c["heat_2x11x261_k3_alpha1"] = _heat(3, np.float32, heat_alpha=1.0)
    a = _all()
    c["all_3x35x57"] = a                                                # overlay + heat + limbs + dots
    c["all_3x35x57_no_dots"] = dict({k: v for k, v in a.items() if k not in ("ids", "palette", "alpha", "contour")}, dots=False)
    c["all_3x35x57_default_colours"] = {k: v for k, v in a.items() if k not in ("colors", "heat_colors")}
    return c


POSE_KEYS = ("skeleton", "limb_colors", "limb_width", "limb_alpha", "heat", "heat_colors", "heat_gain", "heat_alpha")


def render(case, backend="host", **over):
    """A case through viz: render, or paint_pose for a case without dots."""
    c = dict(case, **over)
    if c.pop("dots", True):
        return viz.render(backend=backend, **c)
    frames, tracks = c.pop("frames"), c.pop("tracks", None)
    kw = {k: c.pop(k) for k in POSE_KEYS + ("visibles", "colors", "radius") if k in c}
    assert not c, sorted(c)
    return viz.paint_pose(frames, tracks, dots=False, backend=backend, **kw)


@functools.lru_cache(maxsize=None)
def expected(name: str) -> np.ndarray:
    """The host backend's frames of a case, computed once per session and shared (read-only)."""
    out = render(cases()[name])
    out.setflags(write=False)
    return out
