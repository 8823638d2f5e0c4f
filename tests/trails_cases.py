"""Shared cases of the trail renderer (fgvc_render_trails_u8), what it is held to -- viz.render(trail=..., backend='host')
-- and a plain restatement of the rule that shares no code with viz's trail stage: a per-pixel Python loop over scalar floats.

A case is the keyword arguments of viz.render (numpy arrays) plus, optionally, dots=False (then it goes through viz.paint_trails, which has
no overlay).  The shapes are the smallest at which the kernel can go wrong: a workgroup owns TILE = (8 rows, 256 columns), so segments cross
and end on the tile edges at x = 256 and y = 8, 16; the item list is filled 256 candidates at a time, so one case keeps more than 256 items in
ONE tile; and every way a segment is refused (NaN, the infinities, 1e30, an invisible end) sits next to segments that are drawn."""
import functools
import math

import numpy as np

from fgvc_amd import viz
from tests import render_cases as RC

TILE = RC.TILE


def _walk(rng, start, T, step):
    """(P, T, 2): every start point moved by a random step of up to `step` px a frame."""
    start = np.asarray(start, np.float64)
    moves = rng.uniform(-step, step, (start.shape[0], T, 2))
    moves[:, 0] = 0.0
    return start[:, None, :] + np.cumsum(moves, 1)


def _cross(linewidth):
    T, H, W = 5, 17, 258
    rng = np.random.default_rng(21)
    paths = [
        [(249.0, 3.0), (252.5, 4.0), (255.5, 7.5), (259.0, 9.0), (262.0, 6.0)],          # over x = 256; one end exactly on the corner (256, 8)
        [(255.5, 12.0), (255.5, 15.5), (251.0, 15.5), (255.5, 15.5), (257.5, 16.5)],     # ends on x = 256, y = 16 and on the corner (258, 17)
        [(100.0, 5.0), (100.0, 7.5), (100.5, 11.0), (101.0, 15.5), (101.0, 19.0)],       # down over y = 8 and y = 16, out of the bottom
        [(-0.5, 2.0), (-0.5, 9.0), (3.0, 16.5), (-0.5, -0.5), (5.0, -0.5)],              # on the left, bottom and top borders
        [(-6.0, 8.0), (2.0, 8.5), (-4.0, 3.0), (-9.0, 3.0), (-3.0, 12.0)],               # from outside on the left, and back out
        [(264.0, 8.0), (256.5, 7.0), (261.0, 12.0), (266.0, 1.0), (254.0, 2.0)],         # ... on the right
        [(50.0, -6.0), (52.0, 1.0), (55.0, -4.0), (58.0, -8.0), (60.0, 3.0)],            # ... above
        [(60.0, 23.0), (62.0, 15.0), (66.0, 21.0), (70.0, 25.0), (71.0, 14.0)],          # ... below
        [(10.0, 1.0), (200.0, 15.0), (20.0, 14.0), (257.0, 0.0), (128.0, 8.0)],          # long diagonals through both column tiles
        [(30.0, 7.5), (40.0, 7.5), (40.0, 7.5), (40.0, 15.5), (30.0, 15.5)],             # along y = 8 and y = 16 (and one step that does not move)
    ]
    tracks = np.concatenate([np.asarray(paths, np.float64), _walk(rng, np.stack([rng.uniform(0, W, 8), rng.uniform(0, H, 8)], -1), T, 6.0)])
    P = tracks.shape[0]
    return dict(frames=RC.frames_u8(rng, T, H, W), tracks=tracks, visibles=rng.random((P, T)) > 0.08,
                colors=rng.integers(0, 256, (P, 3)).astype(np.uint8), radius=1, trail=4, linewidth=linewidth)


def _rounds():
    T, H, W, P, L = 6, 20, 40, 70, 5
    rng = np.random.default_rng(22)
    start = np.stack([rng.uniform(6.0, 34.0, P), rng.uniform(9.5, 13.5, P)], -1)
    tracks = _walk(rng, start, T, 2.5)
    tracks[:, :, 1] = np.clip(tracks[:, :, 1], 8.5, 14.5)   # every segment lies inside the tile of rows 8 .. 15: 350 kept items on the last frame
    return dict(frames=RC.frames_u8(rng, T, H, W), tracks=tracks, colors=rng.integers(0, 256, (P, 3)).astype(np.uint8), radius=1, trail=L,
                linewidth=2.0, trail_fade=np.array([0.9, 0.7, 0.55, 0.35, 0.2]))


def _degenerate():
    T, H, W = 4, 12, 20
    rng = np.random.default_rng(23)
    n, i, big = np.nan, np.inf, 1e30
    tracks = np.asarray([
        [(3.0, 3.0), (3.0, 3.0), (3.0, 3.0), (8.0, 5.0)],          # zero-length segments, then a step
        [(10.0, 2.0), (n, 4.0), (12.0, 6.0), (14.0, 8.0)],         # NaN in the middle: the segments on both sides of it go
        [(5.0, 9.0), (7.0, n), (n, n), (9.0, 9.0)],
        [(15.0, 3.0), (i, 3.0), (15.0, 6.0), (15.0, -i)],          # the infinities
        [(2.0, 10.0), (big, 10.0), (4.0, 10.0), (4.0, -big)],      # finite, beyond 2^20
        [(18.0, 1.0), (16.0, 4.0), (2.0 ** 20, 4.0), (16.0, 9.0)],  # exactly 2^20: not drawn
        [(6.0, 6.0), (9.0, 7.0), (12.0, 6.5), (14.5, 10.0)],       # ends made invisible below
        [(1.0, 1.0), (18.0, 10.0), (1.0, 10.0), (18.0, 1.0)],      # all drawn
        [(11.5, 5.5), (11.5, 5.5), (11.5, 5.5), (11.5, 5.5)],      # never moves
    ], np.float64)
    P = tracks.shape[0]
    vis = np.ones((P, T), bool)
    vis[6, 1], vis[7, 0] = False, False
    return dict(frames=RC.frames_u8(rng, T, H, W), tracks=tracks, visibles=vis, colors=rng.integers(0, 256, (P, 3)).astype(np.uint8), radius=1,
                trail=8, linewidth=2.0)


def _mixed():
    m = RC._mixed(24, 3, 35, 57)
    rng = np.random.default_rng(25)
    P = m["tracks"].shape[0]
    tracks = _walk(rng, m["tracks"][:, 0], 3, 7.0)
    return dict(m, tracks=tracks, visibles=rng.random((P, 3)) > 0.1, trail=2, linewidth=2.5)


@functools.lru_cache(maxsize=None)
def cases():
    c = {}
    for lw in (1.0, 2.0, 3.5):
        c[f"cross_5x17x258_w{lw:g}"] = _cross(lw)
    c["rounds_6x20x40"] = _rounds()
    d = _degenerate()
    c["degenerate_4x12x20"] = d                                               # trail = 8 is longer than the history
    c["degenerate_4x12x20_trail1"] = dict(d, trail=1)
    c["degenerate_1x12x20"] = dict(d, frames=d["frames"][:1], tracks=d["tracks"][:, :1], visibles=d["visibles"][:, :1])    # T = 1: no segment
    c["degenerate_4x12x20_p0"] = dict(d, tracks=np.zeros((0, 4, 2)), visibles=np.zeros((0, 4), bool), colors=np.zeros((0, 3), np.uint8))
    m = _mixed()
    c["mixed_3x35x57"] = m                                                    # overlay + trails + dots
    c["mixed_3x35x57_no_dots"] = dict({k: v for k, v in m.items() if k != "ids"}, dots=False)
    c["mixed_3x35x57_time"] = dict(m, trail_color_by="time")
    c["mixed_3x35x57_f32"] = dict(m, tracks=m["tracks"].astype(np.float32))
    c["mixed_3x35x57_i64"] = dict(m, tracks=np.rint(m["tracks"]).astype(np.int64))
    return c


def render(case, backend="host", **over):
    """A case through viz: render, or paint_trails for a case without dots."""
    c = dict(case, **over)
    if c.pop("dots", True):
        return viz.render(backend=backend, **c)
    c = dict(c)
    frames, tracks = c.pop("frames"), c.pop("tracks")
    kw = dict(visibles=c.pop("visibles", None), colors=c.pop("colors", None), trail=c.pop("trail"), linewidth=c.pop("linewidth", 2.0),
              fade=c.pop("trail_fade", None), color_by=c.pop("trail_color_by", "track"), radius=c.pop("radius", None))
    assert not c, sorted(c)
    return viz.paint_trails(frames, tracks, dots=False, backend=backend, **kw)


@functools.lru_cache(maxsize=None)
def expected(name: str) -> np.ndarray:
    """The host backend's frames of a case, computed once per session and shared (read-only)."""
    out = render(cases()[name])
    out.setflags(write=False)
    return out


# ---- the rule, restated: scalar floats, one pixel at a time ---------------------------------------------------------------------------------------
def restate_trails(image_stack, tracks, visibles, colour_of, trail, linewidth, fade, whole_image=False):
    """Draws the trails of every frame into image_stack (T, H, W, 3) uint8 (a list of lists would do: only indexing is used).  colour_of(i, s)
    -> three ints.  Only pixels within ro + 2 of a segment's bounding box are visited (beyond ro the coverage is 0 and the pixel keeps its
    value); whole_image=True visits every pixel, to show that."""
    T, H, W = len(image_stack), len(image_stack[0]), len(image_stack[0][0])
    ro = linewidth / 2 + 0.5
    ri = max(linewidth / 2 - 0.5, 0.0)
    ro2 = ro * ro
    g = 1.0 / (ro2 - ri * ri)
    for t in range(T):
        for i in range(len(tracks)):
            for s in range(max(0, t - trail), t):
                if visibles is not None and not (visibles[i][s] and visibles[i][s + 1]):
                    continue
                four = [float(tracks[i][s][0]), float(tracks[i][s][1]), float(tracks[i][s + 1][0]), float(tracks[i][s + 1][1])]
                if not all(math.isfinite(q) and abs(q) < 2 ** 20 for q in four):
                    continue
                ax, ay, bx, by = four[0] + 0.5, four[1] + 0.5, four[2] + 0.5, four[3] + 0.5
                if whole_image:
                    ys, xs = range(H), range(W)
                else:
                    ys = range(max(0, int(min(ay, by) - ro - 2)), min(H, int(max(ay, by) + ro + 3)))
                    xs = range(max(0, int(min(ax, bx) - ro - 2)), min(W, int(max(ax, bx) + ro + 3)))
                dx = bx - ax
                dy = by - ay
                L2 = dx * dx + dy * dy
                colour = colour_of(i, s)
                f = float(fade[t - 1 - s])
                for py in ys:
                    for px in xs:
                        u = 0.0 if L2 == 0 else min(max(((px - ax) * dx + (py - ay) * dy) / L2, 0.0), 1.0)
                        ex = px - (ax + u * dx)
                        ey = py - (ay + u * dy)
                        d2 = ex * ex + ey * ey
                        cov = min(max((ro2 - d2) * g, 0.0), 1.0)
                        if cov <= 0:
                            continue
                        op = cov * f
                        for ch in range(3):
                            image_stack[t][py][px][ch] = int((1 - op) * float(image_stack[t][py][px][ch]) + op * float(colour[ch]))
    return image_stack


def restate(case, whole_image=False) -> np.ndarray:
    """A case by the restatement: viz's overlay (pinned by tests/test_render_host.py), the trails above, viz's dots (pinned there too)."""
    c = dict(case)
    dots = c.pop("dots", True)
    frames = c["frames"]
    T = frames.shape[0]
    out = viz.render(frames, ids=c["ids"], palette=c.get("palette"), alpha=c.get("alpha", 128), contour=c.get("contour", True)) if "ids" in c \
        else frames.copy()
    tracks = np.asarray(c["tracks"]).astype(np.float64)
    P = tracks.shape[0]
    colors = c["colors"] if c.get("colors") is not None else viz.track_colors(P)
    L = c["trail"]
    fade = c["trail_fade"] if c.get("trail_fade") is not None else [(L - age) / L for age in range(L)]
    if c.get("trail_color_by", "track") == "time":
        def colour_of(i, s):
            k = min(int(s / max(1, T - 2) * 256), 255)
            return (255, k, 255 - k)
    else:
        def colour_of(i, s):
            return colors[i]
    vis = c.get("visibles")
    restate_trails(out, tracks.tolist(), None if vis is None else vis.tolist(), colour_of, L, float(c.get("linewidth", 2.0)), fade, whole_image)
    if dots and P:
        out = viz.render(out, tracks=tracks, visibles=vis, colors=colors, radius=c.get("radius"))
    return out


@functools.lru_cache(maxsize=None)
def restated(name: str) -> np.ndarray:
    out = restate(cases()[name])
    out.setflags(write=False)
    return out
