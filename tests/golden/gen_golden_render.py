"""Record the fixtures of the point painter (fgvc_amd/viz.py) from the reference, executed read-only in place.

    python tests/golden/gen_golden_render.py          # writes tests/golden/render_*.npz

The reference's `paint_point_track` and `_get_colors` (mmpt/datasets/flyingthingsplus/utils/visualize.py:70-155) are lifted out of their
module by AST at generation time -- the module itself imports absl and mediapy, absent here -- and run unchanged on numpy, colorsys and
random.  The painter draws its colour table at random: numpy.random and random are seeded, ONE `_get_colors(P)` call records the table,
both are seeded again and the painter is called, so the recorded table is the one the painter used.  Only data is stored: frames, tracks
(float64: the contract is the reference called with float64 tracks), visibles, colours, the painter's output.

Both cases hold three points stacked within one pixel of each other (order and the truncation after every point decide the result),
points up to 3 px outside every border (clamped and drawn at the edge), some invisible points, and rows of pure 0 and pure 255.
"""
from __future__ import annotations

import ast
import colorsys
import os
import random
import sys
from typing import List, Tuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle.ref_import import REF_ROOT  # noqa: E402

REL = "mmpt/datasets/flyingthingsplus/utils/visualize.py"
CASES = (("render_3x40x56", 3, 40, 56, 12, 1, 101), ("render_2x100x104", 2, 100, 104, 9, 2, 202))


def lift():
    src = open(os.path.join(REF_ROOT, REL)).read()
    names = ("_get_colors", "paint_point_track")
    body = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(n.name for n in body) == sorted(names), [n.name for n in body]
    mod = ast.Module(body, [])
    ast.fix_missing_locations(mod)
    ns = {"np": np, "colorsys": colorsys, "random": random, "List": List, "Tuple": Tuple}
    exec(compile(mod, "ref:" + REL, "exec"), ns)
    return ns["_get_colors"], ns["paint_point_track"]


def inputs(T, H, W, P, seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (T, H, W, 3), dtype=np.uint8)
    frames[:, 0], frames[:, 1], frames[:, H - 1], frames[:, H // 2] = 0, 255, 255, 0          # rows of pure 0 and pure 255
    tracks = np.stack([rng.uniform(4.0, W - 4.0, (P, T)), rng.uniform(4.0, H - 4.0, (P, T))], -1)
    # three points within one pixel of each other, on every frame
    tracks[1] = tracks[0] + rng.uniform(-0.5, 0.5, (T, 2))
    tracks[2] = tracks[0] + rng.uniform(-0.5, 0.5, (T, 2))
    # up to 3 px outside every border, and on the borders' corners
    tracks[3, :, 0], tracks[4, :, 0] = -rng.uniform(0.0, 3.0, T), W + rng.uniform(0.0, 3.0, T)
    tracks[5, :, 1], tracks[6, :, 1] = -rng.uniform(0.0, 3.0, T), H + rng.uniform(0.0, 3.0, T)
    tracks[7, 0], tracks[7, 1] = (-3.0, -3.0), (W + 3.0, H + 3.0)
    tracks[8, 0], tracks[8, 1] = (W - 0.5, 1.25), (0.0, H - 0.25)                            # on the 255 / 0 rows
    visibles = rng.random((P, T)) > 0.2
    visibles[:3], visibles[7], visibles[8] = True, True, True
    visibles[5, 0], visibles[2, T - 1] = False, False
    return frames, tracks.astype(np.float64), visibles


def main():
    get_colors, paint = lift()
    for name, T, H, W, P, radius, seed in CASES:
        assert int(round(min(H, W) * 0.015)) == radius
        frames, tracks, visibles = inputs(T, H, W, P, seed)
        np.random.seed(seed)
        random.seed(seed)
        colors = np.array(get_colors(P), dtype=np.uint8)
        np.random.seed(seed)
        random.seed(seed)
        out = paint(frames.copy(), tracks, visibles)
        assert out.dtype == np.uint8 and out.shape == frames.shape and (out != frames).any()
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, frames=frames, tracks=tracks, visibles=visibles, colors=colors, out=out, radius=np.int64(radius))
        print(name, os.path.getsize(path), "bytes;", int((out != frames).any(-1).sum()), "pixels painted")


if __name__ == "__main__":
    main()
