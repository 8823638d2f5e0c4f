#!/usr/bin/env python3
"""Write a seeded synthetic DAVIS-2017 set (the layout fgvc_amd.datasets.Davis2017 reads): moving ellipses on a smooth random texture,
several objects per sequence, palette PNG annotations on every frame.

    python tools/make_fake_davis.py OUT_DIR [--sequences 2 --frames 8 --size 120 208 --objects 3 --seed 0]
"""
from __future__ import annotations

import argparse
import os

import numpy as np


def _texture(rng, h, w):
    base = rng.random((h // 8 + 2, w // 8 + 2, 3))
    big = np.kron(base, np.ones((8, 8, 1)))[:h, :w]
    return (40 + 120 * big + 20 * rng.random((h, w, 3))).astype(np.float64)


def make(out: str, sequences: int = 2, frames: int = 8, size=(120, 208), objects: int = 3, seed: int = 0, split: str = "val"):
    from PIL import Image
    rng = np.random.default_rng(seed)
    h, w = size
    palette = [0, 0, 0, 128, 0, 0, 0, 128, 0, 128, 128, 0, 0, 0, 128, 128, 0, 128, 0, 128, 128] + [255] * (768 - 21)
    names = [f"fake{s:02d}" for s in range(sequences)]
    os.makedirs(os.path.join(out, "ImageSets", "2017"), exist_ok=True)
    with open(os.path.join(out, "ImageSets", "2017", f"{split}.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    yy, xx = np.mgrid[0:h, 0:w]
    for name in names:
        jdir = os.path.join(out, "JPEGImages", "480p", name)
        adir = os.path.join(out, "Annotations", "480p", name)
        os.makedirs(jdir, exist_ok=True)
        os.makedirs(adir, exist_ok=True)
        bg = _texture(rng, h, w)
        obj = []
        for k in range(objects):
            obj.append(dict(c=np.array([rng.uniform(0.25, 0.75) * h, rng.uniform(0.2, 0.8) * w]),
                            v=rng.uniform(-1.5, 1.5, 2) * np.array([h, w]) / 120.0,
                            r=np.array([rng.uniform(0.1, 0.2) * h, rng.uniform(0.08, 0.16) * w]),
                            col=rng.uniform(0, 255, 3), tex=_texture(rng, h, w) * 0.3))
        for t in range(frames):
            img = bg.copy()
            ann = np.zeros((h, w), np.uint8)
            for k, o in enumerate(obj):                       # later objects occlude earlier ones
                c = o["c"] + t * o["v"]
                inside = ((yy - c[0]) / o["r"][0]) ** 2 + ((xx - c[1]) / o["r"][1]) ** 2 <= 1.0
                img[inside] = 0.7 * o["col"] + o["tex"][inside]
                ann[inside] = k + 1
            Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(os.path.join(jdir, f"{t:05d}.jpg"), quality=95)
            a = Image.fromarray(ann, mode="P")
            a.putpalette(palette)
            a.save(os.path.join(adir, f"{t:05d}.png"))
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--sequences", type=int, default=2)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(120, 208))
    ap.add_argument("--objects", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    print(make(a.out, a.sequences, a.frames, tuple(a.size), a.objects, a.seed))


if __name__ == "__main__":
    main()
