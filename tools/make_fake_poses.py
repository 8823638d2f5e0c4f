#!/usr/bin/env python3
"""Write small synthetic JHMDB / BADJA sets in the layouts fgvc_amd.datasets.JhmdbPoses / BadjaPoses read (the reference's file layouts),
for end-to-end runs of tools/test.py --task jhmdb|badja without the real data.

    python tools/make_fake_poses.py OUT_DIR --task jhmdb [--videos 2 --frames 5]

Each video: a textured background with a textured blob that moves by a constant step per frame; the joints sit on the blob and move with
it, so a tracker has something to follow.  JHMDB: `val_list.txt`, `<video>/*.png` frames and `<video>.mat` with pos_img (2, 15, T),
1-based.  BADJA: `joint_annotations/<animal>.json` records (image_path / segmentation_path with a 6-character prefix, joints 37 x (y, x),
visibility), `JPEGImages/Full-Resolution/<animal>/%05d.jpg` frames and `Annotations/Full-Resolution/<animal>/%05d.png` silhouettes."""
from __future__ import annotations

import argparse
import json
import os

import numpy as np


def _video(rng, T, h, w, n_joints):
    yy, xx = np.mgrid[0:h, 0:w]
    bg = np.kron(rng.random((h // 8 + 2, w // 8 + 2, 3)), np.ones((8, 8, 1)))[:h, :w]
    tex = np.kron(rng.random((h // 4 + 2, w // 4 + 2, 3)), np.ones((4, 4, 1)))[:h, :w]
    c = rng.uniform([0.35 * h, 0.35 * w], [0.65 * h, 0.65 * w])
    v = rng.uniform(-1.5, 1.5, 2)
    r = rng.uniform([0.15 * h, 0.15 * w], [0.25 * h, 0.25 * w])
    offs = rng.uniform(-0.7, 0.7, (n_joints, 2)) * r
    frames, sils, joints = [], [], []
    for t in range(T):
        ct = c + t * v
        inside = ((yy - ct[0]) / r[0]) ** 2 + ((xx - ct[1]) / r[1]) ** 2 <= 1.0
        shift = np.roll(np.roll(tex, int(round(t * v[0])), 0), int(round(t * v[1])), 1)
        img = np.where(inside[..., None], 0.3 + 0.7 * shift, 0.6 * bg)
        frames.append((img * 255).astype(np.uint8))
        sils.append(inside.astype(np.uint8) * 255)
        joints.append(ct[None, :] + offs)                     # (J, 2) = (y, x)
    return frames, sils, np.stack(joints)


def make_jhmdb(root: str, videos: int = 2, frames: int = 5, size=(60, 80), seed: int = 0):
    import scipy.io as sio
    from PIL import Image
    rng = np.random.default_rng(seed)
    lines = []
    for v in range(videos):
        name = f"vid{v:02d}"
        os.makedirs(os.path.join(root, name), exist_ok=True)
        fr, _, joints = _video(rng, frames, size[0], size[1], 15)
        for t, f in enumerate(fr):
            Image.fromarray(f).save(os.path.join(root, name, f"{t + 1:05d}.png"))
        pos = joints[:, :, ::-1].transpose(2, 1, 0) + 1.0     # (2, 15, T) = (x; y), 1-based
        sio.savemat(os.path.join(root, name + ".mat"), {"pos_img": pos})
        lines.append(f"{name}.mat {name}")
    with open(os.path.join(root, "val_list.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    return [ln.split()[1] for ln in lines]


def make_badja(root: str, videos: int = 2, frames: int = 5, size=(64, 96), seed: int = 0):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "joint_annotations"), exist_ok=True)
    names = []
    for v in range(videos):
        animal = f"animal{v:02d}"
        jdir = os.path.join(root, "JPEGImages", "Full-Resolution", animal)
        adir = os.path.join(root, "Annotations", "Full-Resolution", animal)
        os.makedirs(jdir, exist_ok=True)
        os.makedirs(adir, exist_ok=True)
        fr, sils, joints = _video(rng, frames, size[0], size[1], 37)
        records = []
        for t in range(frames):
            Image.fromarray(fr[t]).save(os.path.join(jdir, f"{t:05d}.jpg"), quality=95)
            Image.fromarray(sils[t]).save(os.path.join(adir, f"{t:05d}.png"))
            if t % 2 == 0:                                    # every other frame annotated, as BADJA's sparse labels
                records.append(dict(image_path=f"BADJA/JPEGImages/Full-Resolution/{animal}/{t:05d}.jpg",
                                    segmentation_path=f"BADJA/Annotations/Full-Resolution/{animal}/{t:05d}.png",
                                    joints=joints[t].tolist(), visibility=[1] * 37))
        with open(os.path.join(root, "joint_annotations", animal + ".json"), "w") as f:
            json.dump(records, f)
        names.append(animal)
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--task", choices=["jhmdb", "badja"], required=True)
    ap.add_argument("--videos", type=int, default=2)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    fn = make_jhmdb if a.task == "jhmdb" else make_badja
    print(fn(a.out, videos=a.videos, frames=a.frames, seed=a.seed))


if __name__ == "__main__":
    main()
