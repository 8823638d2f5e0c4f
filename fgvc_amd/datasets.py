"""TAP-Vid sample format (mmpt/datasets/tapvid.py:122-174) on synthetic clips, plus the strided per-rank sampler
(mmpt/datasets/samplers/distributed_sampler.py:53).  The real TAP-Vid / JHMDB files are not available offline;
`SyntheticTapVid` produces tensors with exactly the shapes, dtypes and conventions the model consumes:
    rgbs (1,T,3,h,w) float32 (stands for Lab-normalised frames), query_points (1,P,3) = (t,x,y) float32,
    trajectories (1,T,P,2) float32, visibilities (1,T,P) float32.
"""
from __future__ import annotations

import glob
import io
import os
import pickle

import numpy as np
import torch


class SyntheticTapVid:
    """Moving-texture clips with known point tracks: every frame is the first frame shifted by an integer
    (dx,dy) per frame, so ground-truth trajectories are exact and a tracker's accuracy is measurable.
    occluder=True: a STATIC textured rectangle (OCCLUDER_FRACTION of each side, seeded position and texture) is pasted over the frames
    t >= T // 2 -- after every query time, so that query points stay visible -- and the points under it are marked invisible in
    `visibilities`.  Everything else (the frames outside the rectangle, points, trajectories, queries) is the occluder=False sample.
    raw=True: the frames as a decoder would hand them over, `rgbs` (1, T, h, w, 3) uint8 = the same texture quantised to
    round(128 + 48 x) clamped to 0..255 -- for a tracker whose test_cfg.input = dict(type='rgb8'); the rest as before."""

    OCCLUDER_FRACTION = 0.4

    def __init__(self, n_videos=4, frames=8, size=(256, 256), points=8, query_mode="first", seed=0, device="cpu", occluder=False,
                 raw=False):
        self.n, self.T, self.h, self.w, self.P = n_videos, frames, size[0], size[1], points
        self.query_mode, self.seed, self.device = query_mode, seed, device
        self.occluder = bool(occluder)
        self.raw = bool(raw)

    def occluder_box(self, i):
        """(t_on, y0, y1, x0, x1) of video i's rectangle: present in frames t_on .. T-1, rows y0:y1, columns x0:x1 (None without one)."""
        if not self.occluder:
            return None
        g = torch.Generator().manual_seed(self.seed * 1000 + i + 500009)             # its own stream: the sample's draws stay as they are
        rh, rw = max(1, int(self.h * self.OCCLUDER_FRACTION)), max(1, int(self.w * self.OCCLUDER_FRACTION))
        y0 = int(torch.randint(0, self.h - rh + 1, (1,), generator=g))
        x0 = int(torch.randint(0, self.w - rw + 1, (1,), generator=g))
        return self.T // 2, y0, y0 + rh, x0, x0 + rw

    def _paste_occluder(self, i, rgbs, traj, vis):
        t_on, y0, y1, x0, x1 = self.occluder_box(i)
        g = torch.Generator().manual_seed(self.seed * 1000 + i + 700001)
        rh, rw = y1 - y0, x1 - x0
        tex = torch.nn.functional.interpolate(torch.randn(1, 3, rh // 4 + 2, rw // 4 + 2, generator=g), size=(rh, rw), mode="bilinear",
                                              align_corners=False)[0]
        tex = 1.5 * tex + 0.25 * torch.randn(tex.shape, generator=g)
        rgbs = rgbs.clone()
        rgbs[t_on:, :, y0:y1, x0:x1] = tex
        x, y = traj[..., 0], traj[..., 1]
        under = (x >= x0) & (x <= x1 - 1) & (y >= y0) & (y <= y1 - 1)
        under[:t_on] = False
        return rgbs, vis * (~under).float()

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000 + i)
        T, h, w, P = self.T, self.h, self.w, self.P
        pad = 2 * T
        base = torch.nn.functional.interpolate(torch.randn(1, 3, (h + 2 * pad) // 8 + 1, (w + 2 * pad) // 8 + 1, generator=g),
                                               size=(h + 2 * pad, w + 2 * pad), mode="bilinear", align_corners=False)[0]
        base = base + 0.25 * torch.randn(base.shape, generator=g)
        vx, vy = int(torch.randint(-2, 3, (1,), generator=g)), int(torch.randint(-2, 3, (1,), generator=g))
        rgbs = torch.stack([base[:, pad - vy * t: pad - vy * t + h, pad - vx * t: pad - vx * t + w] for t in range(T)], 0)
        t0 = torch.zeros(P) if self.query_mode == "first" else torch.randint(0, max(1, T // 2), (P,), generator=g).float()
        margin = 2 * T + 8
        x0 = torch.rand(P, generator=g) * (w - 2 * margin) + margin
        y0 = torch.rand(P, generator=g) * (h - 2 * margin) + margin
        ts = torch.arange(T).view(T, 1).float()
        traj = torch.stack([x0.view(1, P) + vx * (ts - t0.view(1, P)) + 0 * ts, y0.view(1, P) + vy * (ts - t0.view(1, P))], -1)
        # express the query at its own time: position at t0 is (x0,y0)
        qp = torch.stack([t0, x0, y0], -1)
        vis = (ts >= t0.view(1, P)).float()
        if self.occluder:
            rgbs, vis = self._paste_occluder(i, rgbs, traj, vis)
        d = self.device
        if self.raw:
            rgbs = (128.0 + 48.0 * rgbs).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()     # (T,h,w,3)
        return dict(rgbs=rgbs.unsqueeze(0).to(d), query_points=qp.unsqueeze(0).to(d),
                    trajectories=traj.unsqueeze(0).to(d), visibilities=vis.unsqueeze(0).to(d))


class StridedLoader:
    """indices[rank::world], one video per step (samples_per_gpu=1, tools/test.py:127)."""

    def __init__(self, dataset, rank=0, world=1):
        self.dataset, self.rank, self.world = dataset, rank, world
        self.total = len(dataset)

    def __iter__(self):
        for i in range(self.rank, len(self.dataset), self.world):
            yield self.dataset[i]

    def __len__(self):
        return len(range(self.rank, len(self.dataset), self.world))


# ---- TAP-Vid input contract (configs/eval/base_data.py:1-7: RGB2LAB + Normalize(mean=[50,0,0], std=[50,127,127])) -------
_M_RGB2XYZ = ((0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), (0.019334, 0.119193, 0.950227))
_WHITE_D65 = (0.950456, 1.0, 1.088754)


def rgb_to_lab(rgb: torch.Tensor) -> torch.Tensor:
    """sRGB in [0,1], (..., 3, h, w) float -> CIE L*a*b* (D65), L in [0,100], a/b in about [-127,127]: the conversion
    `cv2.cvtColor(img01_float32, cv2.COLOR_RGB2Lab)` performs in the reference (augmentation.py:1372-1391), with OpenCV's
    documented constants.  Parity with OpenCV is UNPINNED here (cv2 is not installed; its float path evaluates the
    transfer curve and the cube root through spline tables, documented accuracy ~1e-3): the known answers in
    tests/test_host.py are the CIE values of the sRGB primaries."""
    x = rgb.to(torch.float32)
    lin = torch.where(x > 0.04045, ((x + 0.055) / 1.055).clamp_min(0) ** 2.4, x / 12.92)
    r, g, b = lin.unbind(-3)
    xyz = [(m[0] * r + m[1] * g + m[2] * b) / w for m, w in zip(_M_RGB2XYZ, _WHITE_D65)]
    f = [torch.where(t > 0.008856, t.clamp_min(1e-12) ** (1.0 / 3.0), 7.787 * t + 16.0 / 116.0) for t in xyz]
    L = torch.where(xyz[1] > 0.008856, 116.0 * f[1] - 16.0, 903.3 * xyz[1])
    return torch.stack([L, 500.0 * (f[0] - f[1]), 200.0 * (f[1] - f[2])], -3)


def preprocess_tapvid_frames(frames_uint8: torch.Tensor, size=(256, 256)) -> torch.Tensor:
    """(T, h0, w0, 3) uint8 RGB -> (1, T, 3, h, w) float32 network input: bilinear resize to `size`, /255, RGB->Lab,
    (x - [50,0,0]) / [50,127,127]  (configs/eval/base_data.py:1-7; tapvid.py:106-108 scales the points by the same size)."""
    x = frames_uint8.permute(0, 3, 1, 2).to(torch.float32)
    if tuple(x.shape[-2:]) != tuple(size):
        x = torch.nn.functional.interpolate(x, size=size, mode="bilinear", align_corners=False)
    lab = rgb_to_lab((x / 255.0).clamp(0, 1))
    mean = torch.tensor([50.0, 0.0, 0.0], device=lab.device).view(1, 3, 1, 1)
    std = torch.tensor([50.0, 127.0, 127.0], device=lab.device).view(1, 3, 1, 1)
    return ((lab - mean) / std).unsqueeze(0)


def _label_imgs(frames_uint8: torch.Tensor, size, device, raw: bool = False) -> torch.Tensor:
    """(T, h0, w0, 3) uint8 -> the `imgs` of a label-map sample on `device`: (1, 1, 3, T, h, w) float32 through the input contract, or with
    raw=True the frames themselves, (1, 1, T, h0, w0, 3) uint8 (for test_cfg.input = dict(type='rgb8', size=size))."""
    if raw:
        return frames_uint8.to(device).unsqueeze(0).unsqueeze(0)
    rgbs = preprocess_tapvid_frames(frames_uint8.to(device), size)
    return rgbs.permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous()


# ---- TAP-Vid files (mmpt/datasets/tapvid.py:36-174, tapvid_evaluation_datasets.py:284-395) ---------------------------------
def _queries_first(occluded: np.ndarray, points: np.ndarray):
    """One query per track at its first visible frame; tracks that are never visible are dropped
    (tapvid_evaluation_datasets.py:352-395).  occluded (P,T) bool, points (P,T,2) = (x,y).  Returns (queries (Q,3) = (t,y,x),
    points (Q,T,2), occluded (Q,T))."""
    keep = (~occluded).any(axis=1)
    points, occluded = points[keep], occluded[keep]
    t0 = np.argmax(~occluded, axis=1)
    rows = np.arange(points.shape[0])
    q = np.stack([t0.astype(points.dtype), points[rows, t0, 1], points[rows, t0, 0]], axis=-1)
    return q, points, occluded


def _queries_strided(occluded: np.ndarray, points: np.ndarray, stride: int = 5):
    """A query at every `stride`-th frame for every track visible there; tracks are repeated per query
    (tapvid_evaluation_datasets.py:284-349)."""
    qs, ps, os_ = [], [], []
    for t in range(0, occluded.shape[1], stride):
        vis = ~occluded[:, t]
        qs.append(np.stack([np.full(int(vis.sum()), t, dtype=points.dtype), points[vis, t, 1], points[vis, t, 0]], axis=-1))
        ps.append(points[vis])
        os_.append(occluded[vis])
    return np.concatenate(qs, 0), np.concatenate(ps, 0), np.concatenate(os_, 0)


class TapVidPickles:
    """TAP-Vid videos from pickles in the sample format the model consumes (the reference's TAPVidDataset, tapvid.py:36-174).
    `root`: a directory of `*.pkl` files with one video each (what the reference globs, tapvid.py:66), or ONE pickle holding
    {name: video} or [video, ...] (the published tapvid_davis.pkl).  A video = dict(video (T,H,W,3) uint8 frames -- or an
    array of encoded JPEG byte strings, tapvid.py:91-99 --, points (P,T,2) = (x,y) in [0,1], occluded (P,T) bool).
    Frames go through the TAP-Vid input contract (`preprocess_tapvid_frames`: resize to `input_size`, RGB->Lab, normalise),
    points are scaled to `input_size` pixels (tapvid.py:106-108), queries are sampled by `query_mode` 'first' | 'strided'.
    raw=True: `rgbs` is the decoded video itself, (1, T, H, W, 3) uint8 on `device` at its own size, for a tracker whose
    test_cfg.input = dict(type='rgb8', size=input_size) resizes and converts it; everything else as before."""

    def __init__(self, root: str, query_mode: str = "first", input_size=(256, 256), device="cpu", raw=False):
        self.raw = bool(raw)
        if query_mode not in ("first", "strided"):
            raise ValueError(f"Unknown query mode {query_mode}.")                                   # tapvid.py:115
        self.query_mode, self.input_size, self.device = query_mode, tuple(input_size), device
        self.videos = []                       # (path, key): key = None for one-video files
        files = sorted(glob.glob(os.path.join(root, "*.pkl"))) if os.path.isdir(root) else [root]
        for f in files:
            with open(f, "rb") as fh:
                obj = pickle.load(fh)
            if isinstance(obj, dict) and "video" in obj:
                self.videos.append((f, None))
            elif isinstance(obj, dict):
                self.videos.extend((f, k) for k in obj)
            else:
                self.videos.extend((f, i) for i in range(len(obj)))
        self._open = (None, None)

    def __len__(self):
        return len(self.videos)

    def _raw(self, i):
        f, key = self.videos[i]
        if self._open[0] != f:
            with open(f, "rb") as fh:
                self._open = (f, pickle.load(fh))
        obj = self._open[1]
        return obj if key is None else obj[key]

    @staticmethod
    def _frames(video) -> torch.Tensor:
        if len(video) and isinstance(video[0], (bytes, bytearray)):                                  # JPEG bytes
            from PIL import Image
            video = np.stack([np.array(Image.open(io.BytesIO(b)).convert("RGB")) for b in video])
        return torch.from_numpy(np.ascontiguousarray(np.asarray(video, dtype=np.uint8)))

    def __getitem__(self, i):
        sample = self._raw(i)
        frames = self._frames(sample["video"])                                                      # (T,H,W,3) uint8
        h, w = self.input_size
        points = np.asarray(sample["points"], dtype=np.float32) * np.array([w, h], dtype=np.float32)   # tapvid.py:108
        occluded = np.asarray(sample["occluded"]).astype(bool)
        q, points, occluded = (_queries_first if self.query_mode == "first" else _queries_strided)(occluded, points)
        query_points = torch.from_numpy(q[:, [0, 2, 1]].astype(np.float32))                         # (t,y,x) -> (t,x,y), :132-133
        traj = torch.from_numpy(points).permute(1, 0, 2).contiguous()                               # (T,P,2)
        vis = ~torch.from_numpy(occluded).permute(1, 0).contiguous()                                # (T,P)
        P = query_points.shape[0]
        qt = query_points[:, 0].long()
        # Kubric reports query points on the crop boundary as invisible (tapvid.py:135-150)
        for p in range(P):
            if not vis[qt[p], p]:
                x, y = float(query_points[p, 1]), float(query_points[p, 2])
                xb, yb = min(abs(x), abs(x - (w - 1))) < 1e-3, min(abs(y), abs(y - (h - 1))) < 1e-3
                xin, yin = 0 <= x <= w - 1, 0 <= y <= h - 1
                if (xb and yin) or (xin and yb) or (xb and yb):
                    vis[qt[p], p] = True
        assert bool(vis[qt, torch.arange(P)].all()), "Query points must be visible"                # tapvid.py:160-161
        assert torch.allclose(query_points[:, 1:], traj[qt, torch.arange(P)], atol=1.0)             # tapvid.py:164-168
        if self.raw:
            rgbs = frames.to(self.device).unsqueeze(0)                                              # (1,T,H,W,3) uint8
        else:
            rgbs = preprocess_tapvid_frames(frames.to(self.device), self.input_size)                # (1,T,3,h,w)
        d = self.device
        return dict(rgbs=rgbs, query_points=query_points.unsqueeze(0).to(d), trajectories=traj.unsqueeze(0).to(d),
                    visibilities=vis.float().unsqueeze(0).to(d))


# ---- heat-map form of the pose samples (jhmdb_dataset.py:101-141, badja_dataset.py:350-410, augmentation.py:790-807) ----------------
def draw_label_map(img: np.ndarray, pt, sigma) -> np.ndarray:
    """The pose datasets' draw_label_map (jhmdb_dataset.py:282-309; badja_dataset.py:298-325 is the same with pt = (y, x), so call it
    with pt[::-1] there), restated: an unnormalised Gaussian patch of side 6 sigma + 1 (centre value 1) is ASSIGNED (not max-combined)
    into img (h, w) in place around pt = (x, y).  The patch corners are int() of pt -/+ 3 sigma (+ 1): truncation toward zero, so
    a point just left of / above the frame still draws a clipped patch; a patch entirely off the frame leaves img unchanged."""
    h, w = img.shape
    x_lo, y_lo = int(pt[0] - 3 * sigma), int(pt[1] - 3 * sigma)
    x_hi, y_hi = int(pt[0] + 3 * sigma + 1), int(pt[1] + 3 * sigma + 1)
    if x_lo >= w or y_lo >= h or x_hi < 0 or y_hi < 0:
        return img
    side = 6 * sigma + 1
    r = np.arange(0, side, 1, float)
    c = side // 2
    patch = np.exp(-((r[None, :] - c) ** 2 + (r[:, None] - c) ** 2) / (2 * sigma ** 2))
    px0, px1 = max(0, -x_lo), min(x_hi, w) - x_lo
    py0, py1 = max(0, -y_lo), min(y_hi, h) - y_lo
    img[max(0, y_lo):min(y_hi, h), max(0, x_lo):min(x_hi, w)] = patch[py0:py1, px0:px1]
    return img


def _cv2_linear_taps(n_in: int, n_out: int):
    """Source indices and weights of OpenCV's INTER_LINEAR along one axis (resize.cpp, float / double images): the coordinate
    (d + 0.5) * (n_in / n_out) - 0.5 is computed in double and rounded to float, its floor is the first tap and the float remainder the
    second tap's weight; a coordinate below 0 snaps to (0, weight 0), one at or past n_in - 1 to (n_in - 1, weight 0).  The weights are
    float, the interpolation is done in the image's depth (double for float64)."""
    f = ((np.arange(n_out, dtype=np.float64) + 0.5) * (n_in / n_out) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    lo, hi = s < 0, s >= n_in - 1
    f[lo | hi] = 0.0
    s[lo] = 0
    s[hi] = n_in - 1
    return s, np.minimum(s + 1, n_in - 1), (np.float32(1.0) - f).astype(np.float32), f


def cv2_resize_linear(img: np.ndarray, size) -> np.ndarray:
    """cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR) of a float64 (h0, w0, K) image, restated (mmcv.imresize(...,
    'bilinear', backend='cv2'), augmentation.py:798-802).  PARITY UNPINNED: cv2 is not installed.  What the restatement assumes of
    OpenCV: the same size is a plain copy; otherwise a horizontal pass then a vertical pass, each a sum of two products in double with
    float weights (_cv2_linear_taps), rows clamped to the image; the vertical weights keep their fraction where the row index is
    clamped (row -1 and row 0 both read row 0).  Not covered: OpenCV's switch to INTER_AREA for an exact 2x downscale (the pose datasets
    only upsample their maps) and any fused multiply-add OpenCV's build may use."""
    h, w = size
    img = np.asarray(img, dtype=np.float64)
    if img.shape[:2] == (h, w):
        return img.copy()
    h0, w0 = img.shape[:2]
    xs0, xs1, xw0, xw1 = _cv2_linear_taps(w0, w)
    tmp = img[:, xs0] * xw0.astype(np.float64)[None, :, None] + img[:, xs1] * xw1.astype(np.float64)[None, :, None]
    fy = ((np.arange(h, dtype=np.float64) + 0.5) * (h0 / h) - 0.5).astype(np.float32)
    sy = np.floor(fy).astype(np.int64)
    fy = (fy - sy.astype(np.float32)).astype(np.float32)
    r0, r1 = np.clip(sy, 0, h0 - 1), np.clip(sy + 1, 0, h0 - 1)
    b0, b1 = (np.float32(1.0) - fy).astype(np.float64), fy.astype(np.float64)
    return tmp[r0] * b0[:, None, None] + tmp[r1] * b1[:, None, None]


def pose_heatmaps(points_xy: np.ndarray, shape, sigma, size) -> np.ndarray:
    """(K, 2) = (x, y) joints on a (h, w) = shape canvas -> (K, h', w') float64 heat maps at size = (h', w'): one draw_label_map per
    joint on its own zero map, then cv2_resize_linear to the network size, channels first (the layout Resize leaves, augmentation.py:807)."""
    h, w = shape
    maps = np.zeros((h, w, len(points_xy)), dtype=np.float64)
    for j, p in enumerate(points_xy):
        draw_label_map(maps[:, :, j], p, sigma)
    return np.ascontiguousarray(cv2_resize_linear(maps, size).transpose(2, 0, 1))


# ---- JHMDB (mmpt/datasets/jhmdb_dataset.py:72-141) -> the tracker's sample format -------------------------------------------------
class JhmdbPoses:
    """JHMDB pose videos in the sample format VanillaTracker.forward_test consumes.  The reference's JHMDB dataset yields
    `imgs` / `ref_seg_map` (jhmdb_dataset.py:112-141), which the released tracker does not accept;
    this is the adaptation the release lacks: the 15 joints of the FIRST frame become query points at t = 0.

    Files as the reference reads them (:72-96): `<list_path>/<split>_list.txt` with lines "<anno.mat> <frames dir>", both relative
    to `root`; frames `*.png`; the .mat holds `pos_img` (2, 15, T) = (x; y), 1-based (:125 "magic -1").  Frames are resized to
    `input_size` (test_pipeline_jhmdb: 320 x 320, keep_ratio=False) and go through the RGB->Lab contract; joints are scaled
    the same way.  `pose_prediction(sample, traj_pred)` maps a prediction back to the (2, 15, T) original-resolution array that
    `metrics.jhmdb_pck` (jhmdb_dataset.py:174-256) scores against `sample["gt_poses"]`.

    form="heatmap": the reference's own first-frame label instead (jhmdb_dataset.py:119-141, Resize augmentation.py:790-807): data =
    dict(imgs (1,1,3,T,h,w), ref_seg_map (1, 15, h, w) float64 = one draw_label_map Gaussian (sigma 4) per joint at the video's own
    resolution, resized to the network size by cv2_resize_linear (parity unpinned), img_meta = [dict(original_shape=(h0, w0))]).
    VanillaTracker.forward_test with test_cfg.coords=True returns the (2, 15, T) coordinates at (h0, w0) directly.

    raw=True: the frames stay uint8 at the video's own size on `device` -- rgbs (1, T, h0, w0, 3), imgs (1, 1, T, h0, w0, 3) -- for a
    tracker whose test_cfg.input = dict(type='rgb8', size=input_size); joints, maps and meta as before."""
    NUM_KEYPOINTS = 15
    SIGMA = 4

    def __init__(self, root: str, list_path: str = None, split: str = "val", input_size=(320, 320), device="cpu", form: str = "points",
                 raw=False):
        if form not in ("points", "heatmap"):
            raise ValueError(f"form={form!r}: 'points' or 'heatmap'")
        self.root, self.input_size, self.device, self.form = root, tuple(input_size), device, form
        self.raw = bool(raw)
        self.samples = []
        with open(os.path.join(list_path or root, f"{split}_list.txt")) as f:
            for line in f:
                if not line.strip():
                    continue
                anno, vname = line.strip("\n").split()
                frames = sorted(glob.glob(os.path.join(root, vname, "*.png")))
                if frames:
                    self.samples.append(dict(frames_path=frames, anno_path=os.path.join(root, anno), video_path=os.path.join(root, vname)))

    def __len__(self):
        return len(self.samples)

    def __getitem__(self, i):
        import scipy.io as sio
        from PIL import Image
        s = self.samples[i]
        frames = torch.from_numpy(np.stack([np.array(Image.open(p).convert("RGB")) for p in s["frames_path"]]))   # (T,h0,w0,3)
        T, h0, w0 = frames.shape[:3]
        gt = np.asarray(sio.loadmat(s["anno_path"])["pos_img"], dtype=np.float64) - 1.0                          # (2,15,Tg)
        Tg = gt.shape[-1]
        h, w = self.input_size
        scale = np.array([w / w0, h / h0]).reshape(2, 1, 1)
        gts = gt * scale
        n = min(T, Tg)                                                                                           # :205
        if self.form == "heatmap":
            heat = pose_heatmaps(gt[:, :, 0].T, (h0, w0), self.SIGMA, (h, w))                                   # (15, h, w) f64
            imgs = _label_imgs(frames[:n], self.input_size, self.device, self.raw)                              # (1,1,3,T,h,w)
            data = dict(imgs=imgs, ref_seg_map=torch.from_numpy(heat).unsqueeze(0).to(self.device), img_meta=[dict(original_shape=(h0, w0))])
            return data, dict(gt_poses=gt[:, :, :n], original_shape=(h0, w0))
        traj = torch.from_numpy(gts[:, :, :n]).permute(2, 1, 0).float().contiguous()                             # (T,15,2)
        qp = torch.cat([torch.zeros(self.NUM_KEYPOINTS, 1), traj[0]], 1)                                        # (15,3) = (0,x,y)
        rgbs = frames[:n].to(self.device).unsqueeze(0) if self.raw else preprocess_tapvid_frames(frames[:n].to(self.device), self.input_size)
        d = self.device
        return dict(rgbs=rgbs, query_points=qp.unsqueeze(0).to(d), trajectories=traj.unsqueeze(0).to(d),
                    visibilities=torch.ones(1, n, self.NUM_KEYPOINTS, device=d)), dict(gt_poses=gt[:, :, :n], original_shape=(h0, w0))

    def pose_prediction(self, meta, traj_pred) -> np.ndarray:
        """traj_pred (1,T,15,2) at the network input size -> (2,15,T) at the video's own resolution."""
        h0, w0 = meta["original_shape"]
        h, w = self.input_size
        p = np.asarray(traj_pred.cpu() if hasattr(traj_pred, "cpu") else traj_pred, dtype=np.float64)[0]            # (T,15,2)
        return p.transpose(2, 1, 0) * np.array([w0 / w, h0 / h]).reshape(2, 1, 1)


def jhmdb_evaluate(model, dataset: "JhmdbPoses"):
    """Run the tracker over a JhmdbPoses dataset and score PCK@0.1..0.5 as the reference's pck_evaluate does."""
    from . import metrics
    preds, gts = [], []
    for i in range(len(dataset)):
        sample, meta = dataset[i]
        out = model(test_mode=True, **sample)
        assert torch.equal(out[4], sample["query_points"])              # every query is at t = 0: one group, order kept
        pred = out[2]
        preds.append(dataset.pose_prediction(meta, pred))
        gts.append(meta["gt_poses"])
    return metrics.jhmdb_pck(preds, gts)


def jhmdb_evaluate_heatmap(model, dataset: "JhmdbPoses"):
    """The heat-map form (JhmdbPoses(form='heatmap'), a model whose test_cfg has coords=True): the (2, 15, T) coordinates the tracker
    returns at the video's own resolution go to metrics.jhmdb_pck as they are."""
    from . import metrics
    assert dataset.form == "heatmap", "jhmdb_evaluate_heatmap reads JhmdbPoses(form='heatmap')"
    preds, gts = [], []
    for i in range(len(dataset)):
        data, meta = dataset[i]
        preds.append(np.asarray(model(test_mode=True, **data)[0], dtype=np.float64))
        gts.append(meta["gt_poses"])
    return metrics.jhmdb_pck(preds, gts)


def img2coord_maps(maps: np.ndarray, topk: int = 5) -> np.ndarray:
    """img2coord (vanilla_tracker.py:172-191) of a returned stack (T, K, h0, w0) -> (2, K, T) float64, with the read-out kernel's tie rule
    (fgvc_heatmap_coords_f32): the top 5 by value, the higher flat index first among equals (a stable ascending argsort's tail; numpy's
    default sort leaves that order open), normalised in the stack's dtype, coordinates summed in float64 in ascending order of value.
    A map whose float64 sum is 0 gives (-1, -1) (the reference sums in the stack's dtype: the same test for non-negative maps)."""
    maps = np.asarray(maps)
    T, K, h, w = maps.shape
    coords = np.zeros((2, K, T), dtype=np.float64)
    for f in range(T):                                                    # per frame: the argsort's indices are 8 bytes per value
        flat = maps[f].reshape(K, -1)
        order = np.argsort(flat, axis=-1, kind="stable")[:, -topk:]
        v = np.take_along_axis(flat, order, axis=-1)
        v = v / (np.sum(v, keepdims=True, axis=-1) + maps.dtype.type(1e-9))
        coords[0, :, f] = np.sum((order % w) * v, axis=-1)
        coords[1, :, f] = np.sum((order // w) * v, axis=-1)
        coords[:, flat.sum(axis=-1, dtype=np.float64) == 0, f] = -1
    return coords


class MapsAsCoords:
    """A tracker whose test_cfg has return_maps=True, presented as one with coords=True: each call returns [img2coord_maps(maps)], so that
    jhmdb_evaluate_heatmap / badja_evaluate_heatmap score it unchanged.  `on_maps(i, maps)` sees the i-th call's (T, K, h0, w0) array."""

    def __init__(self, model, on_maps=None):
        self.model, self.on_maps, self.calls = model, on_maps, 0

    def __call__(self, **kw):
        maps = self.model(**kw)[0]
        if self.on_maps is not None:
            self.on_maps(self.calls, maps)
        self.calls += 1
        return [img2coord_maps(maps)]


# SMAL joints BADJA annotates (badja_dataset.py:71-82 `SMALJointInfo.annotated_classes`): 20 of the 37 per frame
BADJA_ANNOTATED = (8, 9, 10, 12, 13, 14, 15, 18, 19, 20, 22, 23, 24, 25, 28, 31, 32, 33, 35, 36)


class BadjaPoses:
    """BADJA animal videos in the sample format VanillaTracker.forward_test consumes.  Like the reference's JHMDB dataset, its
    BadjaDataset yields `imgs` / `ref_seg_map` (badja_dataset.py:355-410), which the released tracker does not accept (SURVEY.md
    section 8b): the joints of the FIRST frame become query points at t = 0.

    Files as the reference reads them (:152-229): `<list_path>/joint_annotations/*.json`, each a list of records with `image_path`,
    `segmentation_path` (their first 6 characters are dropped and the rest joined to `root`), `joints` (37 x (y, x)) and `visibility`;
    a video = the frames `JPEGImages/Full-Resolution/<animal>/%05d.jpg` from the first to the last annotated number, silhouettes
    `Annotations/Full-Resolution/<animal>/%05d.png`; frames without a record have no joints (:206-211).  Videos under `extra_videos`
    are skipped (:177); the reference's IGNORE_ANIMALS list is ONE string by a missing comma (:38-41) and ignores nothing -- same here.
    Frames are resized to `size` = (320, 512) (:355-362; the released pipeline's Resize(-1, 320) then changes nothing) and go through
    the RGB->Lab contract; joints are scaled the same way (:364-366, :489-494).  Image resizing is PIL's here, OpenCV's there: the
    adapter is restated from the file, "parity unpinned" (no BADJA data or mmcv offline).

    form="heatmap": the reference's own first-frame label instead (badja_dataset.py:350-410): data = dict(imgs (1,1,3,T,h,w),
    ref_seg_map (1, J, h, w) float64 = one draw_label_map Gaussian (sigma 3, point (y, x)) per joint on a (h // 2, w // 2) canvas at half
    the joint coordinates, resized to `size` by cv2_resize_linear (Resize, parity unpinned), img_meta = [dict(original_shape=size)]).

    raw=True: the frames stay uint8 at their own size on `device` -- rgbs (1, T, h0, w0, 3), imgs (1, 1, T, h0, w0, 3) -- for a tracker whose
    test_cfg.input = dict(type='rgb8', size=size); joints, maps and meta as before."""
    SIGMA, SCALE = 3, 2

    def __init__(self, root: str, list_path: str = None, size=(320, 512), length: int = -1, device="cpu", form: str = "points", raw=False):
        self.raw = bool(raw)
        import json
        if form not in ("points", "heatmap"):
            raise ValueError(f"form={form!r}: 'points' or 'heatmap'")
        self.root, self.size, self.length, self.device, self.form = root, tuple(size), int(length), device, form
        self.videos = []
        adir = os.path.join(list_path or root, "joint_annotations")
        for name in sorted(os.listdir(adir)):
            with open(os.path.join(adir, name)) as f:
                records = json.load(f)
            first, last = records[0]["segmentation_path"], records[-1]["segmentation_path"]
            if "extra_videos" in first:
                continue
            animal = first.split("/")[-2]
            lo, hi = int(first.split("/")[-1].split(".")[0]), int(last.split("/")[-1].split(".")[0])
            by_file = {os.path.join(root, r["image_path"][6:]): r for r in records}
            frames, segs, joints, vis = [], [], [], []
            for fr in range(lo, hi + 1):
                img = os.path.join(root, "JPEGImages/Full-Resolution/%s/%05d.jpg" % (animal, fr))
                r = by_file.get(img)
                frames.append(img)
                segs.append(os.path.join(root, r["segmentation_path"][6:]) if r else
                            os.path.join(root, "Annotations/Full-Resolution/%s/%05d.png" % (animal, fr)))
                joints.append(np.asarray(r["joints"], dtype=np.float64)[list(BADJA_ANNOTATED)] if r else None)
                vis.append(np.asarray(r["visibility"])[list(BADJA_ANNOTATED)] if r else None)
            if frames:
                self.videos.append(dict(name=animal, frames=frames, segs=segs, joints=joints, visibles=vis))

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, i):
        from PIL import Image
        v = self.videos[i]
        n = len(v["frames"]) if self.length == -1 else min(self.length, len(v["frames"]))
        imgs = [Image.open(p).convert("RGB") for p in v["frames"][:n]]
        w0, h0 = imgs[0].size
        h, w = self.size
        sy, sx = h / h0, w / w0
        frames = torch.from_numpy(np.stack([np.asarray(im) for im in imgs]))                       # (T,h0,w0,3)
        # silhouette -> the frame's size, then the network size.  The reference's first resize is cv2.resize(sil, (w, h), cv2.INTER_NEAREST)
        # (badja_dataset.py:255, :276): the flag sits in the `dst` position, so OpenCV runs its default, INTER_LINEAR -- when a mask and
        # its frame differ in size the `seg > 0` area (the PCK threshold) is the bilinear one.  Same size: both are the identity.
        segs = [np.asarray(Image.open(p).resize((w0, h0), Image.BILINEAR).resize((w, h), Image.NEAREST)) for p in v["segs"][:n]]
        joints = [None if j is None else j * np.array([sy, sx]) for j in v["joints"][:n]]          # (J,2) = (y,x) at the network size
        visibles = list(v["visibles"][:n])
        assert joints[0] is not None, "BADJA: the first frame of a video carries the query joints (badja_dataset.py:364)"
        J = joints[0].shape[0]
        traj = torch.zeros(n, J, 2)
        vis = torch.zeros(n, J)
        for t in range(n):
            if joints[t] is not None:
                traj[t] = torch.from_numpy(joints[t][:, ::-1].copy()).float()                      # (x,y)
                vis[t] = torch.from_numpy((np.asarray(visibles[t]) > 0).astype(np.float32))
        meta = dict(joints=joints, visibles=visibles, segs=segs, original_shape=(h0, w0), name=v["name"])
        if self.form == "heatmap":         # joints (y, x) at the network size, halved, drawn on the half-size canvas (:382-397)
            heat = pose_heatmaps(joints[0][:, ::-1] / self.SCALE, (h // self.SCALE, w // self.SCALE), self.SIGMA, (h, w))
            imgs = _label_imgs(frames, self.size, self.device, self.raw)
            return (dict(imgs=imgs, ref_seg_map=torch.from_numpy(heat).unsqueeze(0).to(self.device), img_meta=[dict(original_shape=(h, w))]),
                    meta)
        qp = torch.cat([torch.zeros(J, 1), traj[0]], 1)                                            # (J,3) = (0,x,y)
        rgbs = frames.to(self.device).unsqueeze(0) if self.raw else preprocess_tapvid_frames(frames.to(self.device), self.size)
        d = self.device
        return (dict(rgbs=rgbs, query_points=qp.unsqueeze(0).to(d), trajectories=traj.unsqueeze(0).to(d), visibilities=vis.unsqueeze(0).to(d)),
                dict(joints=joints, visibles=visibles, segs=segs, original_shape=(h0, w0), name=v["name"]))

    @staticmethod
    def pose_prediction(traj_pred) -> np.ndarray:
        """traj_pred (1,T,J,2) = (x,y) at the network size -> (2,J,T), the layout pck_evaluate reads (:526-527)."""
        p = np.asarray(traj_pred.cpu() if hasattr(traj_pred, "cpu") else traj_pred, dtype=np.float64)[0]
        return p.transpose(2, 1, 0)


def badja_evaluate(model, dataset: "BadjaPoses"):
    """Run the tracker over a BadjaPoses dataset and score PCK@0.1..0.4 as the reference's pck_evaluate does (BASELINE.md quotes its
    PCK@0.2)."""
    from . import metrics
    preds, js, vs, ss = [], [], [], []
    for i in range(len(dataset)):
        sample, meta = dataset[i]
        out = model(test_mode=True, **sample)
        assert torch.equal(out[4], sample["query_points"])              # every query is at t = 0: one group, order kept
        preds.append(dataset.pose_prediction(out[2]))
        js.append(meta["joints"]); vs.append(meta["visibles"]); ss.append(meta["segs"])
    return metrics.badja_pck(preds, js, vs, ss)


def badja_evaluate_heatmap(model, dataset: "BadjaPoses"):
    """The heat-map form (BadjaPoses(form='heatmap'), a model whose test_cfg has coords=True): the (2, J, T) coordinates at the network
    size go to metrics.badja_pck as they are."""
    from . import metrics
    assert dataset.form == "heatmap", "badja_evaluate_heatmap reads BadjaPoses(form='heatmap')"
    preds, js, vs, ss = [], [], [], []
    for i in range(len(dataset)):
        data, meta = dataset[i]
        preds.append(np.asarray(model(test_mode=True, **data)[0], dtype=np.float64))
        js.append(meta["joints"]); vs.append(meta["visibles"]); ss.append(meta["segs"])
    return metrics.badja_pck(preds, js, vs, ss)


class Davis2017:
    """DAVIS-2017 semi-supervised VOS in the sample format VanillaTracker.forward_test's mask path consumes (the reference's mask
    pipelines yield `imgs` / `ref_seg_map` / `img_meta`, configs/eval/base_data.py:15-39).

    Files: `ImageSets/2017/<split>.txt` (one sequence per line), `JPEGImages/480p/<seq>/*.jpg`, `Annotations/480p/<seq>/*.png` (palette
    PNGs: the palette index is the object id, 0 = background).  Frames go through the RGB->Lab + Normalize contract at their native size
    (no resize).  Item i = (data, meta): data = dict(imgs (1,1,3,T,h,w), ref_seg_map (1,h,w) uint8 = the first annotation,
    img_meta = [dict(original_shape=(h,w))]); meta = dict(name, gt (T,h,w) uint8 -- every annotation the set has, frames without
    one are all-zero -- n_objects).  raw=True: imgs (1, 1, T, h, w, 3) uint8 on `device`, the decoded frames themselves, for a tracker
    whose test_cfg.input = dict(type='rgb8'); everything else as before."""

    def __init__(self, root: str, split: str = "val", resolution: str = "480p", device="cpu", max_frames: int = -1, raw=False):
        self.raw = bool(raw)
        self.root, self.res, self.device, self.max_frames = root, resolution, device, int(max_frames)
        with open(os.path.join(root, "ImageSets", "2017", f"{split}.txt")) as f:
            self.sequences = [ln.strip() for ln in f if ln.strip()]

    def __len__(self):
        return len(self.sequences)

    def __getitem__(self, i):
        from PIL import Image
        seq = self.sequences[i]
        jdir = os.path.join(self.root, "JPEGImages", self.res, seq)
        adir = os.path.join(self.root, "Annotations", self.res, seq)
        names = sorted(os.path.splitext(n)[0] for n in os.listdir(jdir) if n.endswith(".jpg"))
        if self.max_frames > 0:
            names = names[:self.max_frames]
        frames = torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(jdir, n + ".jpg")).convert("RGB")) for n in names]))
        h, w = frames.shape[1:3]
        gt = np.zeros((len(names), h, w), np.uint8)
        for t, n in enumerate(names):
            p = os.path.join(adir, n + ".png")
            if os.path.exists(p):
                im = Image.open(p)
                gt[t] = np.asarray(im if im.mode in ("P", "L") else im.convert("L"))
        imgs = _label_imgs(frames, (h, w), self.device, self.raw)                         # (1,1,3,T,h,w), native size
        ref = torch.from_numpy(gt[0].copy()).unsqueeze(0).to(self.device)
        data = dict(imgs=imgs, ref_seg_map=ref, img_meta=[dict(original_shape=(h, w))])
        return data, dict(name=seq, gt=gt, n_objects=int(gt[0].max()))


def davis_evaluate(model, dataset: "Davis2017", backend: str = "host", boxes: bool = False) -> dict:
    """Run the mask path over the set and score it (metrics.davis_jf).  backend='hip': the counts behind J and F come from
    fgvc_jf_counts_u8; the annotation of a sequence is uploaded once, and a prediction the model returns on the device (test_cfg.masks=
    'device') is scored where it is.  boxes=True: every sequence also gets 'Box-IoU', metrics.mean_box_iou of the predicted against the
    annotated maps' boxes (on the same backend), and the result 'Box-IoU-Mean', their mean over the sequences."""
    from . import metrics
    hip = metrics._backend(backend)
    seqs, box_iou = {}, {}
    for i in range(len(dataset)):
        data, meta = dataset[i]
        pred = model(test_mode=True, **data)[0]
        gt = meta["gt"]
        if not hip and isinstance(pred, torch.Tensor):                  # (a model with test_cfg.masks='device', scored on the host)
            pred = pred.cpu().numpy()
        if hip and isinstance(gt, np.ndarray) and gt.dtype == np.uint8:
            gt = torch.from_numpy(gt).to(pred.device if isinstance(pred, torch.Tensor) and pred.is_cuda else "cuda")
        seqs[meta["name"]] = (gt, pred)
        if boxes:
            box_iou[meta["name"]] = metrics.mean_box_iou(gt, pred, int(gt.max()) + 1, backend=backend)
    jf = metrics.davis_jf(seqs, backend=backend)
    if boxes:
        for name, v in box_iou.items():
            jf["sequences"][name]["Box-IoU"] = v
        jf["Box-IoU-Mean"] = float(np.nanmean(list(box_iou.values()))) if np.isfinite(list(box_iou.values())).any() else float("nan")
    return jf


class YoutubeVos:
    """YouTube-VOS semi-supervised VOS, where an object is annotated at the frame it first appears in (parity unpinned: the data is not
    available offline, the layout is restated from the format's public description).

    Files under `root`: `JPEGImages/<video>/<frame>.jpg`, `Annotations/<video>/<frame>.png` (palette PNGs: index = object id) at least at
    the frames where objects first appear, and `meta.json` with videos.<video>.objects.<id>.frames = the frame names the object is asked
    for, the first of them its first appearance.  Item i = (data, meta): data = dict(imgs (1,1,3,T,h,w) -- or the uint8 frames with raw=True,
    as Davis2017 --, ref_seg_map = {frame index: (h, w) uint8 map} for a tracker whose test_cfg.refs is set, img_meta); meta = dict(name,
    frames = the frame names, gt (T, h, w) uint8 = every annotation on disk, zero elsewhere, has_gt (T,) bool, n_objects).
    A first frame of meta.json without a PNG, or whose PNG lacks the object, raises ValueError naming the video."""

    def __init__(self, root: str, device="cpu", max_frames: int = -1, raw=False):
        import json
        self.root, self.device, self.max_frames, self.raw = root, device, int(max_frames), bool(raw)
        with open(os.path.join(root, "meta.json")) as f:
            self.meta = json.load(f)["videos"]
        self.videos = sorted(self.meta)

    def __len__(self):
        return len(self.videos)

    def __getitem__(self, i):
        from PIL import Image
        vid = self.videos[i]
        jdir, adir = os.path.join(self.root, "JPEGImages", vid), os.path.join(self.root, "Annotations", vid)
        names = sorted(os.path.splitext(n)[0] for n in os.listdir(jdir) if n.endswith(".jpg"))
        if self.max_frames > 0:
            names = names[:self.max_frames]
        frames = torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(jdir, n + ".jpg")).convert("RGB")) for n in names]))
        h, w = frames.shape[1:3]
        gt, has_gt = np.zeros((len(names), h, w), np.uint8), np.zeros(len(names), bool)
        for t, n in enumerate(names):
            p = os.path.join(adir, n + ".png")
            if os.path.exists(p):
                im = Image.open(p)
                gt[t], has_gt[t] = np.asarray(im if im.mode in ("P", "L") else im.convert("L")), True
        refs, n_objects = {}, 0
        for oid, obj in sorted(self.meta[vid]["objects"].items(), key=lambda kv: int(kv[0])):
            first, oid = obj["frames"][0], int(oid)
            if first not in names:
                if self.max_frames > 0:
                    continue                                      # the object enters after the frames that were kept
                raise ValueError(f"YoutubeVos: video {vid!r}: meta.json puts object {oid}'s first frame at {first!r}, which has no JPEG")
            t = names.index(first)
            if not has_gt[t] or not (gt[t] == oid).any():
                raise ValueError(f"YoutubeVos: video {vid!r}: meta.json puts object {oid}'s first frame at {first!r}, but "
                                 f"Annotations/{vid}/{first}.png {'does not show it' if has_gt[t] else 'does not exist'}")
            refs[t] = torch.from_numpy(gt[t].copy()).to(self.device)
            n_objects = max(n_objects, oid)
        if not refs:
            raise ValueError(f"YoutubeVos: video {vid!r} has no annotated object")
        imgs = _label_imgs(frames, (h, w), self.device, self.raw)
        data = dict(imgs=imgs, ref_seg_map=refs, img_meta=[dict(original_shape=(h, w))])
        return data, dict(name=vid, frames=names, gt=gt, has_gt=has_gt, n_objects=n_objects)


def ytvos_run(model, dataset: "YoutubeVos", out_dir: Optional[str] = None) -> dict:
    """Run the mask path (a tracker with test_cfg.refs) over the set.  out_dir: one palette PNG (the DAVIS palette) per frame in the
    submission layout, out_dir/Annotations/<video>/<frame>.png.  Videos whose every frame has an annotation on disk are scored with
    metrics.davis_jf (its frame rule); the returned dict holds `videos` (the names), and `jf` (that score, None when no video has
    ground truth beyond the given frames)."""
    from PIL import Image
    from . import metrics
    from .viz import davis_palette
    scored, done = {}, []
    for i in range(len(dataset)):
        data, meta = dataset[i]
        pred = model(test_mode=True, **data)[0]
        pred = pred.cpu().numpy() if isinstance(pred, torch.Tensor) else np.asarray(pred)
        ids = np.rint(pred).astype(np.uint8)
        if out_dir is not None:
            vdir = os.path.join(out_dir, "Annotations", meta["name"])
            os.makedirs(vdir, exist_ok=True)
            for t, n in enumerate(meta["frames"]):
                im = Image.fromarray(ids[t], mode="P")
                im.putpalette(davis_palette().tobytes())
                im.save(os.path.join(vdir, n + ".png"))
        if bool(meta["has_gt"].all()):
            scored[meta["name"]] = (meta["gt"], ids)
        done.append(meta["name"])
    return dict(videos=done, jf=metrics.davis_jf(scored) if scored else None)


FLO_MAGIC = 202021.25      # 'PIEH' read as a little-endian float32: the Middlebury .flo header


def write_flo(path, flow) -> None:
    """Middlebury .flo: the magic float, int32 width and height, then h x w (u, v) float32 pairs row by row, little-endian.  flow (2, h, w)
    (channel 0 = x, as the trackers return it) or (h, w, 2); numpy only."""
    f = np.asarray(flow)
    if f.ndim != 3 or 2 not in (f.shape[0], f.shape[2]):
        raise ValueError(f"write_flo: a flow of shape (2, h, w) or (h, w, 2), got {f.shape}")
    if f.shape[0] == 2:                                                   # (2, h, w) wins where both readings fit
        f = f.transpose(1, 2, 0)
    h, w = f.shape[:2]
    with open(path, "wb") as fh:
        np.array([FLO_MAGIC], "<f4").tofile(fh)
        np.array([w, h], "<i4").tofile(fh)
        np.ascontiguousarray(f, "<f4").tofile(fh)


def read_flo(path) -> np.ndarray:
    """-> (2, h, w) float32, channel 0 = x.  ValueError for a wrong magic number or a truncated file."""
    with open(path, "rb") as fh:
        head = fh.read(12)
        if len(head) != 12 or np.frombuffer(head[:4], "<f4")[0] != np.float32(FLO_MAGIC):
            raise ValueError(f"{path}: not a Middlebury .flo file (magic number)")
        w, h = (int(v) for v in np.frombuffer(head[4:], "<i4"))
        if w < 1 or h < 1:
            raise ValueError(f"{path}: size {w} x {h}")
        data = np.frombuffer(fh.read(), "<f4")
    if data.size != 2 * h * w:
        raise ValueError(f"{path}: {data.size} values for a {h} x {w} flow")
    return np.ascontiguousarray(data.reshape(h, w, 2).transpose(2, 0, 1)).astype(np.float32)


# ---- Y'CbCr video at 8..16 bits, 4:2:0 / 4:2:2 / 4:4:4: the input contract as torch ops (DESIGN.md sections 19 and 26) ----------------------
def _chroma_taps(n_luma: int, n: int, back: bool, device):
    """Chroma samples around every luma index of one axis: s = p / 2 - 0.25 (`back`) or p / 2, clamped to [0, n - 1] -> i0, i1, weight of i1."""
    p = torch.arange(n_luma, device=device, dtype=torch.float32)
    s = (p / 2 - (0.25 if back else 0.0)).clamp(0, n - 1)
    i0 = s.floor()
    return i0.long(), (i0.long() + 1).clamp(max=n - 1), s - i0


def _yuv_subsampling(subsampling):
    try:
        sx, sy = (int(s) for s in subsampling)
    except (TypeError, ValueError):
        raise ValueError(f"subsampling={subsampling!r}: (sub_x, sub_y), each 1 or 2") from None
    if sx not in (1, 2) or sy not in (1, 2):
        raise ValueError(f"subsampling={subsampling!r}: (sub_x, sub_y), each 1 or 2")
    return sx, sy


def yuv_samples(p: torch.Tensor, depth: int = 8, shift: int = 0) -> torch.Tensor:
    """A plane of uint8 / uint16 words -> its samples as f32: (word >> shift) & (2^depth - 1) -- P010 keeps its sample in the high bits
    (shift 6), a low-aligned format may carry anything above the depth.  (Through int32: torch has no shifts on uint16.)"""
    if p.dtype not in (torch.uint8, torch.uint16):
        raise TypeError(f"expected torch.uint8 or torch.uint16, got {p.dtype}")
    depth, shift = int(depth), int(shift)
    if not 8 <= depth <= 16 or shift < 0 or depth + shift > 8 * p.element_size():
        raise ValueError(f"depth={depth}, shift={shift}: depth 8..16 and depth + shift within the {8 * p.element_size()} bits of {p.dtype}")
    return ((p.to(torch.int32) >> shift) & ((1 << depth) - 1)).to(torch.float32)


def yuv_chroma_at_luma(c: torch.Tensor, h0: int, w0: int, subsampling=(2, 2), siting: str = "left") -> torch.Tensor:
    """One chroma plane (T, ceil(h0 / sub_y), ceil(w0 / sub_x)) of sample values -> its value at every luma pixel (T, h0, w0) f32.  A
    subsampled axis is interpolated bilinearly, edge clamped: vertically between the luma rows, horizontally on the even luma columns
    ('left': MPEG-2, H.264, HEVC) or between them ('center': JPEG, MPEG-1); a full-resolution axis takes the sample at the luma index and no
    arithmetic touches it.  Exact: sixteenths on integers below 2^16 are 20 bits at most."""
    if siting not in ("left", "center"):
        raise ValueError(f"siting={siting!r}: 'left' or 'center'")
    sx, sy = _yuv_subsampling(subsampling)
    c = c.to(torch.float32)

    def across(r):
        if sx == 1:
            return r
        x0, x1, lx = _chroma_taps(w0, c.shape[2], siting == "center", c.device)
        return (1 - lx) * r[:, :, x0] + lx * r[:, :, x1]
    if sy == 1:
        return across(c)
    y0, y1, ly = _chroma_taps(h0, c.shape[1], True, c.device)
    return (1 - ly)[:, None] * across(c[:, y0]) + ly[:, None] * across(c[:, y1])


def yuv_to_rgb(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, depth: int = 8, shift: int = 0, subsampling=(2, 2),
               matrix: str = "bt601", range: str = "limited", siting: str = "left") -> torch.Tensor:
    """Planes y (T, h0, w0), u, v (T, ceil(h0 / sub_y), ceil(w0 / sub_x)) of uint8 / uint16 words -> R'G'B' (T, 3, h0, w0) f32 on the 0..255
    scale, neither clamped nor rounded: samples by yuv_samples, chroma at the luma pixel, then yy = cy (Y - y_off), cb = U - c_off,
    cr = V - c_off, R = yy + crv cr, G = (yy + cgu cb) + cgv cr, B = yy + cbu cb with ops.yuv_coefficients_depth rounded to f32 -- one
    rounded f32 operation after another, the order the kernels keep.  CPU or GPU tensors."""
    from .ops import yuv_coefficients_depth
    y_off, cy, c_off, crv, cgu, cgv, cbu = (float(np.float32(c)) for c in yuv_coefficients_depth(matrix, range, depth))
    sx, sy = _yuv_subsampling(subsampling)
    T, h0, w0 = y.shape
    want = (T, (h0 + sy - 1) // sy, (w0 + sx - 1) // sx)
    if tuple(u.shape) != want or tuple(v.shape) != want:
        raise ValueError(f"u, v: chroma planes of shape {want} for luma {tuple(y.shape)} subsampled {(sx, sy)}, got {tuple(u.shape)} and "
                         f"{tuple(v.shape)}")
    yy = cy * (yuv_samples(y, depth, shift) - y_off)
    cb = yuv_chroma_at_luma(yuv_samples(u, depth, shift), h0, w0, (sx, sy), siting) - c_off
    cr = yuv_chroma_at_luma(yuv_samples(v, depth, shift), h0, w0, (sx, sy), siting) - c_off
    return torch.stack([yy + crv * cr, (yy + cgu * cb) + cgv * cr, yy + cbu * cb], 1)


def yuv_to_rgb8(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, depth: int = 8, shift: int = 0, subsampling=(2, 2),
                matrix: str = "bt601", range: str = "limited", siting: str = "left") -> torch.Tensor:
    """-> (T, h0, w0, 3) uint8: yuv_to_rgb clamped to [0, 255] and rounded half to even (what ops.yuv_planes_to_rgb8 computes)."""
    rgb = yuv_to_rgb(y, u, v, depth, shift, subsampling, matrix, range, siting)
    return rgb.clamp(0, 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def preprocess_yuv_frames(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, depth: int = 8, shift: int = 0, subsampling=(2, 2),
                          matrix: str = "bt601", range: str = "limited", siting: str = "left", size=None) -> torch.Tensor:
    """The same planes -> (1, T, 3, h, w) float32 network input: yuv_to_rgb, then preprocess_tapvid_frames' steps on the unclamped R'G'B'
    (bilinear resize to `size`, None = the frames' own; / 255 and clamp; RGB -> Lab; (x - [50, 0, 0]) / [50, 127, 127]).  The contract
    ops.yuv_planes_to_lab is held to."""
    x = yuv_to_rgb(y, u, v, depth, shift, subsampling, matrix, range, siting)
    if size is not None and tuple(x.shape[-2:]) != tuple(size):
        x = torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    lab = rgb_to_lab((x / 255.0).clamp(0, 1))
    mean = torch.tensor([50.0, 0.0, 0.0], device=lab.device).view(1, 3, 1, 1)
    std = torch.tensor([50.0, 127.0, 127.0], device=lab.device).view(1, 3, 1, 1)
    return ((lab - mean) / std).unsqueeze(0)


# 8-bit 4:2:0 (NV12 / I420 planes, section 19): the same contract at depth 8, shift 0, (2, 2) -- bit for bit what these were on their own
def yuv420_chroma_at_luma(c: torch.Tensor, h0: int, w0: int, siting: str = "left") -> torch.Tensor:
    """One chroma plane (T, ch, cw) uint8 -> its value at every luma pixel (T, h0, w0) f32: yuv_chroma_at_luma with both axes subsampled."""
    return yuv_chroma_at_luma(c, h0, w0, (2, 2), siting)


def yuv420_to_rgb(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, matrix: str = "bt601", range: str = "limited",
                  siting: str = "left") -> torch.Tensor:
    """Planes y (T, h0, w0), u, v (T, (h0 + 1) // 2, (w0 + 1) // 2) uint8 -> R'G'B' (T, 3, h0, w0) f32 on the 0..255 scale, neither clamped
    nor rounded: yuv_to_rgb of 8-bit 4:2:0 planes."""
    return yuv_to_rgb(y, u, v, 8, 0, (2, 2), matrix, range, siting)


def yuv420_to_rgb8(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, matrix: str = "bt601", range: str = "limited",
                   siting: str = "left") -> torch.Tensor:
    """-> (T, h0, w0, 3) uint8: yuv420_to_rgb clamped to [0, 255] and rounded half to even (what ops.yuv_frames_to_rgb8 computes)."""
    return yuv_to_rgb8(y, u, v, 8, 0, (2, 2), matrix, range, siting)


def preprocess_yuv420_frames(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, size=None, matrix: str = "bt601", range: str = "limited",
                             siting: str = "left") -> torch.Tensor:
    """8-bit YUV 4:2:0 planes -> (1, T, 3, h, w) float32 network input: preprocess_yuv_frames of them.  The contract ops.yuv_frames_to_lab
    is held to."""
    return preprocess_yuv_frames(y, u, v, 8, 0, (2, 2), matrix, range, siting, size)


# ---- the way out: RGB bytes -> 8-bit YUV 4:2:0, the output contract as torch ops -----------------------------------
def _chroma_filter(p: torch.Tensor, siting: str) -> torch.Tensor:
    """One channel (T, h0, w0) f32 of byte values -> its value at every chroma sample (T, (h0 + 1) // 2, (w0 + 1) // 2): vertically midway
    between the luma rows 2 j and 2 j + 1 (the position yuv420_chroma_at_luma assumes), horizontally midway between the columns 2 i and
    2 i + 1 ('center': the four added, x 0.25) or on column 2 i ('left': weights 1, 2, 1 over 2 i - 1 .. 2 i + 1 per row, the two rows added,
    x 0.125); rows and columns off the frame repeat the edge.  Exact: eighths on bytes."""
    T, h0, w0 = p.shape
    r0 = torch.arange((h0 + 1) // 2, device=p.device) * 2
    r1 = (r0 + 1).clamp(max=h0 - 1)
    c0 = torch.arange((w0 + 1) // 2, device=p.device) * 2
    cp, cm = (c0 + 1).clamp(max=w0 - 1), (c0 - 1).clamp(min=0)
    a, b = p[:, r0], p[:, r1]
    if siting == "center":
        return ((a[:, :, c0] + a[:, :, cp]) + (b[:, :, c0] + b[:, :, cp])) * 0.25
    top = (a[:, :, cm] + 2.0 * a[:, :, c0]) + a[:, :, cp]
    bot = (b[:, :, cm] + 2.0 * b[:, :, c0]) + b[:, :, cp]
    return (top + bot) * 0.125


def rgb8_to_yuv420(frames: torch.Tensor, matrix: str = "bt601", range: str = "limited", siting: str = "left"):
    """uint8 RGB frames (T, h0, w0, 3) -> (y (T, h0, w0), u, v (T, (h0 + 1) // 2, (w0 + 1) // 2)) uint8, odd sizes included: with
    ops.rgb_to_yuv_coefficients rounded to f32 and lum(R, G, B) = (kr R + kg G) + kb B, Y = y_off + sy lum(R, G, B) at every pixel; the R, G, B
    bytes filtered to the chroma sample (_chroma_filter) give L = lum(Rm, Gm, Bm), U = 128 + cu (Bm - L), V = 128 + cv (Rm - L); each byte is
    the value clamped to [0, 255] and rounded half to even.  One rounded f32 operation after another, nothing fused: the order
    ops.rgb_frames_to_yuv420 keeps and equals byte for byte.  CPU or GPU tensors."""
    from .ops import rgb_to_yuv_coefficients
    if siting not in ("left", "center"):
        raise ValueError(f"siting={siting!r}: 'left' or 'center'")
    kr, kg, kb, y_off, sy, cu, cv = (float(np.float32(c)) for c in rgb_to_yuv_coefficients(matrix, range))
    if frames.dtype != torch.uint8:
        raise TypeError(f"frames: expected torch.uint8, got {frames.dtype}")
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[1] == 0 or frames.shape[2] == 0:
        raise ValueError(f"frames: (T, h0, w0, 3) with h0, w0 > 0, got {tuple(frames.shape)}")
    R, G, B = (frames[..., c].to(torch.float32) for c in (0, 1, 2))

    def lum(r, g, b):
        return (kr * r + kg * g) + kb * b

    def byte(x):
        return x.clamp(0, 255).round().to(torch.uint8)
    y = y_off + sy * lum(R, G, B)
    Rm, Gm, Bm = (_chroma_filter(p, siting) for p in (R, G, B))
    L = lum(Rm, Gm, Bm)
    return byte(y), byte(128.0 + cu * (Bm - L)), byte(128.0 + cv * (Rm - L))


def pack_yuv420(y: torch.Tensor, u: torch.Tensor, v: torch.Tensor, fmt: str = "i420") -> torch.Tensor:
    """Planes y (T, h0, w0), u, v (T, h0 / 2, w0 / 2) uint8 -> packed frames (T, 3 h0 / 2, w0): the luma rows, then NV12's rows of
    interleaved (u, v) pairs or I420's u plane and v plane -- the inverse of ops.yuv420_planes.  ValueError for an odd size (no packed form)."""
    if fmt not in ("nv12", "i420"):
        raise ValueError(f"fmt={fmt!r}: one of ('nv12', 'i420')")
    if y.dim() != 3 or y.shape[1] == 0 or y.shape[2] == 0:
        raise ValueError(f"y: (T, h0, w0) with h0, w0 > 0, got {tuple(y.shape)}")
    T, h0, w0 = y.shape
    if h0 % 2 or w0 % 2:
        raise ValueError(f"y: a {h0} x {w0} frame has no packed {fmt} form (an odd side)")
    want = (T, h0 // 2, w0 // 2)
    if tuple(u.shape) != want or tuple(v.shape) != want:
        raise ValueError(f"u, v: chroma planes of shape {want} for luma {tuple(y.shape)}, got {tuple(u.shape)} and {tuple(v.shape)}")
    if any(p.dtype != torch.uint8 for p in (y, u, v)):
        raise TypeError(f"y, u, v: expected torch.uint8, got {y.dtype}, {u.dtype}, {v.dtype}")
    c = torch.stack([u, v], -1 if fmt == "nv12" else 1).reshape(T, h0 // 2, w0)
    return torch.cat([y, c], 1).contiguous()


# ---- Y4M files: progressive planar frames, 8 to 12 bits, 4:2:0 / 4:2:2 / 4:4:4 (DESIGN.md sections 19 and 26) -------------------------------
Y4M_MAGIC = b"YUV4MPEG2"
# a Y4M chroma tag -> (format: a ops.YUV_PIXEL_FORMATS name or 'i420', siting)
_Y4M_PLANES = {"420jpeg": ("i420", "center"), "420mpeg2": ("i420", "left"), "420": ("i420", "left"),
               "422": ("yuv422p", "left"), "444": ("yuv444p", "left"),
               "420p10": ("yuv420p10", "left"), "420p12": ("yuv420p12", "left"),
               "422p10": ("yuv422p10", "left"), "422p12": ("yuv422p12", "left"),
               "444p10": ("yuv444p10", "left"), "444p12": ("yuv444p12", "left")}
_Y4M_SITING = {tag: siting for tag, (fmt, siting) in _Y4M_PLANES.items() if fmt == "i420"}       # the 8-bit 4:2:0 tags: what read_y4m takes
_Y4M_TAGS = {fmt: tag for tag, (fmt, _) in _Y4M_PLANES.items() if fmt != "i420"}


def _y4m_format(fmt: str):
    """-> (sub_x, sub_y, depth, numpy dtype of a stored sample) of 'i420' or a planar ops.YUV_PIXEL_FORMATS name."""
    from .ops import YUV_PIXEL_FORMATS
    if fmt == "i420":
        return 2, 2, 8, np.dtype(np.uint8)
    _, sx, sy, depth, _, dtype = YUV_PIXEL_FORMATS[fmt]
    return sx, sy, depth, np.dtype("<u2") if dtype == torch.uint16 else np.dtype(np.uint8)


def _y4m_header(fh, path):
    """The header line of an open YUV4MPEG2 file -> (width, height, fps, chroma tag ('420jpeg' where it has none), range).  ValueError for
    another signature, interlaced material, an XCOLORRANGE that is neither FULL nor LIMITED and a header without a size."""
    head = fh.readline(4096)
    tags = head.rstrip(b"\n").split(b" ")
    if tags[0] != Y4M_MAGIC or not head.endswith(b"\n"):
        raise ValueError(f"{path}: not a YUV4MPEG2 file (signature)")
    w = h = None
    fps, chroma, rng = (0, 0), "420jpeg", "limited"
    for tag in (t.decode("ascii", "replace") for t in tags[1:] if t):
        k, val = tag[0], tag[1:]
        if k == "W":
            w = int(val)
        elif k == "H":
            h = int(val)
        elif k == "F":
            num, _, den = val.partition(":")
            fps = (int(num), int(den or 1))
        elif k == "I" and val not in ("p", "?"):
            raise ValueError(f"{path}: interlaced material (I{val}) is not supported; deinterlace it first")
        elif k == "C":
            chroma = val
        elif k == "X" and val.upper().startswith("COLORRANGE="):
            rng = val[11:].lower()
            if rng not in ("full", "limited"):
                raise ValueError(f"{path}: XCOLORRANGE={val[11:]} (FULL or LIMITED)")
    if w is None or h is None or w < 1 or h < 1:
        raise ValueError(f"{path}: the header gives no frame size (W, H)")
    return w, h, fps, chroma, rng


def _read_y4m(path, max_frames, tags, supported: str):
    """What read_y4m and read_y4m_planes share: the file's frames as it holds them and read_y4m_planes' info; `tags`: the chroma tags taken,
    `supported`: what the refusal of another says they are."""
    with open(path, "rb") as fh:
        w, h, fps, chroma, rng = _y4m_header(fh, path)
        if chroma not in tags:
            raise ValueError(f"{path}: chroma tag C{chroma} is not supported ({supported})")
        fmt, siting = _Y4M_PLANES[chroma]
        sx, sy, depth, dt = _y4m_format(fmt)
        if w % sx or h % sy:
            raise ValueError(f"{path}: odd size {w} x {h}; a C{chroma} frame with an odd side on a subsampled axis has no packed form")
        rows = h + 2 * h // (sx * sy)
        n = rows * w * dt.itemsize
        frames = []
        while max_frames is None or len(frames) < max_frames:
            line = fh.readline(4096)
            if not line:
                break
            if not line.startswith(b"FRAME") or not line.endswith(b"\n"):
                raise ValueError(f"{path}: frame {len(frames)}: expected a FRAME header")
            data = fh.read(n)
            if len(data) != n:
                raise ValueError(f"{path}: frame {len(frames)} is truncated ({len(data)} of {n} bytes)")
            frames.append(np.frombuffer(data, dt))
    native = np.dtype(dt.type)                                                # (the words in host order)
    arr = np.stack(frames).reshape(len(frames), rows, w).astype(native) if frames else np.zeros((0, rows, w), native)
    return torch.from_numpy(arr.copy()), dict(width=w, height=h, fps=fps, siting=siting, range=rng, format=fmt, depth=depth)


def read_y4m_header(path) -> str:
    """The chroma tag of a YUV4MPEG2 file's header ('420jpeg' where it has none).  ValueError for a file whose header no reader here takes."""
    with open(path, "rb") as fh:
        return _y4m_header(fh, path)[3]


def read_y4m(path, max_frames=None):
    """A YUV4MPEG2 file of progressive 8-bit 4:2:0 frames -> (frames (T, 3 h / 2, w) uint8 tensor, packed I420 as the file holds them; info =
    dict(width, height, fps=(num, den), siting, range)).  C420jpeg and no C tag: siting 'center'; C420mpeg2 and C420: 'left'.
    XCOLORRANGE=FULL | LIMITED: range 'full' | 'limited', absent 'limited'.  ValueError that names the tag or the fact for any other chroma
    tag, interlaced material (It / Ib / Im), an odd size and a truncated frame.  `max_frames`: stop after that many."""
    frames, info = _read_y4m(path, max_frames, _Y4M_SITING, "8-bit 4:2:0 only: C420jpeg, C420mpeg2, C420")
    del info["format"], info["depth"]
    return frames, info


def read_y4m_planes(path, max_frames=None):
    """A YUV4MPEG2 file of progressive frames, 8 to 12 bits, 4:2:0 / 4:2:2 / 4:4:4 -> (frames (T, rows, w) in the file's own arrangement --
    the luma rows, then the u plane and the v plane: what ops.yuv_planes takes apart (ops.yuv420_planes for 'i420') -- uint8, or uint16
    from the file's little-endian words; info = read_y4m's keys plus format (an ops.YUV_PIXEL_FORMATS name, or 'i420') and depth).
    C420jpeg, C420mpeg2, C420 and no C tag as read_y4m reads them; C422, C444; C420p10, C420p12, C422p10, C422p12, C444p10, C444p12, siting
    'left'.  ValueError that names the tag or the fact for any other chroma tag (Cmono*, C411, C444alpha, C420paldv, ..), interlaced
    material, a side that is odd on a subsampled axis and a truncated frame.  `max_frames`: stop after that many."""
    return _read_y4m(path, max_frames, _Y4M_PLANES, "planar 4:2:0, 4:2:2 and 4:4:4 at 8, 10 or 12 bits: "
                     + ", ".join("C" + t for t in _Y4M_PLANES))


def write_y4m_planes(path, frames, format: str = "i420", fps=(30, 1), siting: str = "left", range: str = "limited") -> None:
    """read_y4m_planes' inverse: frames (T, rows, w) of 'i420' or a planar ops.YUV_PIXEL_FORMATS name, in its dtype (tensor or array), ->
    a YUV4MPEG2 file: progressive, square pixels, 16-bit samples as little-endian words, XCOLORRANGE=LIMITED | FULL.  'i420' writes
    C420mpeg2 ('left') or C420jpeg ('center'); the other tags have no siting, and a file of them reads back as 'left'.  ValueError for a
    semi-planar format (Y4M has none) and a shape that is no packed frame; TypeError for another dtype."""
    if format != "i420" and format not in _Y4M_TAGS:
        raise ValueError(f"write_y4m_planes: format={format!r} (Y4M holds planar frames: one of {('i420',) + tuple(_Y4M_TAGS)})")
    if siting not in ("left", "center") or range not in ("limited", "full"):
        raise ValueError(f"write_y4m_planes: siting={siting!r} ('left' | 'center'), range={range!r} ('limited' | 'full')")
    sx, sy, _, dt = _y4m_format(format)
    f = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if f.dtype != np.dtype(dt.type):
        raise TypeError(f"write_y4m_planes: expected {np.dtype(dt.type)} frames for {format}, got {f.dtype}")
    k = sx * sy
    if f.ndim != 3 or f.shape[1] == 0 or f.shape[2] == 0 or f.shape[1] * k % (k + 2):
        raise ValueError(f"write_y4m_planes: packed {format} frames (T, h (1 + 2 / {k}), w), got {f.shape}")
    h, w = f.shape[1] * k // (k + 2), f.shape[2]
    if h % sy or w % sx:
        raise ValueError(f"write_y4m_planes: odd size {h} x {w} on a subsampled axis of {format}")
    chroma = ("420mpeg2" if siting == "left" else "420jpeg") if format == "i420" else _Y4M_TAGS[format]
    with open(path, "wb") as fh:
        fh.write(f"YUV4MPEG2 W{w} H{h} F{int(fps[0])}:{int(fps[1])} Ip A1:1 C{chroma} XCOLORRANGE={range.upper()}\n".encode("ascii"))
        for frame in f:
            fh.write(b"FRAME\n")
            fh.write(np.ascontiguousarray(frame, dt).tobytes())


def write_y4m(path, frames, fps=(30, 1), siting: str = "left", range: str = "limited") -> None:
    """Packed I420 frames (T, 3 h / 2, w) uint8 (tensor or array) -> a YUV4MPEG2 file: write_y4m_planes of 'i420' -- progressive, square
    pixels, C420mpeg2 ('left') or C420jpeg ('center'), XCOLORRANGE=LIMITED | FULL.  ValueError for anything else."""
    f = frames.detach().cpu().numpy() if isinstance(frames, torch.Tensor) else np.asarray(frames)
    if f.ndim != 3 or f.dtype != np.uint8 or f.shape[1] % 3 or f.shape[2] % 2:
        raise ValueError(f"write_y4m: packed I420 frames (T, 3 h / 2, w) uint8 with h and w even, got {f.dtype} {f.shape}")
    write_y4m_planes(path, f, "i420", fps, siting, range)


# ---- MOTChallenge text files ----------------------------------------------------------------------------------------

def write_mot(path, tracks, ids=None) -> int:
    """Write an engine.ObjectTracks as a MOTChallenge text file (the layout restated from its public description; parity unpinned): one line
    per present object and frame, `frame, id, left, top, width, height, 1, -1, -1, -1` with frames counted from 1, in frame then id order.
    Only objects of id >= 1 are written (row 0 is the background).  ids: the id to write for every row of `tracks` (N integers; None: the
    row's own number).  Returns the number of lines."""
    boxes, present = tracks.boxes, tracks.present
    T, N = present.shape
    names = list(range(N)) if ids is None else [int(i) for i in ids]
    if len(names) != N:
        raise ValueError(f"ids: {N} integers to go with the tracks, got {len(names)}")
    lines = []
    for t in range(T):
        for o in range(1, N):
            if present[t, o]:
                x0, y0, x1, y1 = (int(v) for v in boxes[t, o])
                lines.append(f"{t + 1},{names[o]},{x0},{y0},{x1 - x0},{y1 - y0},1,-1,-1,-1\n")
    with open(path, "w") as f:
        f.writelines(lines)
    return len(lines)


def read_mot(path):
    """A MOTChallenge text file -> {id: {0-based frame: (x0, y0, x1, y1)}} with half-open integer boxes: write_mot's inverse (the columns after
    the box are not kept; blank lines are skipped)."""
    out = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if not line.strip():
                continue
            v = [c.strip() for c in line.split(",")]
            if len(v) < 6:
                raise ValueError(f"{path}:{n}: expected `frame, id, left, top, width, height, ...`, got {line.strip()!r}")
            frame, obj = int(v[0]), int(v[1])
            left, top, width, height = (int(round(float(c))) for c in v[2:6])
            out.setdefault(obj, {})[frame - 1] = (left, top, left + width, top + height)
    return out
