"""Evaluation arithmetic of the path's consumers -- host-side numpy, not a kernel; the DAVIS J&F functions can take
their integer pixel counts from the library instead (backend='hip': fgvc_jf_counts_u8).

* tapvid_metrics      : TAP-Vid occlusion accuracy / pts-within-threshold / Jaccard
                        (mmpt/datasets/tapvid_evaluation_datasets.py:106-249)
* trajectory_summary  : per-point summary used by TAPVidDataset.tapvid_evaluate
                        (mmpt/datasets/flyingthingsplus/utils/figures.py:179-296; docstring known answers :225-246)
* jhmdb_pck           : PCK@alpha with the 0.6 * ||bbox of visible GT joints|| normaliser
                        (mmpt/datasets/jhmdb_dataset.py:144-152, :174-256)
* tapvid_summaries / save_results : the per-point records and the on-disk files of TAPVidDataset.tapvid_evaluate
                        (mmpt/datasets/tapvid.py:198-350): summaries<dataset>.json, results_df<dataset>.csv, results_list<dataset>.pkl
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Sequence

import numpy as np

TAPVID_THRESHOLDS = (1, 2, 4, 8, 16)


def tapvid_metrics(query_points: np.ndarray, gt_occluded: np.ndarray, gt_tracks: np.ndarray,
                   pred_occluded: np.ndarray, pred_tracks: np.ndarray, query_mode: str = "first",
                   extra_thresholds: Iterable[float] = ()) -> Dict[str, np.ndarray]:
    """query_points (b,n,3)=(t,y,x) [only t is used]; gt/pred_occluded (b,n,T) bool; tracks (b,n,T,2)=(x,y).
    Returns per-video arrays of shape (b,), values in [0,1]."""
    b, n, T = gt_occluded.shape
    qt = np.round(query_points[..., 0]).astype(np.int64)
    evaluate = np.ones((b, n, T), dtype=bool)
    evaluate[np.arange(b)[:, None], np.arange(n)[None, :], qt] = False         # never score the query frame
    if query_mode == "first":
        # the reference indexes gt_occluded[i] (shape (n,T)) with np.where(...)[0][0]: the first POINT that has a
        # visible frame, and blanks evaluation_points[i, :that] -- reproduced as is
        for i in range(b):
            first = np.where(gt_occluded[i] == 0)[0][0]
            evaluate[i, :first] = False
    elif query_mode != "strided":
        raise ValueError("Unknown query mode " + query_mode)
    out = {}
    out["occlusion_accuracy"] = ((pred_occluded == gt_occluded) & evaluate).sum((1, 2)) / evaluate.sum()
    visible, pred_visible = ~gt_occluded.astype(bool), ~pred_occluded.astype(bool)
    d2 = ((pred_tracks - gt_tracks) ** 2).sum(-1)
    n_vis = (visible & evaluate).sum((1, 2))
    fracs, jacs = [], []
    for th in TAPVID_THRESHOLDS:
        within = d2 < th ** 2
        correct = within & visible
        frac = (correct & evaluate).sum((1, 2)) / n_vis
        tp = (correct & pred_visible & evaluate).sum((1, 2))
        fp = (((~visible) & pred_visible) | ((~within) & pred_visible)) & evaluate
        jac = tp / (n_vis + fp.sum((1, 2)))
        out[f"pts_within_{th}"], out[f"jaccard_{th}"] = frac, jac
        fracs.append(frac)
        jacs.append(jac)
    for th in extra_thresholds:
        out[f"pts_within_{th}"] = ((d2 < th ** 2) & visible & evaluate).sum((1, 2)) / n_vis
    out["average_jaccard"] = np.mean(np.stack(jacs, 1), 1)
    out["average_pts_within_thresh"] = np.mean(np.stack(fracs, 1), 1)
    return out


def _ade(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.linalg.norm(a - b, axis=-1).mean()) if len(a) else float("nan")


SUMMARY_EXTRA_THRESHOLDS = (0.01, 0.05, *[0.1 * (i + 1) for i in range(10)], *[(i + 1) for i in range(10)])   # figures.py:281-285


def _visible_chain(vis: np.ndarray, t: int):
    """Slice of the frames around query time t that are visible without interruption (figures.py:112-176)."""
    assert vis[t], "Query point must be visible"
    occ = np.nonzero(~vis)[0]
    after, before = occ[occ > t], occ[occ < t]
    return slice(int(before[-1]) + 1 if len(before) else 0, int(after[0]) if len(after) else len(vis))


def trajectory_summary(traj_gt, traj_pred, vis_gt, vis_pred, query_point, query_mode: str = "first", idx: str = None,
                       extra_thresholds: Iterable[float] = ()) -> Dict[str, float]:
    """One point: traj (T,2), vis (T,) bool, query_point (3,)=(t,x,y).  The record of the reference's compute_summary
    (figures.py:179-296): TAP-Vid numbers x100 (:289), ADEs in pixels, `idx` = "<iter>--<video_idx>--<point_idx_in_video>"."""
    traj_gt, traj_pred = np.asarray(traj_gt, np.float64), np.asarray(traj_pred, np.float64)
    vis_gt, vis_pred = np.asarray(vis_gt).astype(bool), np.asarray(vis_pred).astype(bool)
    s = {}
    if idx is not None:
        s["idx"] = idx
    s.update({"ade": _ade(traj_gt, traj_pred), "ade_visible": _ade(traj_gt[vis_gt], traj_pred[vis_gt])})
    t = int(query_point[0])
    if 0 <= t < len(vis_gt) and vis_gt[t]:
        ch = _visible_chain(vis_gt, t)
        s["ade_visible_chain"] = _ade(traj_gt[ch], traj_pred[ch])
        n_chain = ch.stop - ch.start
    else:
        s["ade_visible_chain"], n_chain = float("nan"), 0
    s.update({"n_timesteps": len(traj_gt), "n_timesteps_visible": int(vis_gt.sum()), "n_timesteps_visible_chain": n_chain})
    m = tapvid_metrics(np.asarray(query_point, np.float64)[None, None], ~vis_gt[None, None], traj_gt[None, None],
                       ~vis_pred[None, None], traj_pred[None, None], query_mode, extra_thresholds)
    s.update({k: float(v[0]) * 100 for k, v in m.items()})
    return s


def tapvid_evaluate(results: Sequence, query_mode: str = "first") -> Dict[str, float]:
    """results: list of the tracker's 5-tuples (trajectories (1,T,P,2), visibilities (1,T,P), trajectories_pred,
    visibilities_pred, query_points (1,P,3)) as produced by single_gpu_test / multi_gpu_test
    (tapvid.py:198-312).  Mean over all points of all videos."""
    rows = []
    for traj, vis, tp, vp, qp in results:
        traj, vis, tp, vp, qp = (np.asarray(x.cpu() if hasattr(x, "cpu") else x) for x in (traj, vis, tp, vp, qp))
        for p in range(traj.shape[2]):
            rows.append(trajectory_summary(traj[0, :, p], tp[0, :, p], vis[0, :, p] > 0.5, vp[0, :, p] > 0.5,
                                           qp[0, p], query_mode))
    keys = rows[0].keys() if rows else []
    return {k: float(np.nanmean([r[k] for r in rows])) for k in keys}


def tapvid_summaries(results: Sequence, query_mode: str = "first", input_size=(256, 256), size=(256, 256)):
    """The per-point records TAPVidDataset.tapvid_evaluate builds (tapvid.py:235-268): one per point of every video, coordinates
    scaled from the network input size back to the evaluation size (`size` = (h, w); :241-245), idx "<video>_<point>" fields
    iter / video_idx / point_idx_in_video as there.  Returns (summaries, results_list)."""
    summaries, results_list = [], []
    sx, sy = size[1] / input_size[1], size[0] / input_size[0]
    for vid, (traj, vis, tp, vp, qp) in enumerate(results):
        traj, vis, tp, vp, qp = (np.asarray(x.cpu() if hasattr(x, "cpu") else x, dtype=np.float64) for x in (traj, vis, tp, vp, qp))
        scale = np.array([sx, sy])
        for n in range(traj.shape[2]):
            rec = {"idx": f"{vid}_{n}", "iter": vid, "video_idx": 0, "point_idx_in_video": n,
                   "trajectory_gt": traj[0, :, n] * scale, "trajectory_pred": tp[0, :, n] * scale,
                   "visibility_gt": vis[0, :, n] > 0.5, "visibility_pred": vp[0, :, n] > 0.5, "query_point": qp[0, n]}
            results_list.append(rec)
            summaries.append(trajectory_summary(rec["trajectory_gt"], rec["trajectory_pred"], rec["visibility_gt"], rec["visibility_pred"],
                                                rec["query_point"], query_mode, idx=f"{vid}--0--{n}",
                                                extra_thresholds=SUMMARY_EXTRA_THRESHOLDS))
    return summaries, results_list


def save_results(summaries, results_list, output_dir: str, metadata: Dict) -> Dict[str, str]:
    """The files of the reference's save_results (tapvid.py:316-350), same names and formats: summaries<dataset>.json (list of
    records), results_df<dataset>.csv (pandas DataFrame.from_records(summaries).to_csv) and, when `results_list` is non-empty,
    results_list<dataset>.pkl.  (The figures the reference draws from the data frame are not produced.)  Returns the paths."""
    import json
    import os
    import pickle

    import pandas as pd
    dataset = metadata["dataset"]
    os.makedirs(output_dir, exist_ok=True)
    paths = {"summaries": os.path.join(output_dir, f"summaries{dataset}.json"),
             "results_df": os.path.join(output_dir, f"results_df{dataset}.csv")}
    with open(paths["summaries"], "w", encoding="utf8") as f:
        json.dump(summaries, f)
    pd.DataFrame.from_records(summaries).to_csv(paths["results_df"])
    if len(results_list) > 0:
        paths["results_list"] = os.path.join(output_dir, f"results_list{dataset}.pkl")
        with open(paths["results_list"], "wb") as f:
            pickle.dump(results_list, f)
    return paths


def jhmdb_pck(pred_poses: Sequence[np.ndarray], gt_poses: Sequence[np.ndarray],
              alphas: Sequence[float] = (0.1, 0.2, 0.3, 0.4, 0.5)) -> Dict[str, float]:
    """pred_poses / gt_poses: per video (2, J, T) arrays (x;y).  A joint counts where the PREDICTION's x > 0
    (jhmdb_dataset.py:219); distance / (0.6 * ||bbox of those joints' GT||); PCK = % of distances <= alpha per joint,
    then the mean over joints."""
    J = gt_poses[0].shape[1]
    dists = [[] for _ in range(J)]
    for pred, gt in zip(pred_poses, gt_poses):
        T = min(pred.shape[-1], gt.shape[-1])
        pred, gt = pred[..., :T], gt[..., :T]
        seen = pred[0] > 0                                                     # (J,T)
        hi = np.where(seen[None], gt, -1.0).max(axis=1)                        # (2,T)
        lo = np.where(seen[None], gt, 1e6).min(axis=1)
        box = 0.6 * np.linalg.norm(hi - lo, axis=0)                            # (T,)
        d = np.linalg.norm(pred - gt, axis=0) / box[None]
        for j in range(J):
            dists[j].extend(d[j, seen[j]].tolist())
    out = {}
    for a in alphas:
        per_joint = [100.0 * np.mean(np.asarray(dj) <= a) for dj in dists if len(dj)]
        out[f"PCK@{a}"] = float(np.mean(per_joint))
    return out


def badja_pck(pred_poses: Sequence[np.ndarray], joints: Sequence[Sequence[Optional[np.ndarray]]],
              visibles: Sequence[Sequence[Optional[np.ndarray]]], segs: Sequence[Sequence[np.ndarray]],
              ratios: Sequence[float] = (0.1, 0.2, 0.3, 0.4)) -> Dict[str, float]:
    """BADJA PCK as BadjaDataset.pck_evaluate computes it (badja_dataset.py:451-571).  Per video: pred_poses (2, J, T) = (x; y) at
    the evaluation size; joints[t] (J, 2) = (y, x) at that size or None for an unlabelled frame (then nothing is counted, :504-508);
    visibles[t] (J,); segs[t] the silhouette at that size.  A VISIBLE joint is correct at ratio r when its distance to the ground
    truth is < r * sqrt(number of silhouette pixels of that frame) (:541-546, strict).  Returns PCK@r over all counted joints of all
    videos (%), and "PCK@0.2 per-video mean": the mean of the per-video PCK@0.2 values (the number :552-557 / :578 write out --
    under the label 'PCK@0.1 AVG'; NaN as soon as one video has no visible labelled joint, as there)."""
    counts = {r: [] for r in ratios}
    per_video = []
    for pred, js, vs, ss in zip(pred_poses, joints, visibles, segs):
        mine = {r: [] for r in ratios}
        T = min(pred.shape[-1], len(js))
        for t in range(T):
            if js[t] is None:
                continue
            thr0 = math.sqrt(float((np.asarray(ss[t]) > 0).sum()))
            for j in range(js[t].shape[0]):
                if not vs[t][j] > 0:
                    continue
                d = math.sqrt((float(js[t][j, 1]) - float(pred[0, j, t])) ** 2 + (float(js[t][j, 0]) - float(pred[1, j, t])) ** 2)
                for r in ratios:
                    ok = d < r * thr0
                    counts[r].append(ok)
                    mine[r].append(ok)
        if 0.2 in mine:      # (a video without one visible labelled joint: the reference's np.mean([]) is NaN and stays in the average, :552-557)
            per_video.append(100.0 * float(np.mean(mine[0.2])) if mine[0.2] else float("nan"))
    out = {f"PCK@{r}": (100.0 * float(np.mean(counts[r])) if counts[r] else float("nan")) for r in ratios}
    out["PCK@0.2 per-video mean"] = float(np.mean(per_video)) if per_video else float("nan")
    return out


# ---- DAVIS-2017 semi-supervised J&F (mmpt/core/evaluation/metrics.py: db_eval_iou, db_eval_boundary, db_statistics, JFM) -----------
# The reference dilates boundaries with cv2.dilate and a skimage disk; neither is installed here, so the dilation is
# scipy.ndimage.binary_dilation with the same disk footprint (x^2 + y^2 <= r^2).  A symmetric footprint and a zero border make the two
# the same operation.

def db_eval_iou(annotation: np.ndarray, segmentation: np.ndarray, void_pixels: Optional[np.ndarray] = None):
    """Region similarity J: intersection over union of two binary masks (..., h, w); an empty union scores 1."""
    assert annotation.shape == segmentation.shape, (annotation.shape, segmentation.shape)
    a, s = annotation.astype(bool), segmentation.astype(bool)
    keep = np.ones_like(a) if void_pixels is None else ~void_pixels.astype(bool)
    inter = np.sum(a & s & keep, axis=(-2, -1))
    union = np.sum((a | s) & keep, axis=(-2, -1))
    with np.errstate(invalid="ignore", divide="ignore"):
        j = inter / union
    if np.ndim(j) == 0:
        return 1.0 if np.isclose(union, 0) else float(j)
    j = np.asarray(j, dtype=np.float64)
    j[np.isclose(union, 0)] = 1.0
    return j


def _seg2bmap(seg: np.ndarray) -> np.ndarray:
    """1-pixel-wide boundary map of a binary mask: a pixel is on the boundary when it differs from its east, south or south-east
    neighbour (the last row compares east only, the last column south only, the corner is never a boundary)."""
    s = seg.astype(bool)
    e, so, se = np.zeros_like(s), np.zeros_like(s), np.zeros_like(s)
    e[:, :-1], so[:-1, :], se[:-1, :-1] = s[:, 1:], s[1:, :], s[1:, 1:]
    b = (s ^ e) | (s ^ so) | (s ^ se)
    b[-1, :] = s[-1, :] ^ e[-1, :]
    b[:, -1] = s[:, -1] ^ so[:, -1]
    b[-1, -1] = False
    return b


def _disk(r: int) -> np.ndarray:
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return (x * x + y * y) <= r * r


def jf_radius(shape, bound_th: float = 0.008) -> int:
    """The disk radius of the boundary measure for masks of `shape` = (h, w): bound_th itself when it is >= 1 (pixels), else
    ceil(bound_th * the image diagonal)."""
    return int(bound_th if bound_th >= 1 else math.ceil(bound_th * np.linalg.norm(shape)))


def f_measure(foreground_mask: np.ndarray, gt_mask: np.ndarray, void_pixels: Optional[np.ndarray] = None,
              bound_th: float = 0.008) -> float:
    """Boundary F of one frame: precision / recall of the boundary pixels within a disk of ceil(bound_th * diagonal) pixels."""
    from scipy.ndimage import binary_dilation
    keep = np.ones(foreground_mask.shape, bool) if void_pixels is None else ~void_pixels.astype(bool)
    fg_b = _seg2bmap(foreground_mask.astype(bool) & keep)
    gt_b = _seg2bmap(gt_mask.astype(bool) & keep)
    fp = _disk(jf_radius(foreground_mask.shape, bound_th))
    fg_d = binary_dilation(fg_b, structure=fp) if fg_b.any() else fg_b
    gt_d = binary_dilation(gt_b, structure=fp) if gt_b.any() else gt_b
    n_fg, n_gt = int(fg_b.sum()), int(gt_b.sum())
    if n_fg == 0 and n_gt == 0:
        precision = recall = 1.0
    elif n_fg == 0:
        precision, recall = 1.0, 0.0
    elif n_gt == 0:
        precision, recall = 0.0, 1.0
    else:
        precision = float((fg_b & gt_d).sum()) / n_fg
        recall = float((gt_b & fg_d).sum()) / n_gt
    return 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)


BACKENDS = ("host", "hip")


def _backend(backend: str, void_pixels=None) -> bool:
    """True for 'hip' (after its refusals), False for 'host'."""
    if backend not in BACKENDS:
        raise ValueError(f"backend={backend!r}: one of {BACKENDS}")
    if backend == "host":
        return False
    if void_pixels is not None:
        raise NotImplementedError("backend='hip' does not take void_pixels (no caller passes them); use backend='host'")
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("backend='hip' needs a GPU (fgvc_jf_counts_u8 has no CPU path); use backend='host'")
    return True


def _device_ids(ids, n_objects: int):
    """Id maps (T, h, w) as the kernel reads them: a uint8 CUDA tensor is used in place; anything else goes through numpy as the host scorer
    reads it (rint; a value outside 1 .. n_objects is no object: 0) and is uploaded as uint8."""
    import torch
    if isinstance(ids, torch.Tensor) and ids.is_cuda:
        if ids.dtype != torch.uint8:
            raise TypeError(f"backend='hip': a device tensor of ids must be uint8, got {ids.dtype}")
        return ids
    m = np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)
    if m.dtype != np.uint8 or (m.size and int(m.max()) > n_objects):
        m = np.rint(m)                                        # (compared as it is: a float array is not widened to int64 first)
        m = np.where((m >= 1) & (m <= n_objects), m, 0).astype(np.uint8)
    return torch.from_numpy(np.ascontiguousarray(m)).cuda()


def jf_counts_hip(gt_ids, pred_ids, n_objects: int, radius: int) -> np.ndarray:
    """(T, n_objects, 6) int64 on the host: one ops.jf_counts call (fgvc_jf_counts_u8) on two (T, h, w) id maps."""
    from . import ops
    if not 0 <= n_objects <= 255:
        raise ValueError(f"backend='hip': {n_objects} objects (the kernel reads byte ids: at most 255)")
    return ops.jf_counts(_device_ids(gt_ids, n_objects), _device_ids(pred_ids, n_objects), n_objects, radius).cpu().numpy()


def jf_from_counts(counts):
    """counts (T, n, 6) integers as fgvc_jf_counts_u8 writes them (|G & S|, |G | S|, |b(S)|, |b(G)|, |b(S) & dil b(G)|, |b(G) & dil b(S)|)
    -> (J (T, n), F (T, n)) float64, by the expressions and branches of db_eval_iou and f_measure: the same bits."""
    c = np.asarray(counts.cpu() if hasattr(counts, "cpu") else counts).astype(np.int64)
    assert c.ndim == 3 and c.shape[2] == 6, c.shape
    inter, union = c[..., 0], c[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        J = np.asarray(inter / union, dtype=np.float64)
    J[np.isclose(union, 0)] = 1.0
    F = np.zeros(c.shape[:2], np.float64)
    for t in range(c.shape[0]):
        for o in range(c.shape[1]):
            n_fg, n_gt, hit_fg, hit_gt = (int(v) for v in c[t, o, 2:])
            if n_fg == 0 and n_gt == 0:
                precision = recall = 1.0
            elif n_fg == 0:
                precision, recall = 1.0, 0.0
            elif n_gt == 0:
                precision, recall = 0.0, 1.0
            else:
                precision = float(hit_fg) / n_fg
                recall = float(hit_gt) / n_gt
            F[t, o] = 0.0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
    return J, F


def _binary_u8(mask):
    """A binary mask (numpy, or a tensor on either side) as the uint8 id map of object 1, on the device."""
    import torch
    if isinstance(mask, torch.Tensor):
        return (mask != 0).to(torch.uint8).cuda()
    return torch.from_numpy(np.asarray(mask).astype(bool).astype(np.uint8)).cuda()


def db_eval_boundary(annotation: np.ndarray, segmentation: np.ndarray, void_pixels: Optional[np.ndarray] = None,
                     bound_th: float = 0.008, backend: str = "host"):
    """Boundary F of (h, w) masks (a float) or of (T, h, w) stacks (an array over T).  backend='hip': the counts come from one
    fgvc_jf_counts_u8 call (ops.jf_counts) and F from jf_from_counts -- the same value."""
    assert annotation.shape == segmentation.shape
    if _backend(backend, void_pixels):
        if annotation.ndim not in (2, 3):
            raise ValueError(f"db_eval_boundary: {annotation.ndim}-D masks")
        g, s = _binary_u8(annotation), _binary_u8(segmentation)
        stack = annotation.ndim == 3
        g, s = (g, s) if stack else (g[None], s[None])
        F = jf_from_counts(jf_counts_hip(g, s, 1, jf_radius(tuple(annotation.shape[-2:]), bound_th)))[1][:, 0]
        return F if stack else float(F[0])
    if annotation.ndim == 2:
        return f_measure(segmentation, annotation, void_pixels, bound_th)
    if annotation.ndim != 3:
        raise ValueError(f"db_eval_boundary: {annotation.ndim}-D masks")
    return np.array([f_measure(segmentation[t], annotation[t], None if void_pixels is None else void_pixels[t], bound_th)
                     for t in range(annotation.shape[0])])


def db_statistics(per_frame_values: np.ndarray):
    """(mean, recall = share of frames above 0.5, decay = mean of the first quarter - mean of the last) of per-frame values, NaNs
    ignored.  The quarters are the reference's: bin edges round(linspace(1, n, 5)) - 1, each bin including its upper edge."""
    v = np.asarray(per_frame_values, dtype=np.float64)
    with np.errstate(invalid="ignore"), _quiet():
        M = np.nanmean(v)
        O = np.nanmean(v > 0.5)
        ids = (np.round(np.linspace(1, len(v), 5) + 1e-10) - 1).astype(np.uint8)
        bins = [v[ids[i]:ids[i + 1] + 1] for i in range(4)]
        D = np.nanmean(bins[0]) - np.nanmean(bins[3])
    return M, O, D


class _quiet:
    def __enter__(self):
        import warnings
        self._w = warnings.catch_warnings()
        self._w.__enter__()
        warnings.simplefilter("ignore", category=RuntimeWarning)

    def __exit__(self, *a):
        return self._w.__exit__(*a)


def _jfm(J_of, F_of, n: int) -> Dict[str, list]:
    out = {k: [] for k in ("JM", "JR", "JD", "FM", "FR", "FD")}
    for o in range(n):
        for key, vals in (("J", J_of(o)), ("F", F_of(o))):
            m, r, d = db_statistics(vals)
            out[key + "M"].append(m)
            out[key + "R"].append(r)
            out[key + "D"].append(d)
    return out


def JFM(all_gt_masks: np.ndarray, all_res_masks: np.ndarray, num_objects: Optional[int] = None, backend: str = "host") -> Dict[str, list]:
    """Per-object J / F statistics of one sequence.  all_gt_masks, all_res_masks: (objects, T, h, w) binary (a result with fewer objects
    is padded with empty masks; more objects than the annotation is an error).  Returns {'JM','JR','JD','FM','FR','FD'}: lists over
    the objects.  backend='hip': the stacks may overlap, so each object is one fgvc_jf_counts_u8 call with n_objects = 1; the statistics
    stay on the host."""
    if _backend(backend):
        gt, res = all_gt_masks, all_res_masks
        if res.shape[0] > gt.shape[0]:
            raise ValueError("JFM: the result has more objects than the annotation")
        r = jf_radius(tuple(gt.shape[-2:]))
        JF = []
        for o in range(gt.shape[0]):
            g = _binary_u8(gt[o])
            s = _binary_u8(res[o]) if o < res.shape[0] else g.new_zeros(g.shape)        # (a missing object: an empty mask)
            J, F = jf_from_counts(jf_counts_hip(g, s, 1, r))
            JF.append((J[:, 0], F[:, 0]))
        return _jfm(lambda o: JF[o][0], lambda o: JF[o][1], len(JF))
    gt, res = np.asarray(all_gt_masks), np.asarray(all_res_masks)
    if res.shape[0] > gt.shape[0]:
        raise ValueError("JFM: the result has more objects than the annotation")
    if res.shape[0] < gt.shape[0]:
        res = np.concatenate([res, np.zeros((gt.shape[0] - res.shape[0], *res.shape[1:]), res.dtype)], 0)
    out = {k: [] for k in ("JM", "JR", "JD", "FM", "FR", "FD")}
    for o in range(gt.shape[0]):
        j = np.asarray(db_eval_iou(gt[o], res[o]), dtype=np.float64)
        f = db_eval_boundary(gt[o], res[o])
        for key, vals in (("J", j), ("F", f)):
            m, r, d = db_statistics(vals)
            out[key + "M"].append(m)
            out[key + "R"].append(r)
            out[key + "D"].append(d)
    return out


def davis_masks_to_objects(masks: np.ndarray, n_objects: int) -> np.ndarray:
    """(T, h, w) index masks -> (n_objects, T, h, w) binary masks of ids 1..n_objects."""
    m = np.asarray(masks)
    return np.stack([m == k for k in range(1, n_objects + 1)], 0) if n_objects else np.zeros((0, *m.shape), bool)


def davis_jf(sequences: Dict[str, tuple], backend: str = "host") -> Dict[str, object]:
    """sequences: name -> (gt (T, h, w) ids, prediction (T, h, w) ids).  Frame 0 (the given annotation) and the last frame are left
    out of the statistics as the DAVIS-2017 semi-supervised evaluation does.  Returns the J&F mean, J mean, F mean and per-sequence
    J&F / J / F means (each a mean over the sequence's objects).  backend='hip': one fgvc_jf_counts_u8 call per sequence on the id maps
    themselves (uint8 CUDA tensors are read in place, anything else is rounded and uploaded); the frame rule and the statistics stay on
    the host, and the result is the same."""
    hip = _backend(backend)
    per_seq, Js, Fs = {}, [], []
    for name, (gt, pred) in sequences.items():
        if not hip:
            gt, pred = np.asarray(gt), np.asarray(pred)
        sl = slice(1, -1) if gt.shape[0] > 2 else slice(0, gt.shape[0])
        if hip:
            n = int(gt.max())
            J, F = jf_from_counts(jf_counts_hip(gt[sl], pred[sl], n, jf_radius(tuple(gt.shape[-2:]))))
            r = _jfm(lambda o: J[:, o], lambda o: F[:, o], n)
        else:
            n = int(gt.max())
            r = JFM(davis_masks_to_objects(gt, n)[:, sl], davis_masks_to_objects(np.rint(pred).astype(np.int64), n)[:, sl], n)
        Js.extend(r["JM"])
        Fs.extend(r["FM"])
        jm, fm = float(np.mean(r["JM"])), float(np.mean(r["FM"]))
        per_seq[name] = {"J&F": (jm + fm) / 2, "J": jm, "F": fm}
    jm, fm = float(np.mean(Js)), float(np.mean(Fs))
    return {"J&F-Mean": (jm + fm) / 2, "J-Mean": jm, "F-Mean": fm, "sequences": per_seq}


def flow_epe(pred, gt, valid=None) -> dict:
    """End-point error of a dense flow: pred, gt (..., 2, h, w) torch tensors (channel 0 = x) on one device, either one; valid (..., h, w)
    or (..., 1, h, w), non-zero = scored (None: every pixel).  Returns {'epe': the mean error in pixels, '1px' / '3px' / '5px': the share
    of scored pixels whose error is below 1, 3 and 5 px, 'n': how many were scored}; with no scored pixel the four figures are NaN."""
    import torch
    if pred.shape != gt.shape or pred.dim() < 3 or pred.shape[-3] != 2:
        raise ValueError(f"flow_epe: two flows of one shape (..., 2, h, w), got {tuple(pred.shape)} and {tuple(gt.shape)}")
    err = (pred.to(torch.float64) - gt.to(torch.float64)).pow(2).sum(-3).sqrt()                      # (..., h, w)
    if valid is None:
        keep = torch.ones_like(err, dtype=torch.bool)
    else:
        keep = valid != 0
        if keep.dim() == err.dim() + 1 and keep.shape[-3] == 1:
            keep = keep.squeeze(-3)
        if keep.shape != err.shape:
            raise ValueError(f"flow_epe: valid of shape {tuple(valid.shape)} for flows of shape {tuple(pred.shape)}")
    e = err[keep.to(err.device)]
    n = int(e.numel())
    if n == 0:
        return {"epe": float("nan"), "1px": float("nan"), "3px": float("nan"), "5px": float("nan"), "n": 0}
    return {"epe": float(e.mean()), "1px": float((e < 1).double().mean()), "3px": float((e < 3).double().mean()),
            "5px": float((e < 5).double().mean()), "n": n}


# ---- objects as boxes ---------------------------------------------------------------------------------------------

def object_stats_host(ids, n_ids: int) -> np.ndarray:
    """The contract of ops.object_stats (fgvc_seg_object_stats_u8), in plain numpy: ids (T, h, w) integers -> (T, n_ids, 8) int64.  For
    frame t and id o = 0 .. n_ids - 1 (the background has its row), over the pixels (y, x) with ids[t, y, x] == o:
        0 area   1 x0 = min x   2 y0 = min y   3 x1 = max x + 1   4 y1 = max y + 1   5 sum of x   6 sum of y
        7 border = how many of them have x == 0, x == w - 1, y == 0 or y == h - 1
    An id without a pixel on a frame: eight zeros.  Ids of n_ids or more are counted nowhere."""
    ids = np.asarray(ids)
    if ids.ndim != 3:
        raise ValueError(f"ids: 3 dimensions (T, h, w), got {ids.shape}")
    if ids.dtype.kind not in "iu":                           # (the mask call's float64 arrays hold small integers)
        ids = np.rint(ids).astype(np.int64)
    n_ids = int(n_ids)
    if not 1 <= n_ids <= 256:
        raise ValueError(f"n_ids={n_ids}: 1 .. 256")
    T, h, w = ids.shape
    out = np.zeros((T, n_ids, 8), np.int64)
    for t in range(T):
        present = np.unique(ids[t])
        for o in present[(present >= 0) & (present < n_ids)].tolist():
            ys, xs = np.nonzero(ids[t] == o)
            ys, xs = ys.astype(np.int64), xs.astype(np.int64)
            edge = (xs == 0) | (xs == w - 1) | (ys == 0) | (ys == h - 1)
            out[t, o] = (xs.size, xs.min(), ys.min(), xs.max() + 1, ys.max() + 1, xs.sum(), ys.sum(), np.count_nonzero(edge))
    return out


def box_iou(a, b) -> np.ndarray:
    """Intersection over union of half-open integer boxes (..., 4) = (x0, y0, x1, y1), broadcast against each other -> float64.  A box with
    x1 <= x0 or y1 <= y0 is empty: against a non-empty box the value is 0, and two empty boxes give NaN (no union to divide by)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape[-1] != 4 or b.shape[-1] != 4:
        raise ValueError(f"boxes: (..., 4) as (x0, y0, x1, y1), got {a.shape} and {b.shape}")

    def area(x0, y0, x1, y1):
        return np.maximum(x1 - x0, 0.0) * np.maximum(y1 - y0, 0.0)
    area_a, area_b = area(*np.moveaxis(a, -1, 0)), area(*np.moveaxis(b, -1, 0))
    inter = area(np.maximum(a[..., 0], b[..., 0]), np.maximum(a[..., 1], b[..., 1]), np.minimum(a[..., 2], b[..., 2]),
                 np.minimum(a[..., 3], b[..., 3]))
    inter = np.where((area_a > 0) & (area_b > 0), inter, 0.0)
    union = area_a + area_b - inter
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(union > 0, inter / union, np.nan)


def mean_box_iou(gt_ids, pred_ids, n_ids: int, backend: str = "host") -> float:
    """The mean box_iou of the objects' boxes in two (T, h, w) id maps, over the objects 1 .. n_ids - 1 and the frames 1 .. T - 1 (frame 0 is
    the given annotation) on which at least one of the two maps has the object; NaN when there is no such pair.  backend='host': both
    sets of boxes from object_stats_host; 'hip': from one ops.object_stats call each (fgvc_seg_object_stats_u8), the same integers."""
    if _backend(backend):
        from . import ops
        sg = ops.object_stats(_device_ids(gt_ids, n_ids - 1), n_ids).cpu().numpy()
        sp = ops.object_stats(_device_ids(pred_ids, n_ids - 1), n_ids).cpu().numpy()
    else:
        def host(x):
            return np.asarray(x.detach().cpu() if hasattr(x, "detach") else x)
        sg, sp = object_stats_host(host(gt_ids), n_ids), object_stats_host(host(pred_ids), n_ids)
    iou = box_iou(sg[1:, 1:, 1:5], sp[1:, 1:, 1:5])
    return float(np.nanmean(iou)) if np.isfinite(iou).any() else float("nan")


# ---- connected components of id maps: the rule of ops.seg_components / ops.seg_clean ----------------------------

def _ids_3d(ids, what="ids") -> np.ndarray:
    ids = np.asarray(ids)
    if ids.ndim != 3:
        raise ValueError(f"{what}: 3 dimensions (T, h, w), got {ids.shape}")
    if ids.dtype.kind not in "iub":                          # (the mask call's float64 arrays hold small integers)
        ids = np.rint(ids)
    return ids.astype(np.int64)


def components_host(ids, connectivity: int = 8, background: bool = False) -> np.ndarray:
    """The contract of ops.seg_components (fgvc_seg_components_i32), in plain Python: ids (T, h, w) integers -> (T, h, w) int32.  Two
    pixels of a frame belong together when they carry the same id and are neighbours: 4- or 8-neighbours (`connectivity`) for a non-zero
    id, ALWAYS 4-neighbours for id 0.  A component is a maximal such set, and a pixel's label is the smallest linear index y * w + x of
    its component (its root).  With background=False the pixels of id 0 get -1.  Frames are independent."""
    ids = _ids_3d(ids)
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity={connectivity}: 4 or 8")
    T, h, w = ids.shape
    out = np.full((T, h, w), -1, np.int32)
    for t in range(T):
        m = ids[t].tolist()
        parent = list(range(h * w))

        def find(a):
            while parent[a] != a:
                parent[a] = parent[parent[a]]
                a = parent[a]
            return a

        def union(a, b):
            a, b = find(a), find(b)
            if a != b:                                       # the smaller index stays the root: a root is its component's minimum
                parent[max(a, b)] = min(a, b)

        for y in range(h):
            row, up = m[y], m[y - 1] if y else None
            for x in range(w):
                v, p = row[x], y * w + x
                if x and row[x - 1] == v:
                    union(p, p - 1)
                if y and up[x] == v:
                    union(p, p - w)
                if y and v != 0 and connectivity == 8:
                    if x and up[x - 1] == v:
                        union(p, p - w - 1)
                    if x + 1 < w and up[x + 1] == v:
                        union(p, p - w + 1)
        lab = np.array([find(p) for p in range(h * w)], np.int32).reshape(h, w)
        out[t] = lab if background else np.where(ids[t] != 0, lab, -1)
    return out


def clean_masks_host(ids, n_ids: int, connectivity: int = 8, min_area: int = 0, keep: str = "all", fill_holes: bool = False,
                     max_hole_area=None, frames=None):
    """The contract of ops.seg_clean (fgvc_seg_clean_u8): ids (T, h, w) integers 0 .. 255 -> (out (T, h, w) uint8, stats (T, n_ids, 4)
    int64), out = fill(drop(ids)) per frame, over the components of components_host.
      drop: a component of an id 1 .. n_ids - 1 becomes 0 when its area is below min_area, and with keep='largest' also when it is not
            the largest component of its id on the frame (equal areas: the smaller root wins).  Pixels of an id >= n_ids are copied; they
            take part in nothing and cannot bound a hole.
      fill (fill_holes, on the map AFTER the drop): a 4-connected component of id 0 becomes id o when it has no pixel on the frame's
            outermost rows and columns, all its 4-neighbours that are not background carry the one id o < n_ids, and its area is at most
            max_hole_area (None: any area).
    frames: (T,) bools; a frame whose entry is false is copied and its stats are zero.  stats[t, o] = components of id o before the drop,
    components kept, pixels dropped, pixels filled with o; row 0 is four zeros."""
    ids = _ids_3d(ids)
    n_ids = int(n_ids)
    if not 1 <= n_ids <= 256:
        raise ValueError(f"n_ids={n_ids}: 1 .. 256")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity={connectivity}: 4 or 8")
    if keep not in ("all", "largest"):
        raise ValueError(f"keep={keep!r}: 'all' or 'largest'")
    if ids.size and (ids.min() < 0 or ids.max() > 255):
        raise ValueError("ids: values 0 .. 255")
    T, h, w = ids.shape
    on = np.ones(T, bool) if frames is None else np.asarray(frames).astype(bool)
    if on.shape != (T,):
        raise ValueError(f"frames: shape ({T},), got {on.shape}")
    out = ids.astype(np.uint8)
    stats = np.zeros((T, n_ids, 4), np.int64)
    for t in np.nonzero(on)[0].tolist():
        if h == 0 or w == 0:
            continue
        m = out[t]
        part = (m > 0) & (m < n_ids)
        lab = components_host(np.where(part, m, 0)[None], connectivity)[0]
        roots, area = np.unique(lab[part], return_counts=True)           # ascending roots
        root_id = m.reshape(-1)[roots]
        dropped = []
        for o in np.unique(root_id).tolist():
            sel = np.nonzero(root_id == o)[0]
            kept = area[sel] >= min_area
            if keep == "largest":
                kept &= np.arange(sel.size) == int(np.argmax(area[sel]))   # the first maximum: the smallest root
            stats[t, o, 0], stats[t, o, 1], stats[t, o, 2] = sel.size, int(kept.sum()), int(area[sel][~kept].sum())
            dropped.extend(roots[sel][~kept].tolist())
        m[np.isin(lab, np.array(dropped, np.int32)) & part] = 0
        if not fill_holes:
            continue
        bg = m == 0
        lab = components_host((~bg)[None], 4, background=True)[0]          # id 0: 4-neighbours
        n = h * w
        edge = np.zeros((h, w), bool)
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = True
        open_ = np.zeros(n, bool)
        open_[lab[bg & edge]] = True
        lo, hi = np.full(n, 256, np.int64), np.full(n, -1, np.int64)
        for a, b in (((slice(1, None), slice(None)), (slice(None, -1), slice(None))), ((slice(None, -1), slice(None)), (slice(1, None), slice(None))),
                     ((slice(None), slice(1, None)), (slice(None), slice(None, -1))), ((slice(None), slice(None, -1)), (slice(None), slice(1, None)))):
            pair = bg[a] & ~bg[b]                                          # a background pixel and its neighbour that is not
            np.minimum.at(lo, lab[a][pair], m[b][pair].astype(np.int64))
            np.maximum.at(hi, lab[a][pair], m[b][pair].astype(np.int64))
        broots, barea = np.unique(lab[bg], return_counts=True)
        for r, a in zip(broots.tolist(), barea.tolist()):
            o = int(lo[r])
            if open_[r] or lo[r] != hi[r] or o >= n_ids or (max_hole_area is not None and a > max_hole_area):
                continue
            m[(lab == r) & bg] = o
            stats[t, o, 3] += a
    return out, stats


# ---- object crops: the window rule ------------------------------------------------------------------------------

WINDOW_MAX_SIDE = 32768        # mask and frame sides above it are refused
WINDOW_MAX_SIZE = 1024         # output sides S_h, S_w: 1 .. 1024
WINDOW_MAX_PAD = 4.0
WINDOW_PAD_ONE = 1024          # pad crosses the C ABI as pad_q = int(round(pad * 1024))


def window_args(n_ids: int, size, pad, min_side, smooth, mask_size, frame_size, objects):
    """The host half of the window rule, shared by object_windows_host and ops.object_windows: checks every argument by name and returns
    (objects list, S_h, S_w, pad_q, min_side, smooth, h, w, H, W) as Python ints."""
    try:
        S_h, S_w = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError(f"size={size!r}: (S_h, S_w)") from None
    if not (1 <= S_h <= WINDOW_MAX_SIZE and 1 <= S_w <= WINDOW_MAX_SIZE):
        raise ValueError(f"size={tuple(size)}: S_h and S_w in 1 .. {WINDOW_MAX_SIZE}")
    pad = float(pad)
    if not 0.0 <= pad <= WINDOW_MAX_PAD:                        # (NaN fails both comparisons)
        raise ValueError(f"pad={pad}: 0 .. {WINDOW_MAX_PAD:g}")
    pad_q = int(round(pad * WINDOW_PAD_ONE))
    min_side, smooth = int(min_side), int(smooth)
    if not 1 <= min_side <= WINDOW_MAX_SIDE:
        raise ValueError(f"min_side={min_side}: 1 .. {WINDOW_MAX_SIDE}")
    if not 0 <= smooth < 1 << 20:
        raise ValueError(f"smooth={smooth}: 0 .. 2^20 - 1 frames on each side")
    if mask_size is None:
        raise ValueError("mask_size: (h, w) of the id map the statistics were taken from")
    h, w = (int(s) for s in mask_size)
    H, W = (h, w) if frame_size is None else (int(s) for s in frame_size)
    for name, v in (("mask_size h", h), ("mask_size w", w), ("frame_size H", H), ("frame_size W", W)):
        if not 1 <= v <= WINDOW_MAX_SIDE:
            raise ValueError(f"{name}={v}: 1 .. {WINDOW_MAX_SIDE}")
    objects = list(range(1, n_ids)) if objects is None else [int(o) for o in objects]
    for o in objects:
        if not 0 <= o < n_ids:
            raise ValueError(f"objects: id {o} outside 0 .. {n_ids - 1} (the statistics have {n_ids} rows)")
    return objects, S_h, S_w, pad_q, min_side, smooth, h, w, H, W


def _cdiv(a: int, b: int) -> int:
    """ceiling division, right for negative numerators too (b > 0)"""
    return -((-a) // b)


def object_windows_host(stats, size, pad: float = 0.125, min_side: int = 8, smooth: int = 0, mask_size=None, frame_size=None,
                        objects=None) -> np.ndarray:
    """The contract of ops.object_windows (fgvc_seg_object_windows_i64), in Python integers: stats (T, N, 8) int64 as object_stats_host
    gives them -> windows (T, M, 8) int64 for the M ids of `objects` (default 1 .. N - 1).  size = (S_h, S_w) the crop's size, pad 0 .. 4
    as pad_q = int(round(pad * 1024)), min_side >= 1, smooth = r >= 0 frames on each side, mask_size = (h, w) of the id map, frame_size
    = (H, W) of the frames the crops are taken from (None: mask_size).  // is floor division and cdiv ceiling division.  For frame t, id o:
        U = {u : |u - t| <= r, 0 <= u < T, area[u, o] > 0};  area[t, o] == 0: eight zeros (no window).  Otherwise n = |U|,
        Wm = max_U (x1 - x0), Hm = max_U (y1 - y0)                              (the maximum: smoothing never clips the object)
        Wp = max(min_side, Wm + 2 cdiv(Wm pad_q, 1024)), Hp likewise
        Wp S_h < Hp S_w: Wp = cdiv(Hp S_w, S_h), else Hp = cdiv(Wp S_h, S_w)    (the output's aspect, by growing one side)
        wx0 = (sum_U (x0 + x1) - n Wp) // (2 n), wx1 = wx0 + Wp, y likewise     (never clamped: the window may leave the frame)
    words 0 .. 3: (wx0, wy0, wx1, wy1) in mask pixels; words 4 .. 7: (wx0 W // w, wy0 H // h, cdiv(wx1 W, w), cdiv(wy1 H, h)) in frame
    pixels -- the same four with frame_size == mask_size."""
    s = np.asarray(stats)
    if s.ndim != 3 or s.shape[2] != 8 or s.dtype != np.int64:
        raise ValueError(f"stats: (T, N, 8) int64, got {s.dtype} {s.shape}")
    T, N = s.shape[:2]
    objects, S_h, S_w, pad_q, min_side, r, h, w, H, W = window_args(N, size, pad, min_side, smooth, mask_size, frame_size, objects)
    out = np.zeros((T, len(objects), 8), np.int64)
    for j, o in enumerate(objects):
        rows = s[:, o].tolist()
        for t in range(T):
            if rows[t][0] <= 0:
                continue
            U = [rows[u] for u in range(max(0, t - r), min(T, t + r + 1)) if rows[u][0] > 0]
            n = len(U)
            Wm, Hm = max(u[3] - u[1] for u in U), max(u[4] - u[2] for u in U)
            Wp = max(min_side, Wm + 2 * _cdiv(Wm * pad_q, WINDOW_PAD_ONE))
            Hp = max(min_side, Hm + 2 * _cdiv(Hm * pad_q, WINDOW_PAD_ONE))
            if Wp * S_h < Hp * S_w:
                Wp = _cdiv(Hp * S_w, S_h)
            else:
                Hp = _cdiv(Wp * S_h, S_w)
            wx0 = (sum(u[1] + u[3] for u in U) - n * Wp) // (2 * n)
            wy0 = (sum(u[2] + u[4] for u in U) - n * Hp) // (2 * n)
            wx1, wy1 = wx0 + Wp, wy0 + Hp
            out[t, j] = (wx0, wy0, wx1, wy1, wx0 * W // w, wy0 * H // h, _cdiv(wx1 * W, w), _cdiv(wy1 * H, h))
    return out
