#!/usr/bin/env python3
"""Evaluation entry point with the steps of the reference's tools/test.py:71-198, on fgvc_amd.

    python tools/test.py CONFIG --task davis [--checkpoint CKPT] [--videos 4 --frames 8 --size 256 256]
    python tools/test.py CONFIG --task vos --data-root DAVIS_2017_DIR     # masks: J&F (test_cfg_vos, else test_cfg_davis's keys)
    python tools/test.py CONFIG --task ytvos --data-root YOUTUBE_VOS_DIR [--out-dir DIR]   # masks from the frames where objects first appear
    python tools/test.py CONFIG --task vos --data-root DIR --eval-arc HRVanillaTracker    # the config's eval_arc overridden
    python tools/test.py CONFIG --task davis --occlusion [--cycle-thresh 1.0] [--occluder]   # predicted visibility: DESIGN.md section 13
    python tools/test.py CONFIG --task davis --chain [--chain-visibility frame|consistency] [--query-mode strided]   # flow chaining: section 18
    python tools/test.py CONFIG --task davis|vos|jhmdb|badja --raw-frames     # uint8 RGB frames into the model (test_cfg.input): section 14
    python tools/test.py CONFIG --task vos --data-root DIR --gpu-metrics     # masks stay on the device, J&F from fgvc_jf_counts_u8: section 15
    python tools/test.py CONFIG --task vos --data-root DIR --boxes           # also the mean box IoU per sequence against the annotation's boxes: section 27
    python tools/test.py CONFIG --task vos --data-root DIR --clean --keep-largest --fill-holes [--min-area N] [--max-hole N]   # test_cfg.clean: section 28
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 tools/test.py CONFIG --launcher pytorch

CONFIG may be the reference's own configs/eval/res18_d1_eval.py.  The TAP-Vid / JHMDB files are not available
offline, so the default dataset is `SyntheticTapVid` (same sample format); `--data-root DIR_OR_PKL` reads TAP-Vid
pickles (`fgvc_amd.datasets.TapVidPickles`: a directory of per-video pickles as the reference globs them, or the
published tapvid_davis.pkl).
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import apis, metrics, viz  # noqa: E402
from fgvc_amd.datasets import Davis2017, YoutubeVos, davis_evaluate, ytvos_run  # noqa: E402
from fgvc_amd.datasets import BadjaPoses, JhmdbPoses, StridedLoader, SyntheticTapVid, TapVidPickles, badja_evaluate, jhmdb_evaluate  # noqa: E402
from fgvc_amd.datasets import MapsAsCoords, badja_evaluate_heatmap, jhmdb_evaluate_heatmap  # noqa: E402

POSE_SIZE = dict(jhmdb=(320, 320), badja=(320, 512))          # the network size of the pose tasks (test_pipeline_jhmdb, badja_dataset.py:355-362)

DEFAULT_CFG = dict(
    model=dict(type="VanillaTracker",
               backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
    test_cfg_davis=dict(precede_frames=5, topk=10, temperature=0.07, strides=(1, 1, 1, 4), out_indices=(2,),
                        neighbor_range=30, step=512, with_first=True, with_first_neighbor=True),
)


def jhmdb_frames(ds, i):
    """The frames the JHMDB heat-map form's coordinates refer to: the video's own."""
    import numpy as np
    from PIL import Image
    return np.stack([np.asarray(Image.open(p).convert("RGB")) for p in ds.samples[i]["frames_path"]])


def badja_frames(ds, i):
    """The frames the BADJA heat-map form's coordinates refer to: the video's, resized to the network size."""
    import numpy as np
    from PIL import Image
    v = ds.videos[i]
    n = len(v["frames"]) if ds.length == -1 else min(ds.length, len(v["frames"]))
    h, w = ds.size
    return np.stack([np.asarray(Image.open(p).convert("RGB").resize((w, h), Image.BILINEAR)) for p in v["frames"][:n]])


class PosePainter:
    """--render: a coords=True tracker that also paints the clip it is called on -- viz.paint_pose on the device with the joints'
    coordinates, their visibility by viz.pose_visibles (with --min-conf: from the peaks of test_cfg.pose) and the skeleton -- into
    DIR/<video>/frame_%05d.png.  Which clip that is comes from the dataset: indexed(ds) notes the index of every item it hands out."""

    def __init__(self, model, out_dir, names, clip, skeleton, min_conf):
        self.model, self.out_dir, self.names, self.clip, self.skeleton, self.min_conf = model, out_dir, names, clip, skeleton, min_conf
        self.index = None

    def indexed(self, ds):
        painter = self

        class Indexed:
            def __len__(self):
                return len(ds)

            def __getitem__(self, i):
                painter.index = i
                return ds[i]

            def __getattr__(self, name):
                return getattr(ds, name)
        return Indexed()

    def __call__(self, **data):
        from PIL import Image
        out = self.model(**data)
        coords, i = out[0], self.index
        peak = self.model.last_pose["peak"] if self.min_conf is not None else None
        frames = self.clip(i)[:coords.shape[2]]
        painted = viz.paint_pose(frames, viz.pose_tracks(coords), viz.pose_visibles(coords, peak, self.min_conf), skeleton=self.skeleton,
                                 backend="hip")
        d = os.path.join(self.out_dir, self.names(i))
        os.makedirs(d, exist_ok=True)
        for t, f in enumerate(painted):
            Image.fromarray(f).save(os.path.join(d, f"frame_{t:05d}.png"))
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default=None)
    ap.add_argument("--task", default="davis")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--launcher", choices=["none", "pytorch"], default="none")
    ap.add_argument("--videos", type=int, default=4)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--query-mode", default="first")
    ap.add_argument("--data-root", default=None, help="TAP-Vid pickles (directory of *.pkl or one .pkl); default: synthetic clips")
    ap.add_argument("--pose-form", choices=["points", "heatmap", "softmap"], default="points",
                    help="jhmdb / badja: 'points' tracks the frame-0 joints as query points; 'heatmap' propagates the reference's first-frame "
                         "Gaussian maps and reads joints out of them (test_cfg.coords=True); 'softmap' has the propagated maps themselves "
                         "returned (test_cfg.return_maps=True) and reads the joints out of them on the host, by the same rule")
    ap.add_argument("--dump-maps", default=None, metavar="DIR", help="--pose-form softmap: write each video's (T, K, h0, w0) array as DIR/<video>.npy")
    ap.add_argument("--render", default=None, metavar="DIR", help="--task jhmdb|badja --pose-form heatmap: paint every clip (JHMDB with its "
                                                                  "skeleton, BADJA the joints alone) into DIR/<video>/frame_%05d.png")
    ap.add_argument("--min-conf", type=float, default=None, metavar="X", help="with --render: hide a joint whose map's peak is below X "
                                                                              "(test_cfg.pose; the scores do not change)")
    ap.add_argument("--eval-arc", default=None, help="tracker class to build, overriding the config's eval_arc (e.g. HRVanillaTracker: the "
                                                     "local-window affinity for masks, heat maps and points)")
    ap.add_argument("--occlusion", action="store_true",
                    help="predict visibility by the forward-backward cycle check (test_cfg.occlusion = dict(type='cycle', ...)): "
                         "average_jaccard and occlusion_accuracy then score a prediction instead of all-occluded zeros")
    ap.add_argument("--cycle-thresh", type=float, default=None, metavar="CELLS",
                    help="with --occlusion: a point is visible while its cycle error is <= this many feature cells (default 1.0)")
    ap.add_argument("--chain", action="store_true",
                    help="track by chaining the dense flow, forward and backward in time (test_cfg.chain = dict(type='flow', ...), DESIGN.md "
                         "section 18): the frames before a query time, which --query-mode strided scores, are tracked too")
    ap.add_argument("--chain-visibility", choices=("frame", "consistency"), default=None,
                    help="with --chain: 'frame' (default, the reference's rule: visible while inside the frame) or 'consistency'")
    ap.add_argument("--occluder", action="store_true", help="synthetic clips: paste a static rectangle over the later frames (SyntheticTapVid(occluder=True))")
    ap.add_argument("--raw-frames", action="store_true",
                    help="hand the decoded uint8 frames to the model (datasets' raw=True) and set test_cfg.input = dict(type='rgb8', size=...): "
                         "resize, RGB -> Lab and normalisation run in the library's input kernel instead of the datasets' torch chain")
    ap.add_argument("--boxes", action="store_true",
                    help="--task vos: also print the mean box IoU per sequence of the predicted objects' boxes against the boxes of the "
                         "ground-truth maps (metrics.mean_box_iou): both from ops.object_stats under --gpu-metrics, from the host contract "
                         "otherwise")
    ap.add_argument("--gpu-metrics", action="store_true",
                    help="--task vos: keep the propagated masks on the device (test_cfg.masks='device') and score J&F from the counts of "
                         "the library's fgvc_jf_counts_u8 (metrics.davis_jf(backend='hip')): the same numbers, DESIGN.md section 15")
    ap.add_argument("--readout", choices=["bilinear", "guided"], default=None,
                    help="--task vos: the mask read-out (test_cfg.readout = dict(type=...)); 'guided' is the edge-aware one, whose effect on "
                         "real DAVIS J&F is unmeasured")
    ap.add_argument("--clean", action="store_true",
                    help="--task vos: clean the propagated masks on the device before they are scored (test_cfg.clean = dict(...), "
                         "ops.seg_clean; DESIGN.md section 28); its effect on real DAVIS J&F is unmeasured")
    ap.add_argument("--min-area", type=int, default=0, metavar="N", help="with --clean: drop connected parts of an object below N pixels")
    ap.add_argument("--keep-largest", action="store_true", help="with --clean: keep only the largest connected part of every object")
    ap.add_argument("--fill-holes", action="store_true", help="with --clean: fill background enclosed by one object")
    ap.add_argument("--max-hole", type=int, default=None, metavar="N", help="with --fill-holes: only holes of at most N pixels")
    ap.add_argument("--out", default=None)
    ap.add_argument("--out-dir", default=None, help="write summaries<task>.json / results_df<task>.csv / results_list<task>.pkl there "
                                                    "(the files of the reference's save_results, tapvid.py:316-350)")
    a = ap.parse_args()

    cfg = api.Config.fromfile(a.config) if a.config else api.Config(DEFAULT_CFG)           # tools/test.py:75
    distributed = a.launcher != "none"
    rank, world = 0, 1
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if distributed:                                                                          # :106-110
        dist.init_process_group("nccl", device_id=dev)
        rank, world = dist.get_rank(), dist.get_world_size()

    if a.task == "vos":
        if not a.data_root:
            raise SystemExit("--task vos needs --data-root (DAVIS-2017 layout: ImageSets/2017/val.txt, JPEGImages/480p, Annotations/480p)")
        dataset = None
    elif a.task == "ytvos":
        if not a.data_root:
            raise SystemExit("--task ytvos needs --data-root (YouTube-VOS layout: JPEGImages/<video>, Annotations/<video>, meta.json)")
        dataset = None
    elif a.task in ("jhmdb", "badja"):
        if not a.data_root:
            raise SystemExit("--task jhmdb needs --data-root (JHMDB frames + joint_positions + val_list.txt); --task badja the BADJA root "
                             "(joint_annotations/*.json, JPEGImages/, Annotations/)")
        dataset = None
    elif a.data_root:
        dataset = TapVidPickles(a.data_root, a.query_mode, tuple(a.size), device=dev, raw=a.raw_frames)   # :121-122
    else:
        dataset = SyntheticTapVid(a.videos, a.frames, tuple(a.size), a.points, a.query_mode, device=dev, occluder=a.occluder, raw=a.raw_frames)
    loader = StridedLoader(dataset, rank, world) if dataset is not None else None          # :124-134
    key = "test_cfg_" + a.task                                                               # :135
    if key not in cfg and a.task in ("jhmdb", "badja", "vos", "ytvos") and "test_cfg_davis" in cfg:
        key = "test_cfg_davis"         # the pose task of DEFAULT_CFG (and of configs without a test_cfg_jhmdb) tracks with the TAP-Vid settings
    if a.task == "ytvos" and key not in cfg and "test_cfg_vos" in cfg:
        key = "test_cfg_vos"
    if key not in cfg:
        raise SystemExit(f"the config has no '{key}' (tasks it defines: {sorted(k[9:] for k in cfg if k.startswith('test_cfg_'))})")
    test_cfg = cfg[key]
    if a.task == "ytvos" and test_cfg.get("refs", None) is None:
        test_cfg = dict(test_cfg, refs=dict(direction="forward", override="new"))    # objects are annotated where they first appear
    heatmap = a.task in ("jhmdb", "badja") and a.pose_form in ("heatmap", "softmap")
    softmap = heatmap and a.pose_form == "softmap"
    if a.dump_maps and not softmap:
        raise SystemExit("--dump-maps goes with --task jhmdb|badja --pose-form softmap")
    if a.render and not (heatmap and not softmap):
        raise SystemExit("--render goes with --task jhmdb|badja --pose-form heatmap")
    if a.min_conf is not None and not a.render:
        raise SystemExit("--min-conf goes with --render")
    if a.min_conf is not None:
        test_cfg = dict(test_cfg, pose=dict(confidence=True, keep_field=False))     # the peaks, for the painter alone
    if softmap:
        test_cfg = dict(test_cfg, return_maps=True)  # the maps themselves (the reference's coords=False return value), decoded below
    elif heatmap:
        test_cfg = dict(test_cfg, coords=True)       # the reference's pose configs: 4-D first-frame maps read out by img2coord
    if a.cycle_thresh is not None and not a.occlusion:
        raise SystemExit("--cycle-thresh goes with --occlusion")
    if a.occlusion:
        if dataset is None:
            raise SystemExit("--occlusion is a read-out of the points call: TAP-Vid tasks only (not vos / jhmdb / badja)")
        if distributed:
            raise SystemExit("--occlusion runs on one GPU (--launcher none)")
        test_cfg = dict(test_cfg, occlusion=dict(type="cycle", cycle_thresh=1.0 if a.cycle_thresh is None else a.cycle_thresh, radius=None))
    if a.chain_visibility is not None and not a.chain:
        raise SystemExit("--chain-visibility goes with --chain")
    if a.chain:
        if dataset is None:
            raise SystemExit("--chain is a form of the points call: TAP-Vid tasks only (not vos / jhmdb / badja)")
        if distributed:
            raise SystemExit("--chain runs on one GPU (--launcher none)")
        if a.occlusion:
            raise SystemExit("--chain has its own visibility (--chain-visibility); --occlusion belongs to label propagation")
        test_cfg = dict(test_cfg, chain=dict(type="flow", visibility=a.chain_visibility or "frame"))
    if a.raw_frames:
        if distributed:
            raise SystemExit("--raw-frames runs on one GPU (--launcher none)")
        net_size = {"vos": None, "ytvos": None, **POSE_SIZE}.get(a.task, tuple(a.size))                                  # what each dataset resizes to
        test_cfg = dict(test_cfg, input=dict(type="rgb8", size=net_size, layout="thwc"))
    if a.boxes and a.task != "vos":
        raise SystemExit("--boxes goes with --task vos (the boxes of the mask path's objects)")
    if a.gpu_metrics:
        if a.task != "vos":
            raise SystemExit("--gpu-metrics goes with --task vos (the J&F of the mask path)")
        test_cfg = dict(test_cfg, masks="device")
    if a.clean or a.min_area or a.keep_largest or a.fill_holes or a.max_hole is not None:
        if not a.clean or a.task not in ("vos", "ytvos"):
            raise SystemExit("--clean goes with --task vos (the index maps of the mask path); --min-area, --keep-largest, --fill-holes and "
                             "--max-hole go with --clean")
        if distributed:
            raise SystemExit("--clean runs on one GPU (--launcher none); the multi-GPU path is not covered")
        test_cfg = dict(test_cfg, clean=dict(min_area=a.min_area, keep="largest" if a.keep_largest else "all", fill_holes=a.fill_holes,
                                             max_hole_area=a.max_hole))
    if a.readout is not None:
        if a.task not in ("vos", "ytvos"):
            raise SystemExit("--readout goes with --task vos (the index-map read-out of the mask path)")
        if distributed:
            raise SystemExit("--readout runs on one GPU (--launcher none); the multi-GPU path is not covered")
        test_cfg = dict(test_cfg, readout=dict(type=a.readout))      # 'guided': DESIGN.md section 24, its default radius and sigmas (untuned)
    model_cfg = dict(type=a.eval_arc or cfg.get("eval_arc", "VanillaTracker"), backbone=dict(cfg.model.backbone))   # :139
    for k in ("out_indices", "strides", "dilations"):                                        # :141-145
        if k in test_cfg:
            model_cfg["backbone"][k] = test_cfg[k]
    model = api.build_model(model_cfg, train_cfg=None, test_cfg=test_cfg)                    # :152
    model.init_weights()                                                                     # :153
    if a.checkpoint:
        api.load_checkpoint(model, a.checkpoint)                                             # :158-159
    model = model.to(dev).eval()

    def scored(names, clip=None):
        """The model the heat-map evaluators call: itself, or under --pose-form softmap its maps decoded on the host (and dumped), or
        under --render itself with every clip painted on the way (clip(i) -> the frames (T, h, w, 3) uint8 the coordinates refer to)."""
        if a.render:
            return PosePainter(model, a.render, names, clip, viz.JHMDB_SKELETON if a.task == "jhmdb" else None, a.min_conf)
        if not softmap:
            return model
        if a.dump_maps:
            os.makedirs(a.dump_maps, exist_ok=True)
        import numpy as np
        dump = (lambda i, maps: np.save(os.path.join(a.dump_maps, names(i) + ".npy"), maps)) if a.dump_maps else None
        return MapsAsCoords(model, dump)

    if a.task == "vos":        # semi-supervised VOS: the first annotation is propagated (VanillaTracker.forward_test_seg), scored by J&F
        if rank == 0:
            jf = davis_evaluate(model, Davis2017(a.data_root, split="val", device=dev, raw=a.raw_frames),
                                backend="hip" if a.gpu_metrics else "host", boxes=a.boxes)
            print(json.dumps({"J&F-Mean": round(jf["J&F-Mean"], 4), "J-Mean": round(jf["J-Mean"], 4), "F-Mean": round(jf["F-Mean"], 4),
                              **({"Box-IoU-Mean": round(jf["Box-IoU-Mean"], 4)} if a.boxes else {})}))
            for name, r in jf["sequences"].items():
                print(json.dumps({"sequence": name, **{k: round(v, 4) for k, v in r.items()}}))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(jf, f, indent=1)
        outputs = None
    elif a.task == "ytvos":    # YouTube-VOS: objects annotated at the frame they first appear in (test_cfg.refs); parity unpinned
        if rank == 0:
            res = ytvos_run(model, YoutubeVos(a.data_root, device=dev, raw=a.raw_frames), a.out_dir)
            print(json.dumps({"videos": len(res["videos"]), "out_dir": a.out_dir,
                              "J&F-Mean": None if res["jf"] is None else round(res["jf"]["J&F-Mean"], 4)}))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(res, f, indent=1)
        outputs = None
    elif a.task == "badja":      # animal pose tracking: the 20 annotated SMAL joints of frame 0 are the query points (datasets.BadjaPoses)
        if rank == 0:          # (one process scores the set, as for JHMDB below; badja_dataset.py:451-571)
            if heatmap:        # --pose-form heatmap: the reference's own first-frame label (BadjaPoses(form='heatmap'))
                ds = BadjaPoses(a.data_root, size=POSE_SIZE["badja"], device=dev, form="heatmap", raw=a.raw_frames)
                m = scored(lambda i: str(ds.videos[i]["name"]), lambda i: badja_frames(ds, i))
                pck = badja_evaluate_heatmap(m, m.indexed(ds) if a.render else ds)
            else:
                pck = badja_evaluate(model, BadjaPoses(a.data_root, size=POSE_SIZE["badja"], device=dev, raw=a.raw_frames))
            print(json.dumps({k: round(v, 2) for k, v in pck.items()}))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(pck, f, indent=1)
        outputs = None
    elif a.task == "jhmdb":    # pose tracking: the 15 joints of frame 0 are the query points (fgvc_amd.datasets.JhmdbPoses)
        # PCK is a mean over ALL videos' joints (jhmdb_dataset.py:174-256), so the set is scored by one process: rank 0 runs it, the
        # other ranks of a `--launcher pytorch` job wait at the common teardown below
        if rank == 0:
            if heatmap:
                ds = JhmdbPoses(a.data_root, split="val", input_size=POSE_SIZE["jhmdb"], device=dev, form="heatmap", raw=a.raw_frames)
                vname = lambda i: os.path.relpath(ds.samples[i]["video_path"], ds.root).replace(os.sep, "_")   # <action>_<video>
                m = scored(vname, lambda i: jhmdb_frames(ds, i))
                pck = jhmdb_evaluate_heatmap(m, m.indexed(ds) if a.render else ds)
            else:
                pck = jhmdb_evaluate(model, JhmdbPoses(a.data_root, split="val", input_size=POSE_SIZE["jhmdb"], device=dev, raw=a.raw_frames))
            print(json.dumps({k: round(v, 2) for k, v in pck.items()}))
            if a.out:
                with open(a.out, "w") as f:
                    json.dump(pck, f, indent=1)
        outputs = None
    else:
        outputs = apis.multi_gpu_test(model, loader) if distributed else apis.single_gpu_test(model, loader)   # :160-190
    if rank == 0 and outputs is not None:
        summary = metrics.tapvid_evaluate(outputs, a.query_mode)                             # :192-198
        keep = ("average_pts_within_thresh", "average_jaccard", "occlusion_accuracy", "ade_visible")
        print(json.dumps({k: round(summary[k], 3) for k in keep}))
        if a.out:
            with open(a.out, "w") as f:
                json.dump(summary, f, indent=1)
        if a.out_dir:
            summaries, results_list = metrics.tapvid_summaries(outputs, a.query_mode, tuple(a.size), tuple(a.size))
            print(json.dumps(metrics.save_results(summaries, results_list, a.out_dir, {"dataset": a.task, "query_mode": a.query_mode})))
    if distributed:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
