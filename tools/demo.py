#!/usr/bin/env python3
"""Track points or propagate a first-frame mask through a clip and write the annotated frames (the reference's tools/demo.py, without cv2 or
mediapy: frames come and go through PIL).

    python tools/demo.py FRAMES_DIR --task points --query-points t x y [t x y ...] --out OUT
    python tools/demo.py FRAMES_DIR --task vos --first-mask MASK.png --out OUT
    python tools/demo.py FRAMES_DIR --task vos --first-mask MASK.png [--boxes] [--box-labels] [--object-trails L] [--mot OUT.txt] [--crops DIR] --out OUT
    python tools/demo.py --synthetic 8 240 320 --task points --query-points 0 100 80 0 200 120 --out OUT
    python tools/demo.py FRAMES_DIR --task points --chain [--chain-visibility consistency] --query-points t x y ... --out OUT
    python tools/demo.py FRAMES_DIR --task points --query-points t x y ... --trails [L] [--trail-width X] [--trail-color track|time] --out OUT
    python tools/demo.py FRAMES_DIR --task flow [--flow-step 1] [--flow-occlusion fb_abs] --out OUT
    python tools/demo.py FRAMES_DIR --task pose --joints x y [x y ...] [--skeleton jhmdb | a-b ...] [--min-conf X] [--heat] --out OUT
    python tools/demo.py CLIP.y4m --task points --query-points t x y ... [--yuv-matrix bt601|bt709] --out OUT
    python tools/demo.py CLIP.y4m --task points --query-points t x y ... --out OUT --out-video OUT.y4m [--out-matrix bt601|bt709] [--out-range limited|full]

FRAMES_DIR holds the clip's frames as JPEG / PNG files, taken in name order.  The frames go to the model as they are decoded -- uint8 RGB, on
the device -- through test_cfg.input = dict(type='rgb8'); the mask task keeps its id maps on the device
(test_cfg.masks='device', section 15); fgvc_amd.viz.render(backend='hip') paints tracks or masks onto the uint8 frames in one launch
(section 16) and OUT gets frame_%05d.png and demo.gif.  --host-render paints with the numpy backend instead (the same bytes, for comparison).
--task flow writes the dense forward flow of every frame pair (test_cfg.flow, section 17) as flow_%05d.flo and, coloured by
fgvc_amd.viz.flow_to_rgb on the host, flow_%05d.png.
CLIP.y4m (what `ffmpeg -i clip.mp4 clip.y4m` writes: uncompressed 8-bit 4:2:0) goes to the model as the file holds it -- packed I420, through
test_cfg.input = dict(type='i420', ...) with the file's chroma siting and range -- and is painted on
ops.yuv_frames_to_rgb8's bytes.  A file whose C tag is 4:2:2, 4:4:4 or 10 / 12 bits (C422, C444, C420p10, ..: `ffmpeg -pix_fmt yuv422p10le`) goes
through datasets.read_y4m_planes, test_cfg.input = dict(type='yuv422p10', ...) and ops.yuv_planes_to_rgb8 (section 26); what is written stays
8-bit.  A Y4M file does not say which matrix made its YUV: --yuv-matrix, by default bt709 from 720 rows up, else bt601.
--out-video OUT.y4m also writes the result as video, for all three tasks (for --task flow the coloured flow frames): the painted frames go
through fgvc_amd.viz.frames_to_yuv420 -- one launch of fgvc_frames_rgb8_to_yuv420 on the device unless --host-render is given (DESIGN.md
section 20) -- and only the packed I420 frames, 1.5 bytes a pixel, cross to the host, where datasets.write_y4m writes them with the clip's frame
rate: `ffmpeg -i OUT.y4m out.mp4` takes the file.  Matrix, range and chroma siting are those the clip was decoded with for a .y4m input, else
yuv_matrix_default(height), 'limited' and 'left'; --out-matrix and --out-range override.  A Y4M header has no matrix tag: the printed line says
which one was used.  Frames with an odd side are refused (Y4M 4:2:0 has no odd form).
--task pose propagates the joints --joints of frame 0 as heat maps (datasets.pose_heatmaps; test_cfg.coords=True with test_cfg.pose) and
paints them with viz.paint_pose: the limbs of --skeleton, the dots, a joint whose map's peak is below --min-conf hidden; --heat blends the
propagated maps in, made on the device from the kept field in frame chunks (maps at the frames' size only: not with another --size).

--trails [L] (--task points; L = 8 when left out) also draws every point's last L steps as a fading poly-line under the dots, what the reference
demo's second video shows: viz.render(trail=L), still one launch (fgvc_render_trails_u8).  --trail-width is the line
width in pixels, --trail-color time the reference's colouring by time in place of the point's own colour.  It goes with --chain (a trail stops
where a chained track ends or is not visible), with --out-video and with --host-render.
--boxes (--task vos) draws every object's box on every frame it is present on, --box-labels its id on a tag above the box, --object-trails L the
last L steps of its centroid with a dot on the centroid, and --mot OUT.txt writes the boxes as a MOTChallenge text file: the model runs with
test_cfg.objects = dict(stats=True) (one launch of fgvc_seg_object_stats_u8 on the masks), viz.render(boxes=...) paints the
boxes with the overlay in one launch, and the trails are a second call, viz.paint_trails, onto that output.  --clean [--min-area N] [--keep-largest] [--fill-holes]
[--max-hole N] cleans the propagated masks first (test_cfg.clean).  They go with --mask, --fuse,
--edge-aware, --out-video and --host-render.
--crops DIR [--crop-size H W] [--crop-pad X] [--crop-smooth R] [--crop-masks] (--task vos) writes every object's crop: a window that follows
the object (metrics.object_windows_host's rule), resampled anti-aliased from the decoded uint8 frames onto H x W on the
device (ops.object_windows + ops.object_crops: three launches for the clip), as DIR/obj%02d/frame_%05d.png with a contact sheet sheet.png per
object, and with --out-video and even crop sides one DIR/obj%02d.y4m per object through the same encoder.
Query points are (t, x, y) in the pixel frame of the clip; with --size h w the model runs at that size and the tracks are scaled back.
Without --checkpoint the encoder has its seeded initial weights: the pipeline runs, the tracks mean little.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fgvc_amd.mmpt_api as api  # noqa: E402
from fgvc_amd import viz  # noqa: E402

EXTENSIONS = (".jpg", ".jpeg", ".png")


def load_frames(path: str) -> np.ndarray:
    from PIL import Image
    names = sorted(n for n in os.listdir(path) if n.lower().endswith(EXTENSIONS))
    if not names:
        raise FileNotFoundError(f"{path}: no {' / '.join(EXTENSIONS)} files")
    frames = [np.asarray(Image.open(os.path.join(path, n)).convert("RGB")) for n in names]
    if len({f.shape for f in frames}) != 1:
        raise ValueError(f"{path}: the frames differ in size")
    return np.stack(frames)


def synthetic_frames(T: int, H: int, W: int, seed: int = 0) -> np.ndarray:
    """A smooth random texture that drifts by (1, 2) px a frame under a fixed vignette, plus noise: (T, H, W, 3) uint8."""
    rng = np.random.default_rng(seed)
    cell = 8
    coarse = rng.random((-(-(H + T) // cell) + 2, -(-(W + 2 * T) // cell) + 2, 3))
    tex = np.kron(coarse, np.ones((cell, cell, 1)))
    k = np.ones(cell) / cell
    for ax in (0, 1):
        tex = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, tex)
    yy, xx = np.mgrid[0:H, 0:W]
    shade = 1.0 - 0.3 * (((yy / H - 0.5) ** 2 + (xx / W - 0.5) ** 2))[..., None]
    out = [tex[cell + t:cell + t + H, cell + 2 * t:cell + 2 * t + W] * shade * 300.0 - 22.0 + rng.normal(0.0, 4.0, (H, W, 3)) for t in range(T)]
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def is_y4m(path) -> bool:
    return bool(path) and os.path.isfile(path) and path.lower().endswith(".y4m")


def yuv_matrix_default(height: int) -> str:
    """What a file that does not say is taken to be: HD material (720 rows and up) BT.709, anything smaller BT.601."""
    return "bt709" if height >= 720 else "bt601"


def load_y4m(a, dev):
    """CLIP.y4m -> (the packed frames as the file holds them -- I420 (T, 3 H / 2, W) uint8, or a planar ops.YUV_PIXEL_FORMATS arrangement in
    uint8 / uint16 words for a C tag of 4:2:2, 4:4:4, 10 or 12 bits -- on the device, their RGB bytes (T, H, W, 3) on the device,
    test_cfg.input of the file's format without its size)."""
    from fgvc_amd import datasets, ops
    packed, info = datasets.read_y4m_planes(a.frames)
    if packed.shape[0] == 0:
        raise ValueError(f"{a.frames}: no frames")
    fmt, depth = info.pop("format"), info.pop("depth")
    what = f"siting {info['siting']}" if fmt == "i420" else f"{fmt} ({depth} bits)"
    matrix = a.yuv_matrix or yuv_matrix_default(info["height"])
    print(f"{a.frames}: {packed.shape[0]} frames of {info['height']} x {info['width']}, {what}, {info['range']} range; matrix {matrix} "
          f"({'--yuv-matrix' if a.yuv_matrix else 'by the height: the file does not say'})")
    a.yuv_info = dict(info, matrix=matrix)
    packed = packed.to(dev)
    kw = dict(matrix=matrix, range=info["range"], siting=info["siting"])
    if fmt == "i420":                                                         # 8-bit 4:2:0: the fixed-format entries
        rgb = ops.yuv_frames_to_rgb8(*ops.yuv420_planes(packed, fmt), **kw)
    else:
        _, sx, sy, depth, shift, _ = ops.YUV_PIXEL_FORMATS[fmt]
        if sx == 1:                                                           # (4:4:4 has no siting: test_cfg.input refuses the key)
            del kw["siting"]
        rgb = ops.yuv_planes_to_rgb8(*ops.yuv_planes(packed, fmt), depth, shift, (sx, sy), **kw)
    return packed, rgb, dict(type=fmt, **kw)


load_y4m_planes = load_y4m            # (the name a 4:2:2 / 4:4:4 / 10- or 12-bit file's loader had on its own)


def _input(a, size):
    """test_cfg.input of the clip at hand: RGB bytes, or what load_y4m made of the file."""
    if getattr(a, "yuv_input", None):
        return dict(a.yuv_input, size=size)
    return dict(type="rgb8", size=size, layout="thwc")


def _raw(a, frames, dev) -> torch.Tensor:
    """The clip as the model takes it, on the device: (T, H, W, 3) RGB bytes, or the Y4M file's packed frames."""
    packed = getattr(a, "yuv_packed", None)
    if packed is not None:
        return packed
    return frames.to(dev) if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev)


def build_model(a, dev, **extra):
    cfg = dict(precede_frames=a.precede_frames, topk=a.topk, temperature=0.07, neighbor_range=a.neighbor_range, with_first=True,
               with_first_neighbor=True, batch_step=a.batch_step, **extra)
    model = api.build_model(dict(type=a.tracker, backbone=dict(type="ResNet", depth=18, strides=tuple(a.strides), out_indices=(2,),
                                                              pool_type="none")), train_cfg=None, test_cfg=api.ConfigDict(**cfg))
    torch.manual_seed(a.seed)
    model.init_weights()
    if a.checkpoint:
        api.load_checkpoint(model, a.checkpoint)
    return model.to(dev).eval()


def run_points(a, frames: np.ndarray, dev):
    """-> tracks (P, T, 2) float64 in the clip's pixel frame, visibles (P, T) bool (from the query time on; with --chain the chained call's own
    visibility, on both sides of it), query points (P, 3) as returned."""
    T, H, W = frames.shape[:3]
    q = np.asarray(a.query_points, np.float64)
    if q.size == 0 or q.size % 3:
        raise ValueError("--query-points: t x y [t x y ...]")
    q = q.reshape(-1, 3)
    if (q[:, 0] < 0).any() or (q[:, 0] >= T).any():
        raise ValueError(f"--query-points: a query time outside 0 .. {T - 1}")
    size = tuple(a.size) if a.size else (H, W)
    q[:, 1:] = viz.scale_tracks(q[:, 1:], (H, W), size)
    chain = dict(chain=dict(type="flow", visibility=a.chain_visibility)) if a.chain else {}
    model = build_model(a, dev, input=_input(a, tuple(a.size) if a.size else None), **chain)
    qp = torch.from_numpy(q).float()[None].to(dev)
    P = q.shape[0]
    with torch.no_grad():
        out = model(test_mode=True, rgbs=_raw(a, frames, dev)[None], query_points=qp,
                    trajectories=torch.zeros(1, T, P, 2, device=dev), visibilities=torch.ones(1, T, P, device=dev))
    traj, qp_out = out[2][0], out[4][0]                                  # (T, P, 2) at the model's size; the points in the order of its columns
    tracks = viz.scale_tracks(traj.permute(1, 0, 2), size, (H, W))
    if a.chain:                                                          # tracked on both sides of the query time, with a predicted visibility
        visibles = out[3][0].t().cpu().numpy() != 0
    else:
        visibles = np.arange(T)[None, :] >= qp_out[:, :1].cpu().numpy()
    return tracks, visibles, qp_out.cpu().numpy()


def parse_skeleton(spec, num_joints: int):
    """--skeleton jhmdb | a-b [a-b ...] -> (E, 2) int32, or None without the flag."""
    if not spec:
        return None
    if len(spec) == 1 and spec[0] == "jhmdb":
        edges = viz.JHMDB_SKELETON
    else:
        try:
            edges = np.asarray([[int(v) for v in e.split("-")] for e in spec], np.int32).reshape(-1, 2)
        except ValueError:
            raise ValueError(f"--skeleton: 'jhmdb' or edges a-b of joint indices, got {spec}") from None
    return viz._check_skeleton(edges, num_joints)


def run_pose(a, frames, dev):
    """-> joints (K, T, 2) float64 in the clip's pixel frame, visibles (K, T) bool, the model (its last_pose holds the peaks and, with --heat,
    the field the maps are made from).  The first-frame maps are datasets.pose_heatmaps of --joints at the model's size."""
    from fgvc_amd import datasets
    T, H, W = frames.shape[:3]
    j = np.asarray(a.joints, np.float64)
    if j.size == 0 or j.size % 2:
        raise ValueError("--joints: x y [x y ...]")
    j = j.reshape(-1, 2)
    size = tuple(a.size) if a.size else (H, W)
    if a.heat and size != (H, W):
        raise ValueError(f"--heat: the heat overlay needs maps at the frames' size {H} x {W}, and --size {size[0]} {size[1]} makes them at "
                         f"another; resizing maps is out of scope (drop --size or --heat)")
    heat = datasets.pose_heatmaps(j, (H, W), a.joint_sigma, size)                          # (K, h, w) float64
    model = build_model(a, dev, input=_input(a, tuple(a.size) if a.size else None), coords=True,
                        pose=dict(confidence=True, keep_field=bool(a.heat)))
    with torch.no_grad():
        out = model(test_mode=True, imgs=_raw(a, frames, dev)[None, None], ref_seg_map=torch.from_numpy(heat)[None].to(dev),
                    img_meta=[dict(original_shape=size)])
    coords = out[0]                                                                       # (2, K, T) at the model's size
    joints = viz.scale_tracks(viz.pose_tracks(coords), size, (H, W))
    visibles = viz.pose_visibles(coords, model.last_pose["peak"], a.min_conf)
    return joints, visibles, model


def paint_pose(a, frames, joints, visibles, model, dev):
    """The painted clip (T, H, W, 3) uint8 as numpy.  With --heat the maps are made on the device from the kept field, in frame chunks under
    test_cfg.maps_budget, and every chunk is painted on its own: the whole (T, K, H, W) stack never exists, on either side."""
    from fgvc_amd import engine
    K = joints.shape[0]
    kw = dict(skeleton=parse_skeleton(a.skeleton, K), limb_width=a.limb_width, radius=a.radius)
    host = a.host_render
    f = (frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames) if host else \
        (frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev))
    backend = "host" if host else "hip"
    if not a.heat:
        out = viz.paint_pose(f, joints, visibles, backend=backend, **kw)
        return out if host else out.cpu().numpy()
    field = model.last_pose["field"]
    T, H, W = f.shape[:3]
    parts = []
    for f0, f1 in engine.plan_map_chunks(T, K, (H, W), 4, model._maps_budget()):
        maps = field.maps(f0, f1, out_dtype=torch.float32)                                # (f1 - f0, K, H, W) on the device
        part = viz.paint_pose(f[f0:f1], joints[:, f0:f1], visibles[:, f0:f1], heat=maps.cpu().numpy() if host else maps,
                              heat_gain=a.heat_gain, backend=backend, **kw)
        parts.append(part if host else part.cpu().numpy())
    return np.concatenate(parts)


def _mask_png(path, H, W, flag) -> np.ndarray:
    from PIL import Image
    mask = np.asarray(Image.open(path))
    if mask.ndim != 2 or mask.shape != (H, W):
        raise ValueError(f"{flag}: a palette or grey PNG of object ids, {H} x {W} as the frames, got an array of shape {mask.shape}")
    return mask.astype(np.uint8)


def run_vos(a, frames: np.ndarray, dev) -> torch.Tensor:
    """-> (T, H, W) uint8 object ids on the device, frame 0 the given mask.  With --mask T PNG (test_cfg.refs): masks at any frames, the
    first annotated frame the given one; --confidence also writes conf_%05d.png into --out and prints the frame scores."""
    T, H, W = frames.shape[:3]
    imgs, meta = _raw(a, frames, dev)[None, None], [dict(original_shape=(H, W))]
    edge = {}
    if a.edge_aware:               # test_cfg.readout: label edges follow the frames' own
        edge = dict(readout=dict(type="guided", radius=a.edge_radius, sigma_space=1.0, sigma_range=a.edge_sigma_range))
    if wants_objects(a):           # test_cfg.objects: the masks' boxes, centroids and areas, kept in a.objects
        edge = dict(edge, objects=dict(stats=True))
    if a.clean:                    # test_cfg.clean: despeckle, keep the largest part, fill holes -- before the boxes
        edge = dict(edge, clean=dict(min_area=a.min_area, keep="largest" if a.keep_largest else "all", fill_holes=a.fill_holes,
                                     max_hole_area=a.max_hole))
    a.objects = a.cleaned = None
    if not a.mask:
        mask = _mask_png(a.first_mask, H, W, "--first-mask")
        model = build_model(a, dev, input=_input(a, None), masks="device", **edge)
        with torch.no_grad():
            out = model(test_mode=True, imgs=imgs, ref_seg_map=torch.from_numpy(mask)[None].to(dev), img_meta=meta)
        a.objects, a.cleaned = model.last_objects, model.last_clean
        return out[0]
    refs = {}
    if a.first_mask:
        refs[0] = torch.from_numpy(_mask_png(a.first_mask, H, W, "--first-mask"))
    for t, path in a.mask:
        if not t.lstrip("-").isdigit() or not 0 <= int(t) < T or int(t) in refs:
            raise ValueError(f"--mask {t} {path}: a frame index 0 .. {T - 1}, each frame once")
        refs[int(t)] = torch.from_numpy(_mask_png(path, H, W, "--mask"))
    spec = dict(direction="both" if a.both_ways else "forward", override=a.override, confidence=a.confidence)
    if a.fuse:                     # the frames between two masks blend the forward and the backward sweep; the model
        spec.update(direction="both", override="all", fuse="linear", confidence=True)   # call keeps the counts beside the confidence
    model = build_model(a, dev, input=_input(a, None), masks="device", **edge, refs=spec)
    from fgvc_amd import engine
    with torch.no_grad():
        out = model(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    lc = model.last_confidence
    a.objects, a.cleaned = model.last_objects, model.last_clean
    if a.fuse:
        print("disagree: " + " ".join(str(v) for v in lc["disagree"].tolist()))
        print(f"annotate next by disagreement: frame {engine.next_frame_to_annotate_by(lc['disagree'], refs)}")
    if a.confidence:
        from PIL import Image
        os.makedirs(a.out, exist_ok=True)
        for f, c in enumerate(lc["conf"].cpu().numpy()):
            Image.fromarray(c).save(os.path.join(a.out, f"conf_{f:05d}.png"))
        print("frame_score: " + " ".join(f"{v:.4f}" for v in lc["frame_score"].tolist()))
        print(f"annotate next: frame {engine.next_frame_to_annotate(lc['frame_score'], refs)}")
    return out[0]


def wants_objects(a) -> bool:
    return bool(a.boxes or a.box_labels or a.object_trails is not None or a.mot or a.crops)


def box_arguments(a, tr) -> dict:
    """viz.render's box arguments for an engine.ObjectTracks: the objects 1 .. N - 1 (the background's row is left out, so 255 objects fit
    the renderer's 255 boxes), each where it is present, in its palette colour, with its id on the tag."""
    N = tr.present.shape[1]
    kw = dict(boxes=tr.boxes[:, 1:], box_visibles=tr.present[:, 1:], box_colors=viz.davis_palette()[1:N])
    if a.box_labels:
        kw["box_labels"] = np.arange(1, N)
    return kw


def write_crops(a, frames, ids, tr, video, dev) -> dict:
    """--crops DIR: every object's window on every frame, resampled onto --crop-size from the decoded uint8 frames
    (with YUV input: the bytes the renderer takes) -- ObjectTracks.crops on the device statistics, three launches for the clip, nothing
    read back before the results -- written as DIR/obj%02d/frame_%05d.png (the frames the object is present on) and DIR/obj%02d/sheet.png
    (viz.contact_sheet of all frames, absent ones black), with --crop-masks also mask_%05d.png, with --out-video and even crop sides
    DIR/obj%02d.y4m through the same encoder."""
    from PIL import Image
    on_dev = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev)
    size = tuple(a.crop_size)
    oc = tr.crops(on_dev, size=size, pad=a.crop_pad, smooth=a.crop_smooth, masks=a.crop_masks, ids=ids if a.crop_masks else None,
                  mask_size=tuple(ids.shape[1:]))
    crops, valid = oc.crops.cpu().numpy(), oc.valid
    masks = oc.masks.cpu().numpy() if a.crop_masks else None
    T = crops.shape[0]
    cols = max(1, min(T, 10))
    for j, o in enumerate(oc.objects):
        d = os.path.join(a.crops, f"obj{o:02d}")
        os.makedirs(d, exist_ok=True)
        for t in range(T):
            if valid[t, j]:
                Image.fromarray(crops[t, j]).save(os.path.join(d, f"frame_{t:05d}.png"))
                if masks is not None:
                    Image.fromarray(masks[t, j]).save(os.path.join(d, f"mask_{t:05d}.png"))
        Image.fromarray(viz.contact_sheet(crops[:, j:j + 1], valid[:, j:j + 1], cols=cols)).save(os.path.join(d, "sheet.png"))
        if video and size[0] % 2 == 0 and size[1] % 2 == 0:
            write_video(os.path.join(a.crops, f"obj{o:02d}.y4m"), oc.crops[:, j].contiguous(), video, dev, host=a.host_render)
    print(f"{a.crops}: {int(valid.sum())} crops of {size[0]} x {size[1]} for {len(oc.objects)} object(s) as obj%02d/frame_%05d.png and sheet.png"
          f"{', masks' if a.crop_masks else ''} (pad {a.crop_pad}, smooth {a.crop_smooth})")
    return dict(crops=crops, crop_masks=masks, crop_windows=oc.windows.cpu().numpy(), crop_valid=valid)


def paint_object_trails(a, rendered, tr, backend):
    """The centroids' last --object-trails steps and a dot on every centroid, onto the rendered frames: viz.paint_trails, a second call."""
    tracks, vis = tr.centroid_tracks()
    if tracks.shape[0] <= 1:
        return rendered
    colors = viz.davis_palette()[1:tracks.shape[0]]
    return viz.paint_trails(rendered, tracks[1:], vis[1:], colors=colors, trail=a.object_trails, radius=a.radius, backend=backend)


def run_flow(a, frames: np.ndarray, dev) -> dict:
    """-> forward_test_flow's dict of device tensors at the clip's own size (test_cfg.flow)."""
    flow = dict(type="window", step=a.flow_step, occlusion=a.flow_occlusion)
    model = build_model(a, dev, input=_input(a, None), flow=flow)
    with torch.no_grad():
        return model(test_mode=True, imgs=_raw(a, frames, dev)[None, None])


def write_flow(out_dir: str, out: dict) -> np.ndarray:
    """flow_%05d.flo (Middlebury) and flow_%05d.png (viz.flow_to_rgb, one colour scale for the clip) of the forward flow; with a check,
    occ_%05d.png (white = consistent).  -> the coloured frames (n, H, W, 3) uint8."""
    from PIL import Image
    from fgvc_amd import datasets
    os.makedirs(out_dir, exist_ok=True)
    fw = out["flow_fw"].cpu().numpy()
    rgb = viz.flow_to_rgb(fw)
    for t in range(fw.shape[0]):
        datasets.write_flo(os.path.join(out_dir, f"flow_{t:05d}.flo"), fw[t])
        Image.fromarray(rgb[t]).save(os.path.join(out_dir, f"flow_{t:05d}.png"))
        if "occ_fw" in out:
            Image.fromarray((out["occ_fw"][t, 0].cpu().numpy() * 255).astype(np.uint8)).save(os.path.join(out_dir, f"occ_{t:05d}.png"))
    return rgb


def write(out_dir: str, rendered: np.ndarray, fps: float):
    from PIL import Image
    os.makedirs(out_dir, exist_ok=True)
    images = [Image.fromarray(f) for f in rendered]
    for t, im in enumerate(images):
        im.save(os.path.join(out_dir, f"frame_{t:05d}.png"))
    images[0].save(os.path.join(out_dir, "demo.gif"), save_all=True, append_images=images[1:], duration=int(round(1000.0 / fps)), loop=0)


def video_settings(a, height: int) -> dict:
    """How --out-video encodes: dict(matrix, range, siting, fps=(num, den)).  A .y4m input hands on the matrix it was decoded with, its range,
    its chroma siting and its frame rate; anything else gets yuv_matrix_default(height), 'limited', 'left' and --fps.  --out-matrix and
    --out-range override."""
    from fractions import Fraction
    info = getattr(a, "yuv_info", None) or {}
    fps = tuple(info.get("fps", (0, 0)))
    if fps[0] <= 0 or fps[1] <= 0:                                        # (a Y4M header may leave the rate out)
        fr = Fraction(a.fps).limit_denominator(1001)
        fps = (fr.numerator, fr.denominator)
    return dict(matrix=a.out_matrix or info.get("matrix") or yuv_matrix_default(height), range=a.out_range or info.get("range", "limited"),
                siting=info.get("siting", "left"), fps=fps)


def check_video_size(height: int, width: int) -> None:
    if height % 2 or width % 2:
        raise ValueError(f"--out-video: {height} x {width} frames have an odd side, and Y4M 4:2:0 has no odd form; crop or pad the clip to even sides")


def write_video(path: str, rendered, settings: dict, dev, host: bool = False) -> torch.Tensor:
    """The painted frames (T, H, W, 3) uint8 (numpy or a tensor on either device) -> a Y4M file of 8-bit 4:2:0 frames.  Encoded on `dev` by
    fgvc_frames_rgb8_to_yuv420 (frames already there stay there: only the packed frames come to the host), or with host=True by
    datasets.rgb8_to_yuv420 on the CPU -- the same bytes.  -> the packed I420 frames (T, 3 H / 2, W) as written, a CPU tensor."""
    from fgvc_amd import datasets
    kw = dict(matrix=settings["matrix"], range=settings["range"], siting=settings["siting"])
    f = rendered if isinstance(rendered, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(rendered))
    check_video_size(f.shape[1], f.shape[2])
    if host:
        packed = viz.frames_to_yuv420(f.cpu(), "i420", backend="host", **kw)
    else:
        packed = viz.frames_to_yuv420(f.to(dev), "i420", backend="hip", **kw).cpu()
    datasets.write_y4m(path, packed, fps=settings["fps"], siting=kw["siting"], range=kw["range"])
    print(f"{path}: {packed.shape[0]} frames of {f.shape[1]} x {f.shape[2]} as 8-bit 4:2:0 ({'host' if host else 'hip'} encoder), matrix {kw['matrix']}, "
          f"{kw['range']} range, siting {kw['siting']}, {settings['fps'][0]}:{settings['fps'][1]} fps -- the Y4M header has no matrix tag: tell the "
          f"next tool (ffmpeg: -colorspace {'bt709' if kw['matrix'] == 'bt709' else 'smpte170m'})")
    return packed


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("frames", nargs="?", help="a directory of JPEG / PNG frames, or a .y4m file (8-bit 4:2:0)")
    ap.add_argument("--yuv-matrix", choices=("bt601", "bt709"), default=None,
                    help="the matrix of a .y4m clip's YUV (the file does not say); default: bt709 from 720 rows up, else bt601")
    ap.add_argument("--synthetic", type=int, nargs=3, metavar=("T", "H", "W"), help="a generated clip instead of FRAMES_DIR")
    ap.add_argument("--task", choices=("points", "vos", "flow", "pose"), required=True)
    ap.add_argument("--joints", type=float, nargs="+", default=[], metavar="V", help="x y [x y ...], pixels of frame 0 (--task pose)")
    ap.add_argument("--joint-sigma", type=float, default=4.0, help="the first-frame Gaussians' sigma in pixels (--task pose)")
    ap.add_argument("--skeleton", nargs="+", default=None, metavar="EDGE", help="'jhmdb' or limbs a-b [a-b ...] of joint indices (--task pose)")
    ap.add_argument("--min-conf", type=float, default=None, metavar="X", help="hide a joint whose map's peak is below X (--task pose)")
    ap.add_argument("--heat", action="store_true", help="blend the propagated heat maps in (--task pose; maps at the frames' size only)")
    ap.add_argument("--heat-gain", type=float, default=1.0, help="with --heat: the maps' values times this, clamped to [0, 1], is the opacity")
    ap.add_argument("--limb-width", type=float, default=2.0, metavar="X", help="with --skeleton: the line width in pixels (1 .. 16)")
    ap.add_argument("--flow-step", type=int, default=1, help="frame distance of a flow pair (--task flow)")
    ap.add_argument("--flow-occlusion", choices=("consistency", "fb_abs"), default=None, help="also write the forward check's mask (--task flow)")
    ap.add_argument("--chain", action="store_true",
                    help="--task points: track by chaining the dense flow, forward and backward in time (test_cfg.chain, DESIGN.md section 18)")
    ap.add_argument("--chain-visibility", choices=("frame", "consistency"), default="frame", help="with --chain: chain.visibility")
    ap.add_argument("--query-points", type=float, nargs="+", default=[], metavar="V", help="t x y [t x y ...], pixels of the clip")
    ap.add_argument("--first-mask", help="PNG of object ids for frame 0 (--task vos)")
    ap.add_argument("--mask", nargs=2, action="append", default=[], metavar=("T", "PNG"),
                    help="PNG of object ids for frame T, repeatable (--task vos; test_cfg.refs: objects may enter at any frame)")
    ap.add_argument("--both-ways", action="store_true", help="with --mask: also label the frames before the first annotated one")
    ap.add_argument("--override", choices=("new", "all"), default="new",
                    help="with --mask: a later mask brings in its new objects only, or replaces the frame's labels (a correction)")
    ap.add_argument("--fuse", action="store_true",
                    help="with --mask: blend the forward and the backward sweep between two masks (test_cfg.refs fuse='linear'; implies "
                         "--both-ways --override all) and print the per-frame disagreement counts")
    ap.add_argument("--confidence", action="store_true",
                    help="with --mask: write conf_%%05d.png (the top-two gap per pixel) and print the frame scores and the frame to annotate next")
    ap.add_argument("--edge-aware", action="store_true",
                    help="--task vos: the edge-aware read-out (test_cfg.readout type='guided': the masks' edges follow the frames')")
    ap.add_argument("--edge-radius", type=int, default=2, choices=(1, 2, 3), help="with --edge-aware: cells around a pixel, per side")
    ap.add_argument("--edge-sigma-range", type=float, default=0.1, metavar="X",
                    help="with --edge-aware: the colour sigma in Lab-normalised units (untuned default)")
    ap.add_argument("--boxes", action="store_true", help="--task vos: draw every object's box (test_cfg.objects, viz.render(boxes=...))")
    ap.add_argument("--box-labels", action="store_true", help="--task vos: the boxes with the object's id on a tag (implies --boxes)")
    ap.add_argument("--object-trails", type=int, default=None, metavar="L", help="--task vos: the last L steps (1 .. 64) of every object's centroid")
    ap.add_argument("--mot", default=None, metavar="OUT.txt", help="--task vos: write the boxes as a MOTChallenge text file")
    ap.add_argument("--crops", default=None, metavar="DIR", help="--task vos: write every object's crop per frame and a contact sheet (test_cfg.objects)")
    ap.add_argument("--crop-size", type=int, nargs=2, default=(128, 128), metavar=("H", "W"), help="with --crops: the crops' size")
    ap.add_argument("--crop-pad", type=float, default=0.125, metavar="X", help="with --crops: the box grows by this share of its side, 0 .. 4")
    ap.add_argument("--crop-smooth", type=int, default=0, metavar="R", help="with --crops: average the window over R frames on each side")
    ap.add_argument("--crop-masks", action="store_true", help="with --crops: also every object's mask in its window")
    ap.add_argument("--clean", action="store_true",
                    help="--task vos: clean the propagated masks on the device before anything reads them (test_cfg.clean, ops.seg_clean)")
    ap.add_argument("--min-area", type=int, default=0, metavar="N", help="with --clean: drop connected parts of an object below N pixels")
    ap.add_argument("--keep-largest", action="store_true", help="with --clean: keep only the largest connected part of every object")
    ap.add_argument("--fill-holes", action="store_true", help="with --clean: fill background enclosed by one object")
    ap.add_argument("--max-hole", type=int, default=None, metavar="N", help="with --fill-holes: only holes of at most N pixels")
    ap.add_argument("--out", required=True)
    ap.add_argument("--host-render", action="store_true", help="paint (and, with --out-video, encode) with viz's numpy backend instead of the kernels")
    ap.add_argument("--out-video", default=None, metavar="OUT.y4m", help="also write the result as a YUV4MPEG2 file of 8-bit 4:2:0 frames")
    ap.add_argument("--out-matrix", choices=("bt601", "bt709"), default=None,
                    help="the matrix of --out-video; default: the one a .y4m clip was decoded with, else bt709 from 720 rows up, else bt601")
    ap.add_argument("--out-range", choices=("limited", "full"), default=None, help="the range of --out-video; default: a .y4m clip's own, else limited")
    ap.add_argument("--size", type=int, nargs=2, metavar=("h", "w"), help="run the points model at this size")
    ap.add_argument("--radius", type=int, default=None)
    ap.add_argument("--trails", type=int, nargs="?", const=8, default=None, metavar="L",
                    help="--task points: draw every point's last L steps (1 .. 64, 8 when L is left out) as a fading line under the dots")
    ap.add_argument("--trail-width", type=float, default=2.0, metavar="X", help="with --trails: the line width in pixels (1 .. 16)")
    ap.add_argument("--trail-color", choices=("track", "time"), default="track",
                    help="with --trails: the point's own colour, or the reference's colouring by time ('spring')")
    ap.add_argument("--alpha", type=int, default=128)
    ap.add_argument("--no-contour", action="store_true")
    ap.add_argument("--fps", type=float, default=10.0)
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--tracker", default="VanillaTracker", choices=("VanillaTracker", "HRVanillaTracker"))
    ap.add_argument("--strides", type=int, nargs=4, default=(1, 2, 1, 1))
    ap.add_argument("--neighbor-range", type=int, default=30)
    ap.add_argument("--precede-frames", type=int, default=5)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--batch-step", type=int, default=8)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    if (a.frames is None) == (a.synthetic is None):
        ap.error("give FRAMES_DIR or --synthetic T H W")
    if a.task == "points" and not a.query_points:
        ap.error("--task points needs --query-points")
    if a.task == "pose" and (not a.joints or len(a.joints) % 2):
        ap.error("--task pose needs --joints x y [x y ...]")
    if a.task != "pose" and (a.joints or a.skeleton or a.heat or a.min_conf is not None or a.heat_gain != 1.0 or a.limb_width != 2.0):
        ap.error("--joints, --skeleton, --min-conf, --heat, --heat-gain and --limb-width go with --task pose")
    if a.task == "pose" and a.heat and a.size and a.synthetic and tuple(a.size) != tuple(a.synthetic[1:]):
        ap.error("--heat: the heat overlay needs maps at the frames' size; --size makes them at another (resizing maps is out of scope)")
    if a.task == "vos" and not (a.first_mask or a.mask):
        ap.error("--task vos needs --first-mask (or --mask T PNG)")
    if (a.both_ways or a.confidence or a.fuse or a.override != "new") and not a.mask:
        ap.error("--both-ways, --override, --fuse and --confidence go with --mask T PNG")
    if (a.edge_aware or a.edge_radius != 2 or a.edge_sigma_range != 0.1) and not (a.task == "vos" and a.edge_aware):
        ap.error("--edge-aware goes with --task vos; --edge-radius and --edge-sigma-range go with --edge-aware")
    if a.task != "vos" and (a.boxes or a.box_labels or a.object_trails is not None or a.mot):
        ap.error("--boxes, --box-labels, --object-trails and --mot go with --task vos")
    if (a.clean or a.min_area or a.keep_largest or a.fill_holes or a.max_hole is not None) and not (a.task == "vos" and a.clean):
        ap.error("--clean goes with --task vos; --min-area, --keep-largest, --fill-holes and --max-hole go with --clean")
    if (a.crops or tuple(a.crop_size) != (128, 128) or a.crop_pad != 0.125 or a.crop_smooth or a.crop_masks) and not (a.task == "vos" and a.crops):
        ap.error("--crops goes with --task vos; --crop-size, --crop-pad, --crop-smooth and --crop-masks go with --crops")
    if a.object_trails is not None and not 1 <= a.object_trails <= 64:
        ap.error("--object-trails L: 1 .. 64")
    if a.yuv_matrix and not (a.frames or "").lower().endswith(".y4m"):
        ap.error("--yuv-matrix goes with a .y4m clip")
    if a.trails is not None and a.task != "points":
        ap.error("--trails goes with --task points")
    if a.trails is None and (a.trail_width != 2.0 or a.trail_color != "track"):
        ap.error("--trail-width and --trail-color go with --trails")
    if (a.out_matrix or a.out_range) and not a.out_video:
        ap.error("--out-matrix and --out-range go with --out-video")
    return a


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/demo.py runs the model on the GPU (fgvc_amd has no CPU path)")
    dev = torch.device("cuda:0")
    a.yuv_packed = a.yuv_input = a.yuv_info = None
    if is_y4m(a.frames):
        a.yuv_packed, frames, a.yuv_input = load_y4m(a, dev)             # frames: the RGB bytes, on the device
    else:
        frames = synthetic_frames(*a.synthetic, seed=a.seed) if a.synthetic else load_frames(a.frames)
    tracks = visibles = ids = points = None
    video = None
    if a.out_video:
        check_video_size(frames.shape[1], frames.shape[2])               # before the model runs
        video = video_settings(a, frames.shape[1])
    if a.task == "flow":
        coloured = write_flow(a.out, run_flow(a, frames, dev))
        print(f"{a.out}: {len(coloured)} flow fields of {frames.shape[1]} x {frames.shape[2]} as flow_%05d.flo and flow_%05d.png")
        if video:
            write_video(a.out_video, coloured, video, dev, host=a.host_render)
        return
    if a.task == "pose":
        tracks, visibles, model = run_pose(a, frames, dev)
        rendered = paint_pose(a, frames, tracks, visibles, model, dev)
        packed = write_video(a.out_video, rendered if a.host_render else torch.from_numpy(rendered).to(dev), video, dev,
                             host=a.host_render) if video else None
        frames = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
        write(a.out, rendered, a.fps)
        print(f"{a.out}: {len(rendered)} frames of {frames.shape[1]} x {frames.shape[2]} and demo.gif (pose, {tracks.shape[0]} joints"
              f"{', heat maps' if a.heat else ''}, {'host' if a.host_render else 'hip'} renderer)")
        r = dict(frames=frames, tracks=tracks, visibles=visibles, peak=model.last_pose["peak"], rendered=rendered)
        if video:
            r.update(video=packed.numpy(), video_settings=video)
        return r
    if a.task == "points":
        tracks, visibles, points = run_points(a, frames, dev)
    else:
        ids = run_vos(a, frames, dev)
    kw = dict(ids=ids, tracks=tracks, visibles=visibles, radius=a.radius, alpha=a.alpha, contour=not a.no_contour)
    if a.trails is not None:
        kw.update(trail=a.trails, linewidth=a.trail_width, trail_color_by=a.trail_color)
    objects = getattr(a, "objects", None)
    if objects is not None and (a.boxes or a.box_labels):
        kw.update(box_arguments(a, objects))
    if objects is not None and a.mot:
        from fgvc_amd import datasets
        print(f"{a.mot}: {datasets.write_mot(a.mot, objects)} boxes of {objects.present.shape[1] - 1} object(s) in the MOTChallenge text layout")
    if a.host_render:
        frames = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
        rendered = viz.render(frames, backend="host", **kw)
        if objects is not None and a.object_trails is not None:
            rendered = paint_object_trails(a, rendered, objects, "host")
        packed = write_video(a.out_video, rendered, video, dev, host=True) if video else None
    else:
        on_dev = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).to(dev)
        rendered = viz.render(on_dev, backend="hip", **kw)
        if objects is not None and a.object_trails is not None:
            rendered = paint_object_trails(a, rendered, objects, "hip")
        packed = write_video(a.out_video, rendered, video, dev) if video else None       # render -> encode on the device
        rendered = rendered.cpu().numpy()
    frames = frames.cpu().numpy() if isinstance(frames, torch.Tensor) else frames
    write(a.out, rendered, a.fps)
    print(f"{a.out}: {len(rendered)} frames of {frames.shape[1]} x {frames.shape[2]} and demo.gif ({a.task}{'' if a.trails is None else f', trails of {a.trails}'}, "
          f"{'host' if a.host_render else 'hip'} renderer)")
    r = dict(frames=frames, tracks=tracks, visibles=visibles, query_points=points, ids=None if ids is None else ids.cpu().numpy(), rendered=rendered)
    if objects is not None:
        r["objects"] = objects
    if objects is not None and a.crops:
        r.update(write_crops(a, frames, ids, objects, video, dev))
    if getattr(a, "cleaned", None) is not None:
        r["clean"] = a.cleaned
        if a.cleaned["stats"] is not None:
            st = a.cleaned["stats"][:, 1:].sum((0, 1)).tolist()
            print(f"clean: {st[0]} component(s), {st[1]} kept, {st[2]} pixel(s) dropped, {st[3]} filled")
    if video:
        r.update(video=packed.numpy(), video_settings=video)
    return r


if __name__ == "__main__":
    main()
