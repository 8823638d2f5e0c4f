"""Trackers behind the reference's registry names and call contract
(mmpt/models/trackers/base.py:24-60, vanilla_tracker.py:25-412, :417-585).

`model(test_mode=True, rgbs=..., query_points=..., trajectories=..., visibilities=...)` returns the
reference's 5-tuple.  Everything after the encoder runs in libfgvc_hip.so through fgvc_amd.engine:
no feature map, label map or score slab visits the host (the reference parks features on the CPU
and re-uploads them per frame, :145-147, :347-352, and ships T*P*h*w floats back for a numpy
argsort, :404-406).
"""
from __future__ import annotations

from typing import Optional

import torch
import torch.nn as nn

from .. import engine, ops
from .builder import build_backbone, build_components
from .config import ConfigDict
from .registry import MODELS


class EncoderOverflow(RuntimeError):
    """An activation left the f16 range of its calibrated scale (ResNet.check_overflow): the pass that raised it is invalid."""


class BaseModel(nn.Module):
    """base.py:24-60: holds train_cfg/test_cfg, dispatches on test_mode."""

    def __init__(self, train_cfg=None, test_cfg=None, init_cfg=None):
        super().__init__()
        self.train_cfg = train_cfg
        self.test_cfg = test_cfg if test_cfg is not None else ConfigDict()

    def init_weights(self):
        for m in self.children():
            if hasattr(m, "init_weights"):
                m.init_weights()

    def forward_train(self, *a, **k):
        raise NotImplementedError("fgvc_amd accelerates the inference path only")

    def forward_test(self, *a, **k):
        raise NotImplementedError

    def forward(self, test_mode=False, **kwargs):
        if not test_mode:
            return self.forward_train(**kwargs)
        try:
            return self.forward_test(**kwargs)
        except EncoderOverflow:
            # The f16 arithmetic of the encoder stores activations at per-tensor scales derived from the weights (canonical frames, 2^8 of
            # headroom); a video with larger activations than that overflows them.  The check that raised has dropped the scales and
            # asked for 2^4 more headroom: run the video once more (up to three times: 2^22 in all).  The video AFTER it starts from the
            # canonical scales again -- no result depends on the videos before it.  Results are never returned from an overflowed pass.
            bb = getattr(self, "backbone", None)
            try:
                for attempt in range(3):
                    self.overflow_retries = getattr(self, "overflow_retries", 0) + 1
                    try:
                        return self.forward_test(**kwargs)
                    except EncoderOverflow:
                        if attempt == 2 or getattr(bb, "calibration", None) != "canonical":
                            raise
            finally:
                if hasattr(bb, "end_overflow_retry"):
                    bb.end_overflow_retry()


@MODELS.register_module()
class BaseTracker(BaseModel):
    def __init__(self, backbone, head=None, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.backbone = build_backbone(backbone)
        self.head = build_components(head) if head is not None else None
        self.register_buffer("iteration", torch.tensor(0, dtype=torch.float))

    def extract_feat(self, imgs):
        x = self.backbone(imgs)
        if self.head is not None:
            x = self.head(x)
        return x


_RAW_DTYPES = (torch.uint8, torch.uint16)      # what test_cfg.input converts: bytes, and the 16-bit words of a 10- to 16-bit YUV type


def _packed_desc(ic, lead: str) -> str:
    """'uint8 nv12 frames of shape (1, T, 3 h0 / 2, w0)' and its kin, for the refusals of a misshapen packed clip."""
    dt = str(engine.input_dtype(ic.type)).replace("torch.", "")
    return f"{dt} {ic.type} frames of shape ({lead}{ops._packed_shape(ic.type)[1:]}"


class LabelSession:
    """A clip encoded once, index maps propagated any number of times (model.open_label_session).  The affinity lists depend on the
    features only, so the session keeps one engine.LabelSweep per (first annotated frame, time direction): a second propagate with the
    same first frame launches no encoder, no pair kernel and no merge -- only the sweep and the read-out.  With fuse='linear' the
    backward lists are those of the LAST annotated frame: a further map between the first and the last computes no lists either.
    counters: encodes (1), affinity_runs (propagate calls that had to compute lists), sweeps (propagate calls)."""

    def __init__(self, model, imgs, img_meta):
        if imgs is None or img_meta is None:
            raise TypeError("open_label_session needs imgs and img_meta")
        model._raw_input(imgs, "imgs")
        model._refuse_occlusion("the mask call (imgs= / ref_seg_map=)")
        model._refuse_refs()
        model._refuse_readout()
        model._refuse_clean()
        if imgs.shape[0] != 1 or imgs.shape[1] != 1:
            raise NotImplementedError("fgvc_amd: the mask path runs batch size 1; call it once per video")
        if not imgs.is_cuda:
            raise RuntimeError(f"fgvc_amd.{type(model).__name__} runs on the GPU only (no CPU fallback)")
        self.model = model
        self.cfg = model._label_config()
        self.out_shape = tuple(int(v) for v in img_meta[0]["original_shape"][:2])
        frames, self.size, self.pad = model._label_frames(imgs)                               # (T, 3, hp, wp)
        self.n_frames, self.device = frames.shape[0], frames.device
        self.feats, self.Hf, self.Wf = model._label_feats(frames, index_map=True)
        # test_cfg.readout type='guided': the padded frames and their cell colours stay with the session (a later propagate encodes nothing)
        self.guide = model._readout_guide(frames, self.Hf, self.Wf)
        self.cells = None if self.guide is None else ops.guide_cells(self.guide, self.Hf, self.Wf)
        self._sweeps = {}
        self.counters = dict(encodes=1, affinity_runs=0, sweeps=0)
        self.last_disagree = None          # (T,) int64 on the host after a propagate with fuse set, else None

    def propagate(self, refs, direction=None, override=None, confidence=False, fuse=None):
        """refs: {frame index: index map (h, w) | (1, h, w)} at the network size, or one tensor for frame 0.  direction / override / fuse
        default to test_cfg.refs' (else 'forward' / 'new' / None).  Returns what the mask call returns, [masks] with masks (T, h0, w0)
        float64 on the host or the uint8 device tensor (test_cfg.masks='device'); confidence=True: (masks, conf, stats) in the same form,
        conf (T, h0, w0) uint8, stats (T, C, 2) int64 (ops.seg_readout_conf).
        fuse='linear' (with direction='both', override='all'): the frames between two annotated frames blend the forward and the backward
        sweep (engine.fuse_refs_host); the per-frame counts of cells on which the two disagree stay in self.last_disagree, and the session
        keeps the lists of (first annotated frame, 'fw') and (last annotated frame, 'bw') only."""
        self.model.last_objects = None
        self.model.last_clean = None
        if self.feats is None:
            raise RuntimeError("LabelSession: propagate after close()")
        base = self.model.refs_cfg or engine.RefsConfig()
        rc = engine.parse_refs(dict(direction=base.direction if direction is None else direction,
                                    override=base.override if override is None else override,
                                    fuse=base.fuse if fuse is None else fuse))
        maps = engine.check_ref_maps(refs, self.n_frames, self.size)
        segs = {t: torch.nn.functional.pad(m.to(self.device, torch.uint8), self.pad).contiguous() for t, m in maps.items()}
        stats, disagree = [], []
        objects = [] if self.model.objects_stats else None
        cleaned = []
        out = engine.propagate_masks_refs(self.feats, self.Hf, self.Wf, segs, self.pad, self.out_shape, self.cfg, rc,
                                          channels=self.model.feat_channels, stats_out=stats, confidence=bool(confidence),
                                          sweeps=self._sweeps, counters=self.counters, guide=self.guide,
                                          readout=self.model.readout_cfg if self.guide is not None else None, cells=self.cells,
                                          disagree_out=disagree, objects_out=objects, clean=self.model.clean_cfg, clean_out=cleaned)
        if objects:
            self.model.last_objects = engine.ObjectTracks(objects[0])
        if cleaned:
            self.model.last_clean = dict(stats=cleaned[0], config=self.model.clean_cfg)
        self.last_disagree = None
        if rc.fuse is not None:            # one annotated frame: nothing was fused, nothing disagrees
            self.last_disagree = disagree[0].cpu() if disagree else torch.zeros(self.n_frames, dtype=torch.int64)
        self.model._refine_stats = stats or None
        self.model._check_kernels()
        device = self.model.masks_form == "device"
        if not confidence:
            return [out] if device else [out.cpu().numpy().astype("float64")]
        masks, conf, st = out
        return (masks, conf, st) if device else (masks.cpu().numpy().astype("float64"), conf.cpu().numpy(), st.cpu().numpy())

    def close(self):
        """Drop the features, the cached lists and the guide."""
        self.feats, self._sweeps, self.guide, self.cells = None, {}, None, None


@MODELS.register_module()
class VanillaTracker(BaseTracker):
    """Label propagation with a dense (disc-masked) affinity and top-k softmax."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        g = self.test_cfg.get
        self.stride_sample = g("stride_sample", False)
        self.feat_channels = None          # the encoder's (un-padded) channel count, known after the first get_feats_hwc()
        self.last_cycle_error = None       # (1, T, P) f32 forward-backward errors of the last points call with test_cfg.occlusion set, else None
        self.input_cfg = engine.parse_input(self.test_cfg.get("input", None))      # test_cfg.input (None: float frames only); a bad key is refused here
        self.masks_form = engine.parse_masks(self.test_cfg.get("masks", None))     # test_cfg.masks: 'numpy' (default) | 'device'; the index-map call only
        self.chain_cfg = engine.parse_chain(self.test_cfg.get("chain", None))      # test_cfg.chain (None: the points call propagates labels, as ever)
        self.last_flow = None              # forward_test_flow's dict of the last points call with test_cfg.chain set, else None
        self.refs_cfg = engine.parse_refs(self.test_cfg.get("refs", None))         # test_cfg.refs (None: ref_seg_map is one tensor for frame 0)
        self.last_confidence = None        # dict(conf, stats, frame_score[, disagree with refs.fuse]) of the last mask call with test_cfg.refs.confidence=True, else None
        self.pose_cfg = engine.parse_pose(self.test_cfg.get("pose", None))         # test_cfg.pose (None: the coords=True call returns coordinates only)
        self.last_pose = None              # dict(peak, field) of the last coords=True call with test_cfg.pose set, else None
        self.readout_cfg = engine.parse_readout(self.test_cfg.get("readout", None))   # test_cfg.readout (None / type='bilinear': the plain read-out)
        self.objects_stats = engine.parse_objects(self.test_cfg.get("objects", None))  # test_cfg.objects = dict(stats=True); the index-map call only
        self.last_objects = None           # engine.ObjectTracks of the masks the last index-map call returned with test_cfg.objects set, else None
        self.clean_cfg = engine.parse_clean(self.test_cfg.get("clean", None))      # test_cfg.clean (None: the read-out's masks are returned as they are)
        self.last_clean = None             # dict(stats=(T, C, 4) int64 device tensor | None for a spec that changes nothing, config=CleanConfig) of the last index-map call with test_cfg.clean set, else None

    # ---- A1/A2: encoder, every frame exactly once, features stay on the device ------------------
    def extract_feat(self, imgs):
        x = self.backbone(imgs)
        if self.stride_sample:
            x = x[:, :, ::self.stride_sample, ::self.stride_sample]
        if self.head is not None:
            x = self.head(x)
        return x

    @torch.no_grad()
    def get_feats_hwc(self, frames: torch.Tensor, split: bool = False, out: Optional[torch.Tensor] = None):
        """frames (T,3,h,w) -> normalised channels-last (T, HfWf, C'), Hf, Wf.
        batch_step frames per encoder call (vanilla_tracker.py:135-147).  split=True: the bank comes back in the pair kernel's operand
        format -- (T, HfWf, 2, C') int16 in the format engine_config().pair_split_fmt names, or (T, HfWf, 4, 256) int16 = split_f16f6x()
        rows (2 KiB per pixel: the f16 + FP6 row and the exact f32 channels behind it; engine_config().bank_fmt, the default) --
        wherever the engine's split pair kernel applies (one pass less; engine.run_affinity takes either form), f32 otherwise.
        `out`: rows of the caller's own feature bank (T, ...) of the shape / dtype this call produces; the encoder then writes there
        and `out` itself is returned (clip sharding: the frames a rank encodes land in its local bank without a copy).  A mismatch
        falls back to a fresh tensor -- compare the result with `out` by identity."""
        step = int(self.test_cfg.get("batch_step", 5))
        norm = bool(self.test_cfg.get("with_norm", True))
        chunks = []
        in_place = out is not None
        Hf = Wf = None
        if self.test_cfg.get("channels_last", False):
            # MIOpen's fastest f32 kernels on gfx950 are NHWC; feeding NHWC avoids its transposes
            frames = frames.contiguous(memory_format=torch.channels_last)
        fast = (hasattr(self.backbone, "forward_hwc") and self.head is None and not self.stride_sample
                and len(getattr(self.backbone, "out_indices", ())) == 1)
        split_if = None
        split_fmt = "bf16"
        if split and fast:
            cfg = self.engine_config()
            split_fmt = cfg.bank_fmt                 # "f16f6x" (2 KiB rows: + the exact f32 channels) where the refining merge runs
            if cfg.pair_precision in ("auto", "split"):
                split_if = lambda C, H, W: ops.split_path_ok(C, H, W, cfg.topk, cfg.with_norm, None, cfg.mask,
                                                             cfg.with_first_neighbor or not cfg.with_first)
        for i in range(0, frames.shape[0], step):
            if fast:       # backbone writes normalised channels-last rows itself (no NCHW round trip)
                o = out[i:i + step] if out is not None else None
                f, Hf, Wf = self.backbone.forward_hwc(frames[i:i + step], norm, split_if=split_if, split_fmt=split_fmt, out=o)
                self.feat_channels = f.shape[-1]                      # (this path never pads)
                chunks.append(f)
                in_place = in_place and o is not None and f is o
                continue
            f = self.extract_feat(frames[i:i + step])
            if isinstance(f, (tuple, list)):
                f = f[0]
            Hf, Wf = f.shape[-2:]
            self.feat_channels = f.shape[1]                           # before the zero padding to a kernel width
            chunks.append(ops.normalize_to_hwc(f.float(), norm, pad=True))
            in_place = False
        if in_place and chunks:
            return out, Hf, Wf
        return (chunks[0] if len(chunks) == 1 else torch.cat(chunks, 0)), Hf, Wf       # (cat of one tensor is a copy)

    def engine_config(self) -> engine.TrackerConfig:
        """The test_cfg as the engine reads it.  Unless test_cfg names `pair_split_fmt` itself, the pair kernel follows the encoder's
        arithmetic: an f16f8 trunk (features +-3e-5 logit from the reference's) goes with fgvc_pair_topk_f16f6 (+-6e-5, half the matrix
        work) where that kernel applies -- every key slot masked, the mask within 64 key blocks of a query tile --, any other trunk
        (set_arith('f16x3') / 'bf16x3') with the 1e-7-grade fgvc_pair_topk_f16x3."""
        cfg = engine.TrackerConfig.from_test_cfg(self.test_cfg)
        if "pair_split_fmt" not in self.test_cfg and getattr(self.backbone, "arith", None) in ("f16f8", "f16f6"):
            all_masked = cfg.with_first_neighbor or not cfg.with_first
            if all_masked and ops.pair_blocks_reached(cfg.mask) <= ops.PAIR_F16F6_MAX_BLOCKS and cfg.topk <= 10 and cfg.with_norm:
                cfg.pair_split_fmt = "f16f6"
        return cfg

    def _check_kernels(self):
        """Fail closed, per video: the pair kernel's LDS protocol waits with bounded spins, and a workgroup whose wait gave up writes
        poison lists (NaN trajectories downstream) and raises a device flag.  The flag is read -- and cleared -- here, at the point
        where the reference synchronises anyway (`.cpu().numpy()` of the label maps, vanilla_tracker.py:404).  `check_kernels=False`
        in test_cfg (an extension key) skips the device synchronisation; the poison still marks the results."""
        if not self.test_cfg.get("check_kernels", True):
            return
        if ops.pair_f16x3_timed_out():
            raise RuntimeError("fgvc_pair_topk_f16x3: a bounded wait of the kernel's LDS protocol timed out; this video's results are invalid")
        st = getattr(self, "_refine_stats", None)
        if st is not None:
            # the refining merge assumes |fgvc_pair_topk_f16f6 score - exact| <= pair_refine_eps; every candidate it re-scores is a sample
            # of that error, and the largest one seen in this video is held against the bound (measured: 5e-6 of 2e-5)
            self._refine_stats = None
            worst, eps = max(ops.refine_max_error(s_) for s_ in st), float(self.engine_config().pair_refine_eps)
            if worst > eps:
                raise RuntimeError(f"fgvc_merge_refine_topk_f32: the pair kernel's score error reached {worst:.2e} on this video, beyond the bound "
                                   f"{eps:.2e} the exact re-scoring assumes; raise test_cfg.pair_refine_eps or set pair_split_fmt='f16'")
        if hasattr(self.backbone, "check_overflow") and self.backbone.check_overflow():
            raise EncoderOverflow("fgvc_amd ResNet: an activation left the f16 range of its calibrated scale (f16 arithmetic of the encoder); "
                               "this video's results are invalid -- the scales were dropped and the next call re-calibrates on its own "
                               "frames (or call backbone.calibrate(frames), or backbone.set_arith('bf16x3'))")

    # ---- predicted visibility: the forward-backward cycle check (test_cfg.occlusion, an extension key) ----------
    _default_neighbor_range = None         # (TrackerConfig.from_test_cfg reads neighbor_range without a default; HRVanillaTracker's is 24)

    def _occlusion(self) -> Optional[engine.OcclusionConfig]:
        """test_cfg.occlusion parsed (None: the option is off).  The default window of the fields is this tracker's own: neighbor_range // 2."""
        spec = self.test_cfg.get("occlusion", None)
        if spec is None:
            return None
        nr = self.test_cfg.get("neighbor_range", self._default_neighbor_range)
        if nr is None and dict(spec).get("radius") is None:
            raise ValueError("test_cfg.occlusion: neighbor_range is None (no window to derive the fields' from); give occlusion.radius")
        return engine.parse_occlusion(spec, 0 if nr is None else int(nr) // 2)

    def _refuse_occlusion(self, what: str):
        if self.test_cfg.get("occlusion", None) is not None:
            raise NotImplementedError(f"fgvc_amd: test_cfg.occlusion is read by the points call only (rgbs= / query_points=); {what} "
                                      "has no visibility output -- remove the key for this call")

    def _window_rows(self, feats, Hf, Wf, radius: int, key: str = "occlusion"):
        """The bank get_feats_hwc(split=True) returned, as the rows engine.run_local_affinity takes for a window of `radius`, and the
        LocalConfig of single-slot pairs on this tracker's own topk, temperature and normalisation key.  The f16 + FP6 bank gives its exact
        f32 channels (a view), a split_f16x2 bank goes in as it is where the 16-bit pair kernel takes the window, any other bank as f32
        rows.  `key`: the test_cfg key that asked, for the refusal's text."""
        cfg = self.engine_config()
        fmt = ops.bank_format(feats, cfg.bank_fmt)
        if fmt == "f16f6x":
            rows = ops.f32_of_f16f6x(feats)
        elif fmt == "f16f6":
            raise NotImplementedError(f"fgvc_amd: test_cfg.{key} needs f32-grade rows; a split_f16f6p() bank (pair_split_fmt='f16f6' with "
                                      "pair_refine=False) holds 11-bit ones -- set pair_refine=True (the default) or pair_split_fmt='f16'")
        elif fmt == "f16" and not ops.split_path_ok(feats.shape[-1], Hf, Wf, cfg.topk, cfg.with_norm, None,
                                                    ops.MaskSpec(ry=radius, rx=radius), True):
            rows = ops.unsplit_f16x2(feats)
        else:
            rows = feats
        lc = engine.LocalConfig(temperature=cfg.softmax_temperature(self.feat_channels or rows.shape[-1]), topk=int(cfg.topk),
                                precede_frames=1, radius=radius, with_first=False, with_norm=bool(cfg.with_norm),
                                pair_precision="f32" if cfg.pair_precision == "f32" else "auto",
                                pair_budget=int(self.test_cfg.get("pair_budget", engine.LOCAL_PAIR_BUDGET)))
        return rows, lc

    def _cycle_fields(self, feats, Hf, Wf, w, occ: engine.OcclusionConfig):
        """The clip's backward coordinate fields from the bank get_feats_hwc(split=True) returned (_window_rows).  Returns
        (fields (T-1, HW, 2), scale)."""
        rows, lc = self._window_rows(feats, Hf, Wf, occ.radius)
        scale = w // Wf                                                               # vanilla_tracker.py:609
        self.cycle_stats = {}
        return engine.backward_fields(rows, Hf, Wf, lc, scale, self.cycle_stats), scale

    # ---- dense optical flow between frames (test_cfg.flow, an extension key) ---------------------------------------
    def _flow(self, spec=None) -> Optional[engine.FlowConfig]:
        """test_cfg.flow (or `spec` in its place) parsed (None: the option is off).  The default window is this tracker's own:
        neighbor_range // 2."""
        spec = self.test_cfg.get("flow", None) if spec is None else spec
        if spec is None:
            return None
        nr = self.test_cfg.get("neighbor_range", self._default_neighbor_range)
        if nr is None and hasattr(spec, "keys") and dict(spec).get("radius") is None:
            raise ValueError("test_cfg.flow: neighbor_range is None (no window to derive the lists' from); give flow.radius")
        return engine.parse_flow(spec, 0 if nr is None else int(nr) // 2)

    @torch.no_grad()
    def forward_test_flow(self, imgs, img_meta=None, fc: Optional[engine.FlowConfig] = None):
        """Dense flow between the frames of a clip `step` apart, both time directions.  imgs as the label-map call takes them: float
        (1, 1, 3, T, h, w), or uint8 frames with test_cfg.input.  Returns a dict of CUDA tensors at the network size (h, w): flow_fw[g] takes
        frame g to frame g + step and flow_bw[g] back, (T-step, 2, h, w) f32 in pixels, channel 0 = x; valid_fw / valid_bw (T-step, h, w)
        uint8; with flow.occlusion set, occ_fw / occ_bw (T-step, 1, h, w) f32, 1 = consistent.  self.flow_stats: what the affinity reported.
        `fc`: a parsed configuration in test_cfg.flow's place (the chained points call's)."""
        fc = self._flow() if fc is None else fc
        if fc is None:
            raise ValueError(f"{type(self).__name__}.forward_test_flow needs test_cfg.flow = dict(type='window', ...)")
        if self.test_cfg.get("occlusion", None) is not None:
            raise ValueError("fgvc_amd: test_cfg.flow and test_cfg.occlusion are both set; the flow call has its own check "
                             "(flow.occlusion = 'consistency' | 'fb_abs') and the cycle check belongs to the points call -- remove one")
        if imgs is None:
            raise TypeError(f"{type(self).__name__}.forward_test_flow needs imgs")
        ic = self._raw_input(imgs, "imgs")
        if not imgs.is_cuda:
            raise RuntimeError(f"fgvc_amd.{type(self).__name__} runs on the GPU only (no CPU fallback)")
        if ic is None and (imgs.dim() != 6 or imgs.shape[0] != 1 or imgs.shape[1] != 1 or imgs.shape[2] != 3):
            raise ValueError(f"imgs: float frames of shape (1, 1, 3, T, h, w), got {tuple(imgs.shape)}")
        frames, (h, w), pad = self._label_frames(imgs)                                        # (T, 3, hp, wp)
        feats, Hf, Wf = self._label_feats(frames)
        hp, wp = frames.shape[-2:]
        if hp % Hf or wp % Wf or hp // Hf != wp // Wf:
            raise NotImplementedError(f"fgvc_amd: the flow read-out needs a feature cell on every `scale`-th pixel of the padded frame; {hp} x {wp} "
                                      f"over {Hf} x {Wf} features is no whole pitch -- pad the frames to the encoder's output stride "
                                      "(HRVanillaTracker: build it with stride = that stride)")
        rows, lc = self._window_rows(feats, Hf, Wf, fc.radius, "flow")
        scale = wp // Wf
        self.flow_stats = {}
        fw, bw, vfw, vbw = engine.flow_fields(rows, Hf, Wf, lc, scale, (h, w), (pad[0], pad[2]), fc.step, fc.renorm, self.flow_stats)
        out = dict(flow_fw=fw, flow_bw=bw, valid_fw=vfw, valid_bw=vbw)
        if fc.occlusion is not None:
            out["occ_fw"], out["occ_bw"] = engine.flow_occlusion(fw, bw, fc.occlusion, fc.diff)
        self._check_kernels()
        return out

    def _flow_call(self, rgbs, query_points, imgs, ref_seg_map) -> bool:
        """forward_test's third call form: imgs= alone (no first-frame labels) with test_cfg.flow set.  Without the key nothing changes."""
        return (self.test_cfg.get("flow", None) is not None and imgs is not None and ref_seg_map is None
                and rgbs is None and query_points is None)

    # ---- point tracks in both time directions by chaining the flow (test_cfg.chain, an extension key) -----------------
    @torch.no_grad()
    def forward_test_chain(self, rgbs, query_points, trajectories=None, visibilities=None):
        """The points call with test_cfg.chain set: the clip's dense flow (forward_test_flow on test_cfg.flow, else dict(type='window')), then
        every query point chained through it forward and backward in time by one kernel (engine.chain_points: the reference's
        RAFT.forward_test, raft.py:247-289).  rgbs float (1, T, 3, h, w), or uint8 frames with test_cfg.input; query_points (1, P, 3) =
        (t, x, y) in pixels of the network size.  Returns the reference's 5-tuple with the points in their given order; traj_pred
        (1, T, P, 2) is filled for all T frames, vis_pred (1, T, P) by chain.visibility.  The flows stay in self.last_flow."""
        cc = self.chain_cfg
        if self.test_cfg.get("occlusion", None) is not None:
            raise ValueError("fgvc_amd: test_cfg.chain and test_cfg.occlusion are both set; the chained call has its own visibility "
                             "(chain.visibility = 'frame' | 'consistency') and the cycle check belongs to label propagation -- remove one")
        spec = self.test_cfg.get("flow", None)
        fc = self._flow(spec if spec is not None else dict(type="window"))
        if fc.step != 1:
            raise ValueError(f"fgvc_amd: test_cfg.chain walks frame by frame; test_cfg.flow has step={fc.step} (set step=1)")
        if cc.visibility == "consistency" and fc.occlusion is None:
            fc.occlusion = "consistency"
        # packed YUV frames are (1, T, 3 h0 / 2, w0); without the key, uint8 frames of either form go on to the flow call's TypeError
        packed = rgbs.dtype in _RAW_DTYPES and (self.input_cfg is None or self.input_cfg.yuv) and rgbs.dim() == 4
        if (not packed and rgbs.dim() != 5) or rgbs.shape[0] != 1:
            raise ValueError(f"rgbs: frames of shape (1, T, 3, h, w), or uint8 ones as test_cfg.input lays them out, got {tuple(rgbs.shape)}")
        if query_points.dim() != 3 or query_points.shape[0] != 1 or query_points.shape[2] != 3:
            raise ValueError(f"query_points: (1, P, 3) = (t, x, y), got {tuple(query_points.shape)}")
        engine.check_query_times(query_points[0, :, 0], rgbs.shape[1])
        # the flow call's layout: float (1, 1, 3, T, h, w) -- a view --, uint8 (1, 1, T, ...)
        imgs = rgbs.unsqueeze(1) if rgbs.dtype in _RAW_DTYPES else rgbs.transpose(1, 2).unsqueeze(1)
        self.last_flow = flow = self.forward_test_flow(imgs, fc=fc)
        ok_fw, ok_bw = engine.chain_masks(flow) if cc.visibility == "consistency" else (None, None)
        traj, vis = engine.chain_points(flow["flow_fw"], flow["flow_bw"], query_points[0], ok_fw, ok_bw, cc.visibility)
        traj, vis = traj.unsqueeze(0), vis.unsqueeze(0)
        if trajectories is not None:
            traj = traj.to(trajectories.device, trajectories.dtype)
        vis = vis.to(visibilities.device, visibilities.dtype) if visibilities is not None else vis.to(torch.float32)
        return trajectories, visibilities, traj, vis, query_points

    def _visibility_from_frame0(self, feats, Hf, Wf, w, coords, qp, visibilities, occ):
        """The fourth return element of the un-regrouped call: every point is tracked from frame 0, whatever its query time
        (vanilla_tracker.py:302-303), so the cycle closes there; frames before a point's own query time are reported invisible.
        qp (P, 3) = (t, x, y), coords (T, P, 2).  Zeros when the option is off."""
        if occ is None:
            return torch.zeros_like(visibilities)
        T, dev = coords.shape[0], coords.device
        fields, scale = self._cycle_fields(feats, Hf, Wf, w, occ)
        v, e, _ = engine.cycle_check(fields, coords, 0, qp[:, 1:], scale, occ.cycle_thresh, Hf, Wf)
        v = v & (torch.arange(T, device=dev).view(T, 1) >= qp[:, 0].to(dev).view(1, -1))
        return self._visibility_like(visibilities, v, e)

    def _visibility_like(self, visibilities, vis_bool, err):
        """(T, P) bool / f32 -> the fourth return element (visibilities' dtype, shape and device; float32 without one) and last_cycle_error."""
        self.last_cycle_error = err.unsqueeze(0)
        v = vis_bool.unsqueeze(0)
        return v.to(visibilities.dtype).to(visibilities.device) if visibilities is not None else v.to(torch.float32)

    # ---- raw frames: test_cfg.input (an extension key) -------------------------------------------------------------
    def _raw_input(self, frames: torch.Tensor, name: str) -> Optional[engine.InputConfig]:
        """None for float frames (they run as ever, with or without the key); self.input_cfg for uint8 ones (uint16 ones where its type's
        samples are 16-bit words), TypeError without the key or for frames of another dtype than the type's."""
        if frames is None or frames.dtype not in _RAW_DTYPES:
            return None
        ic = self.input_cfg
        dt = str(frames.dtype).replace("torch.", "")
        if ic is None:
            raise TypeError(f"{type(self).__name__}: {name} is {dt}, and float frames are expected (Lab-normalised network input); raw RGB "
                            "frames are taken with the extension key test_cfg.input = dict(type='rgb8', size=(h, w) | None, "
                            "layout='thwc' | 'tchw')")
        if frames.dtype != engine.input_dtype(ic.type):
            raise TypeError(f"{type(self).__name__}: {name} is {dt}, and test_cfg.input type={ic.type!r} takes "
                            f"{str(engine.input_dtype(ic.type)).replace('torch.', '')} frames")
        if not frames.is_cuda:
            raise RuntimeError(f"fgvc_amd.{type(self).__name__} runs on the GPU only (no CPU fallback)")
        return ic

    def _points_frames(self, rgbs: torch.Tensor) -> torch.Tensor:
        """The points call's rgbs as float frames (1, T, 3, h, w): uint8 (1, T, h0, w0, 3) | (1, T, 3, h0, w0) goes through the input kernel."""
        ic = self._raw_input(rgbs, "rgbs")
        if ic is None:
            return rgbs
        if ic.yuv:
            if rgbs.dim() != 4 or rgbs.shape[0] != 1:
                raise ValueError(f"rgbs: {_packed_desc(ic, '1, ')}, got {tuple(rgbs.shape)}")
            return self._yuv_to_lab(ic, rgbs[0], "rgbs", ic.size).unsqueeze(0)
        if rgbs.dim() != 5 or rgbs.shape[0] != 1:
            raise ValueError(f"rgbs: uint8 frames of shape (1, T, h0, w0, 3) ('thwc') or (1, T, 3, h0, w0) ('tchw'), got {tuple(rgbs.shape)}")
        return ops.frames_to_lab(rgbs[0], ic.size, layout=ic.layout).unsqueeze(0)

    def _yuv_planes(self, ic, packed: torch.Tensor, name: str):
        """Packed frames of test_cfg.input's type -> their plane views (y, u, v): NV12 / I420 (T, 3 h0 / 2, w0), an ops.YUV_PIXEL_FORMATS
        type (T, 3 h0 / 2 | 2 h0 | 3 h0, w0).  A shape that is no packed frame is a ValueError that states the expected one."""
        lead = "1, " if name == "rgbs" else "1, 1, "
        nv12_i420 = ic.type in ops.YUV_FORMATS
        try:
            return (ops.yuv420_planes if nv12_i420 else ops.yuv_planes)(packed, ic.type)
        except ValueError as e:
            even = " with h0 and w0 even" if nv12_i420 else ""
            raise ValueError(f"{name}: {_packed_desc(ic, lead)}{even}, got the frames {tuple(packed.shape)} ({e})") from None

    def _planes_to_lab(self, ic, planes, size, pad=(0, 0, 0, 0)) -> torch.Tensor:
        """_yuv_planes' views -> (T, 3, hp, wp): ops.yuv_frames_to_lab for NV12 / I420, ops.yuv_planes_to_lab with the format's depth, shift
        and subsampling for an ops.YUV_PIXEL_FORMATS type."""
        fmt = ops.YUV_PIXEL_FORMATS.get(ic.type)
        if fmt is None:
            return ops.yuv_frames_to_lab(*planes, size, pad, ic.matrix, ic.range, ic.siting)
        return ops.yuv_planes_to_lab(*planes, fmt[3], fmt[4], (fmt[1], fmt[2]), size, pad, ic.matrix, ic.range, ic.siting)

    def _yuv_to_lab(self, ic, packed: torch.Tensor, name: str, size) -> torch.Tensor:
        """Packed frames of test_cfg.input's type -> the unpadded float frames (T, 3, h, w); size=None: the frames' own."""
        return self._planes_to_lab(ic, self._yuv_planes(ic, packed, name), size)

    def _label_frames(self, imgs: torch.Tensor):
        """The label-map call's imgs -> the frames padded to a multiple of _pad_unit() (T, 3, hp, wp), the network size (h, w), the pad.
        Float imgs (1, 1, 3, T, h, w): F.pad and a transposed view.  uint8 imgs (1, 1, T, h0, w0, 3) | (1, 1, T, 3, h0, w0) with test_cfg.input
        set: the input kernel writes the padded tensor itself."""
        ic = self._raw_input(imgs, "imgs")
        if ic is None:
            h, w = imgs.shape[-2:]
            _, pad = engine.pad_divide_by(h, w, self._pad_unit())
            return torch.nn.functional.pad(imgs[0, 0], pad).transpose(0, 1), (h, w), pad
        if ic.yuv:
            if imgs.dim() != 5 or imgs.shape[0] != 1 or imgs.shape[1] != 1:
                raise ValueError(f"imgs: {_packed_desc(ic, '1, 1, ')}, got {tuple(imgs.shape)}")
            planes = self._yuv_planes(ic, imgs[0, 0], "imgs")
            h, w = ic.size if ic.size is not None else tuple(planes[0].shape[1:])      # (the luma plane: the height by the format's rows)
            _, pad = engine.pad_divide_by(h, w, self._pad_unit())
            return self._planes_to_lab(ic, planes, (h, w), pad), (h, w), pad
        if imgs.dim() != 6:
            raise ValueError(f"imgs: uint8 frames of shape (1, 1, T, h0, w0, 3) ('thwc') or (1, 1, T, 3, h0, w0) ('tchw'), got {tuple(imgs.shape)}")
        v = imgs[0, 0]
        h, w = ic.size if ic.size is not None else (tuple(v.shape[1:3]) if ic.layout == "thwc" else tuple(v.shape[2:4]))
        _, pad = engine.pad_divide_by(h, w, self._pad_unit())
        return ops.frames_to_lab(v, (h, w), pad, ic.layout), (h, w), pad

    # ---- A10: regrouping by query time ----------------------------------------------------------
    @torch.no_grad()
    def forward_test(self, rgbs=None, query_points=None, trajectories=None, visibilities=None, save_image=False, save_path=None,
                     iteration=None, imgs=None, ref_seg_map=None, img_meta=None):
        """rgbs (1,T,3,h,w), query_points (1,P,3)=(t,x,y), trajectories (1,T,P,2), visibilities (1,T,P).
        Called with imgs= / ref_seg_map= / img_meta= (what BaseModel.forward(test_mode=True, **data) passes for the reference's mask
        datasets) it propagates segmentation masks instead: forward_test_seg."""
        if self._flow_call(rgbs, query_points, imgs, ref_seg_map):
            return self.forward_test_flow(imgs, img_meta)
        if self._label_call(rgbs, query_points, imgs, ref_seg_map, img_meta):
            return self.forward_test_seg(imgs, ref_seg_map, img_meta, save_image=save_image, save_path=save_path, iteration=iteration)
        if self.chain_cfg is not None:
            return self.forward_test_chain(rgbs, query_points, trajectories, visibilities)
        rgbs = self._points_frames(rgbs)
        if not rgbs.is_cuda:
            raise RuntimeError("fgvc_amd.VanillaTracker runs on the GPU only (no CPU fallback)")
        assert rgbs.shape[0] == 1, "batch size must be 1 (vanilla_tracker.py:134)"
        cfg = self.engine_config()
        if not cfg.regroup:
            # single group that starts at frame 0 regardless of the query times (vanilla_tracker.py:302-303)
            return self.forward_test_main(rgbs, query_points, trajectories, visibilities)
        occ = self._occlusion()
        self.last_cycle_error = None
        T, h, w = rgbs.shape[1], rgbs.shape[-2], rgbs.shape[-1]
        dev = rgbs.device
        qp = query_points[0]
        t_min = int(qp[:, 0].min().item())
        # frames before the earliest query time are never used by any group
        feats, Hf, Wf = self.get_feats_hwc(rgbs[0, t_min:], split=True)
        qp_rel = qp.clone()
        qp_rel[:, 0] -= t_min
        stats = []
        traj, order = engine.track_points(feats, Hf, Wf, h, w, qp_rel, cfg, channels=self.feat_channels, stats_out=stats)   # (T-t_min, P, 2) f64, regrouped
        self._refine_stats = stats or None
        order = order.to(dev)
        traj_pred = torch.zeros_like(trajectories)
        traj_pred[0, t_min:] = traj.to(traj_pred.dtype)
        vis_pred = torch.zeros_like(visibilities)
        if occ is not None:
            fields, scale = self._cycle_fields(feats, Hf, Wf, w, occ)                # once per clip, shared by every query-time group
            qo = qp_rel.detach().cpu()[order.cpu()]                                   # (one host read for every group's columns)
            v, e = engine.cycle_check_groups(fields, traj, qo[:, 0], qo[:, 1:], scale, occ.cycle_thresh, Hf, Wf)
            vis = torch.zeros((T, qp.shape[0]), device=dev, dtype=torch.bool)
            err = torch.full((T, qp.shape[0]), float("inf"), device=dev, dtype=torch.float32)
            vis[t_min:], err[t_min:] = v, e
            vis_pred = self._visibility_like(visibilities, vis, err)
        self._check_kernels()
        return (trajectories[:, :, order], visibilities[:, :, order], traj_pred, vis_pred, query_points[:, order])

    def _label_call(self, rgbs, query_points, imgs, ref_seg_map, img_meta) -> bool:
        """forward_test's two call forms: True for the label-map one (imgs= / ref_seg_map= / img_meta=), False for points; TypeError for a
        mixture of the two or a points call without its tensors."""
        name = type(self).__name__
        if imgs is not None or ref_seg_map is not None or img_meta is not None:
            if rgbs is not None or query_points is not None:
                raise TypeError(f"{name}.forward_test: give either rgbs= / query_points= (points) or imgs= / ref_seg_map= / img_meta= (masks)")
            return True
        if rgbs is None or query_points is None:
            raise TypeError(f"{name}.forward_test: missing rgbs / query_points")
        return False

    def output_stride(self) -> int:
        """The encoder's output stride d (frame size / feature size): the mask path pads the frames to a multiple of it
        (pad_divide_by), so that the feature grid is exactly the padded size / d.  (The reference's VanillaTracker has no `stride`
        attribute; HRVanillaTracker's is the one its mask path reads.)"""
        bb = self.backbone
        if not all(hasattr(bb, a) for a in ("strides", "out_indices", "conv1")):
            raise NotImplementedError(f"fgvc_amd: the mask path needs the output stride of the encoder; unknown for {type(bb).__name__}")
        d = bb.conv1.conv.stride[0] * (2 if getattr(bb, "pool", None) is not None else 1)
        for s_ in bb.strides[:max(bb.out_indices) + 1]:
            d *= s_
        return d * (int(self.stride_sample) if self.stride_sample else 1)

    @torch.no_grad()
    def forward_test_seg(self, imgs, ref_seg_map, img_meta, save_image=False, save_path=None, iteration=None, ref=None):
        """Semi-supervised video object segmentation: HRVanillaTracker.forward_test_backward_save_mem (vanilla_tracker.py:663-830) with
        VanillaTracker's dense masked affinity (:366-378).  imgs (1,1,3,T,h,w) Lab-normalised frames, ref_seg_map (1,h,w) integer ids
        (0 = background), img_meta[0]['original_shape'] = (h0, w0).  Returns a list over the batch of one ndarray (T, h0, w0) of ids
        (frame 0 = the given map, nearest-resized), as the reference does; the array is float64 here (the reference's is float32: the
        ids are small integers, exact in either)."""
        g = self.test_cfg.get
        if ref_seg_map is None or imgs is None or img_meta is None:
            raise TypeError("VanillaTracker.forward_test_seg needs imgs, ref_seg_map and img_meta")
        self._raw_input(imgs, "imgs")                      # uint8 frames: TypeError without test_cfg.input, the GPU-only rule with it
        self._refuse_occlusion("the mask / heat-map / soft-map call (imgs= / ref_seg_map=)")
        self._refuse_readout(soft=torch.is_tensor(ref_seg_map) and ref_seg_map.ndim == 4)
        self.last_objects = None
        self.last_clean = None
        self._refuse_clean()
        if self.objects_stats and (g("coords", False) or g("return_maps", False)):
            raise NotImplementedError("fgvc_amd: test_cfg.objects describes the id maps of the index-map call; coords=True / return_maps=True "
                                      "(soft labels) return none -- remove one of the keys")
        if self.refs_cfg is None and hasattr(ref_seg_map, "keys"):
            raise TypeError("ref_seg_map: a mapping {frame index: index map} is taken with the extension key test_cfg.refs = "
                            "dict(direction='forward' | 'both', override='new' | 'all'); without it ref_seg_map is frame 0's tensor")
        if self.refs_cfg is not None:
            return self._forward_test_refs(imgs, ref_seg_map, img_meta)
        return_maps = bool(g("return_maps", False))        # extension key: the propagated soft maps themselves (the reference's coords=False output)
        if return_maps and g("coords", False):
            raise ValueError("fgvc_amd: return_maps=True and coords=True ask for two read-outs of one call; set one of them")
        if return_maps and ref_seg_map.ndim != 4:
            raise NotImplementedError("fgvc_amd: return_maps=True takes soft (4-D) first-frame labels; for the per-object maps of an index map "
                                      "pass its one-hot as float labels (1, C, h, w)")
        if not return_maps and (ref_seg_map.ndim == 4) != bool(g("coords", False)):
            raise NotImplementedError("fgvc_amd: soft (4-D) first-frame labels go with coords=True only (the JHMDB / BADJA heat-map form: "
                                      "joint coordinates), and coords=True with soft labels only (img2coord asserts on an index map); "
                                      "full-resolution soft maps are not returned -- track the joints as query points instead "
                                      "(forward_test(rgbs=, query_points=, ...)) or pass coords=True")
        if g("save_np", False):
            raise NotImplementedError("fgvc_amd: save_np=True is not supported; the masks are returned (save them with numpy.save)")
        if ref_seg_map.ndim == 4:
            return self._forward_test_heatmap(imgs, ref_seg_map, img_meta, return_maps=return_maps)
        if imgs.shape[0] != 1 or imgs.shape[1] != 1 or ref_seg_map.shape[0] != 1:     # (B, clips, 3, T, h, w): :676 folds clips into B
            raise NotImplementedError("fgvc_amd: the mask path runs batch size 1; call it once per video")
        if ref_seg_map.dtype != torch.uint8:
            lo, hi = int(ref_seg_map.min()), int(ref_seg_map.max())
            if hi > 255:
                raise NotImplementedError(f"fgvc_amd: the mask path takes at most 255 object ids (largest id {hi}); split the objects "
                                          "over several calls")
            if lo < 0:
                raise ValueError(f"ref_seg_map: negative id {lo}")
        if not imgs.is_cuda:
            raise RuntimeError("fgvc_amd.VanillaTracker runs on the GPU only (no CPU fallback)")
        return self._seg_index_maps(imgs, ref_seg_map, img_meta)

    def _seg_index_maps(self, imgs, ref_seg_map, img_meta):
        """forward_test_seg past its refusals: index maps -> [ (T, h0, w0) float64 ]; with test_cfg.masks='device' (an extension key; DESIGN.md
        section 15) the uint8 CUDA tensor itself, which metrics.davis_jf(backend='hip') scores in place."""
        cfg = self._label_config()
        h0, w0 = (int(v) for v in img_meta[0]["original_shape"][:2])
        frames, _, pad = self._label_frames(imgs)                                             # (T, 3, hp, wp)
        seg = torch.nn.functional.pad(ref_seg_map[0].to(imgs.device, torch.uint8), pad).contiguous()
        feats, Hf, Wf = self._label_feats(frames, index_map=True)
        stats, self.label_stats = [], {}
        objects = [] if self.objects_stats else None
        cleaned = []
        masks = engine.propagate_masks(feats, Hf, Wf, seg, pad, (h0, w0), cfg, channels=self.feat_channels, stats_out=stats,
                                       affinity_stats=self.label_stats, guide=self._readout_guide(frames, Hf, Wf),
                                       readout=self.readout_cfg, objects_out=objects, clean=self.clean_cfg, clean_out=cleaned)
        if objects:
            self.last_objects = engine.ObjectTracks(objects[0])
        if cleaned:
            self.last_clean = dict(stats=cleaned[0], config=self.clean_cfg)
        self._refine_stats = stats or None
        self._check_kernels()
        if self.masks_form == "device":
            return [masks]
        return [masks.cpu().numpy().astype("float64")]

    def _refuse_clean(self):
        """test_cfg.clean cleans the id maps of the index-map call: refused by name with the calls that return none."""
        g = self.test_cfg.get
        if self.clean_cfg is not None and (g("coords", False) or g("return_maps", False)):
            raise NotImplementedError("fgvc_amd: test_cfg.clean cleans the id maps of the index-map call; coords=True / return_maps=True "
                                      "(soft labels) return none -- remove one of the keys")

    # ---- the edge-aware read-out: test_cfg.readout (an extension key) -------------------------------------------------
    def _refuse_readout(self, soft: bool = False):
        """What test_cfg.readout = dict(type='guided') does not cover, each refused by name before any work.  Without the key: nothing."""
        if self.readout_cfg is None:
            return
        g = self.test_cfg.get
        if g("coords", False) or g("return_maps", False) or soft:
            raise NotImplementedError("fgvc_amd: test_cfg.readout type='guided' reads out index maps only; coords=True / return_maps=True "
                                      "(soft labels) are not covered -- remove one of the keys")
        if g("save_np", False):
            raise NotImplementedError("fgvc_amd: test_cfg.readout type='guided' with save_np=True: save_np is not supported; the masks are "
                                      "returned (save them with numpy.save)")

    def _readout_guide(self, frames: torch.Tensor, Hf: int, Wf: int) -> Optional[torch.Tensor]:
        """The padded frames (T, 3, hp, wp) as the guided read-out's guide (contiguous f32), None without the key.  The feature grid has to
        divide the padded frame: HRVanillaTracker's grid is whatever its encoder makes of the frame, and is refused by name where it does not."""
        if self.readout_cfg is None:
            return None
        hp, wp = frames.shape[-2:]
        if hp % Hf or wp % Wf:
            raise NotImplementedError(f"fgvc_amd: test_cfg.readout type='guided' with {type(self).__name__}: the feature grid {Hf} x {Wf} does "
                                      f"not divide the padded frame {hp} x {wp}; use type='bilinear' or frames the grid divides")
        return frames.to(torch.float32).contiguous()

    # ---- index maps at any frame: test_cfg.refs (an extension key) ----------------------------------------------------
    def _refuse_refs(self):
        """What test_cfg.refs does not cover, each refused by name before any work."""
        g = self.test_cfg.get
        if isinstance(self._label_config(), engine.LocalConfig):
            raise NotImplementedError(f"fgvc_amd: test_cfg.refs with {type(self).__name__}: the local-window plan (plan_local_clip) has no start "
                                      "frame; annotate frame 0 and remove the key, or use VanillaTracker")
        if g("coords", False) or g("return_maps", False):
            raise NotImplementedError("fgvc_amd: test_cfg.refs takes index maps only; coords=True / return_maps=True (soft labels) start at "
                                      "frame 0 -- remove one of the keys")
        if g("save_np", False):
            raise NotImplementedError("fgvc_amd: save_np=True is not supported; the masks are returned (save them with numpy.save)")

    def open_label_session(self, imgs, img_meta):
        """Encode the clip once for any number of mask propagations: LabelSession.  imgs / img_meta as the mask call takes them (float
        frames, or raw ones with test_cfg.input)."""
        return LabelSession(self, imgs, img_meta)

    def _forward_test_refs(self, imgs, ref_seg_map, img_meta):
        """The index-map call with test_cfg.refs set: one LabelSession, one propagate.  Returns [masks] as the call without the key does;
        with refs.confidence=True the confidence bytes, statistics and frame scores stay in self.last_confidence, with refs.fuse set the
        session's disagreement counts too ('disagree')."""
        rc = self.refs_cfg
        self.last_confidence = None
        session = LabelSession(self, imgs, img_meta)
        try:
            out = session.propagate(ref_seg_map, confidence=rc.confidence)
        finally:
            session.close()
        if not rc.confidence:
            return out
        masks, conf, stats = out
        self.last_confidence = dict(conf=conf, stats=stats, frame_score=engine.frame_scores(torch.as_tensor(stats), session.out_shape))
        if rc.fuse is not None:
            self.last_confidence["disagree"] = session.last_disagree
        return [masks]

    def _forward_test_heatmap(self, imgs, heat, img_meta, return_maps=False):
        """forward_test_seg with soft first-frame labels and test_cfg.coords=True (the JHMDB / BADJA heat-map form): heat (1, K, hm, wm)
        float32 | float64, padded by its OWN pad_divide_by (vanilla_tracker.py:672).  Returns a list over the batch of one ndarray
        (2, K, T) float64 = img2coord of the propagated maps at img_meta[0]['original_shape'] (:814-818).  Frame 0 is the padded map
        resized to that shape, NOT unpadded (:712-716): the reference's quirk, kept.
        return_maps (test_cfg.return_maps=True instead of coords): the maps themselves, one ndarray (T, K, h0, w0) in heat's dtype
        (:800-803, :826-831)."""
        if self._label_config().hard_prop:
            raise NotImplementedError("fgvc_amd: hard_prop=True with soft labels (the reference's F.one_hot without num_classes drops the last "
                                      "channel when it never wins, and the next frame's cat then fails, vanilla_tracker.py:762-768)")
        if imgs.shape[0] != 1 or imgs.shape[1] != 1 or heat.shape[0] != 1:
            raise NotImplementedError("fgvc_amd: the heat-map path runs batch size 1; call it once per video")
        if heat.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"ref_seg_map: soft labels must be float32 or float64, got {heat.dtype}")
        K = heat.shape[1]
        if not 1 <= K <= 256:
            raise NotImplementedError(f"fgvc_amd: the heat-map path takes 1 to 256 joints (got {K})")
        if not imgs.is_cuda:
            raise RuntimeError("fgvc_amd.VanillaTracker runs on the GPU only (no CPU fallback)")
        heat = heat[0].to(imgs.device).contiguous()
        if not bool(torch.isfinite(heat).all()):
            raise ValueError("ref_seg_map: the soft labels hold a non-finite value")
        return self._seg_softmaps(imgs, heat, img_meta) if return_maps else self._seg_heatmaps(imgs, heat, img_meta)

    # The label-map methods below are shared with HRVanillaTracker, which overrides these three hooks only.  After a call `label_stats` holds
    # what the affinity reported (the local window's route, chunks and workspace_bytes; nothing on the dense one) and `_refine_stats` the
    # refining merge's counters (dense only) until _check_kernels reads them.
    def _label_config(self):
        """The configuration the label-map path propagates with (its `hard_prop` is read before the heat-map path's other checks); its type
        names the engine's affinity."""
        return self.engine_config()

    def _pad_unit(self) -> int:
        """What frames and maps are padded to a multiple of (pad_divide_by): here the encoder's output stride, so that the feature grid is
        exactly the padded size / d."""
        return self.output_stride()

    def _label_feats(self, frames: torch.Tensor, index_map: bool = False):
        """frames (T,3,hp,wp) padded -> the bank engine.run_affinity takes, Hf, Wf.  index_map: the index-map read-out needs the feature
        grid to be the padded frame / d."""
        feats, Hf, Wf = self.get_feats_hwc(frames, split=True)
        if index_map:
            d, (hp, wp) = self._pad_unit(), frames.shape[-2:]
            if (Hf * d, Wf * d) != (hp, wp):
                raise RuntimeError(f"fgvc_amd: features {Hf}x{Wf} are not the padded frame {hp}x{wp} / {d}")
        return feats, Hf, Wf

    def _heat_inputs(self, imgs, heat, img_meta):
        """Frames and map each padded by its own pad_divide_by with _pad_unit() (:671-672): the padded frames (T, 3, hp, wp), the map's pad,
        (h0, w0)."""
        h0, w0 = (int(v) for v in img_meta[0]["original_shape"][:2])
        _, map_pad = engine.pad_divide_by(heat.shape[1], heat.shape[2], self._pad_unit())
        frames, _, _ = self._label_frames(imgs)                                               # (T, 3, hp, wp)
        return frames, map_pad, (h0, w0)

    def _seg_heatmaps(self, imgs, heat, img_meta):
        """_forward_test_heatmap past its refusals: heat (K, hm, wm) on the device -> [ (2, K, T) float64 ]."""
        cfg = self._label_config()
        frames, map_pad, out_shape = self._heat_inputs(imgs, heat, img_meta)
        feats, Hf, Wf = self._label_feats(frames)
        stats, self.label_stats = [], {}
        pose, self.last_pose = self.pose_cfg, None
        field = [] if pose is not None and pose.keep_field else None
        coords = engine.propagate_heatmaps(feats, Hf, Wf, heat, map_pad, out_shape, cfg, channels=self.feat_channels, stats_out=stats,
                                           affinity_stats=self.label_stats, peak=pose is not None and pose.confidence, field_out=field)
        self._refine_stats = stats or None
        self._check_kernels()
        if pose is not None:
            peak = None
            if pose.confidence:
                coords, peak = coords
                peak = peak.cpu().numpy()
            self.last_pose = dict(peak=peak, field=field[0] if field else None)
        return [coords.cpu().numpy()]

    def _maps_budget(self) -> int:
        return int(self.test_cfg.get("maps_budget", engine.MAPS_BUDGET))

    def _seg_softmaps(self, imgs, heat, img_meta):
        """_forward_test_heatmap(return_maps=True) past its refusals -> [ (T, K, h0, w0) in heat's dtype ].  The bank is propagated once;
        the read-out goes to the host in chunks of at most test_cfg.maps_budget bytes of device memory (engine.softmaps_to_host)."""
        cfg = self._label_config()
        frames, map_pad, out_shape = self._heat_inputs(imgs, heat, img_meta)
        engine.plan_map_chunks(frames.shape[0], heat.shape[0], out_shape, heat.element_size(), self._maps_budget())   # refuse before any work
        feats, Hf, Wf = self._label_feats(frames)
        stats, self.label_stats = [], {}
        bank, _ = engine.propagate_soft_bank(feats, Hf, Wf, heat, map_pad, cfg, channels=self.feat_channels, stats_out=stats,
                                             affinity_stats=self.label_stats)
        self._refine_stats = stats or None
        maps = engine.softmaps_to_host(bank, heat, Hf, Wf, map_pad, out_shape, self._maps_budget())
        self._check_kernels()
        return [maps]

    @torch.no_grad()
    def forward_test_main(self, rgbs, query_points, trajectories, visibilities):
        """vanilla_tracker.py:305-412: all points are propagated from frame 0 of `rgbs`."""
        cfg = self.engine_config()
        occ = self._occlusion()
        self.last_cycle_error = None
        T, h, w = rgbs.shape[1], rgbs.shape[-2], rgbs.shape[-1]
        feats, Hf, Wf = self.get_feats_hwc(rgbs[0], split=True)
        plan = engine.plan_clip(T, [0], cfg)
        tk = engine.run_affinity(feats, Hf, Wf, plan, cfg, channels=self.feat_channels)
        self._refine_stats = [tk.refine_stats] if tk.refine_stats is not None else None
        pts = query_points[0, :, 1:].to(rgbs.device, torch.float32)
        _, coords = engine.run_propagation(tk, 0, pts, Hf, Wf, h, w, cfg)
        vis_pred = self._visibility_from_frame0(feats, Hf, Wf, w, coords, query_points[0], visibilities, occ)
        self._check_kernels()
        return trajectories, visibilities, coords.unsqueeze(0), vis_pred, query_points


@MODELS.register_module()
class HRVanillaTracker(VanillaTracker):
    """Single-scale local-window variant (vanilla_tracker.py:417-660): mmcv.ops.Correlation(max_displacement=R)
    + F.unfold + top-k is one call to fgvc_local_corr_topk_{f16x3,f32} per frame.

    Keys read here exactly as the reference reads them: `neighbor_range` (default 24, -> R), `withnorm` (sic, :437; NOT
    `with_norm`), `topk` (10), `temperature` (default 1, :563), `precede_frames`, `with_first` (slot 0, default True, :534;
    regrouping, default False, :246), `batch_step`.  `dilations` is passed by the reference as the dilation of the
    Correlation KERNEL (:426-428), which has a single tap (kernel_size=1): any value gives the same result, so it is accepted
    and has no effect (mmcv arithmetic: "parity unpinned").  `save_mem=True` (:432, :537-545: one key frame, the previous one, and no
    first-frame slot) runs as in the reference for `precede_frames = 1` and is refused otherwise (the reference's branch then pairs one
    key frame with several label maps and fails at its reshape, :552)."""

    def __init__(self, stride=2, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.stride = stride
        g = self.test_cfg.get
        self.infer_radius = g("neighbor_range", 24) // 2
        self.infer_dilations = g("dilations", 1)
        self.grid_size_hr = 2 * self.infer_radius + 1
        self._default_neighbor_range = 24                                # (the occlusion fields' default window = infer_radius)
        self.save_mem = bool(g("save_mem", False))                      # :432
        if self.save_mem and int(g("precede_frames", 5)) != 1:
            raise NotImplementedError("fgvc_amd: HRVanillaTracker save_mem=True needs precede_frames = 1: the reference's branch pairs ONE key "
                                      "frame with the label maps of all preceding frames (vanilla_tracker.py:520-545) and fails at its "
                                      "reshape (:552) for any other value")

    def _feats_hwc(self, frames: torch.Tensor):
        """frames (T,3,h,w) -> channels-last rows (T, HfWf, C'), L2-normalised iff `withnorm` (:437-439), Hf, Wf."""
        step = int(self.test_cfg.get("batch_step", 5))
        norm = bool(self.test_cfg.get("withnorm", True))
        chunks = []
        for i in range(0, frames.shape[0], step):
            f = self.extract_feat(frames[i:i + step])
            if isinstance(f, (tuple, list)):
                f = f[0]
            Hf, Wf = f.shape[-2:]
            chunks.append(ops.normalize_to_hwc(f.float(), norm, pad=True))
        return (chunks[0] if len(chunks) == 1 else torch.cat(chunks, 0)), Hf, Wf, norm

    def _sweep(self, feats, Hf, Wf, norm, h, w, pts):
        """Labels + read-out for the points `pts` (P,2)=(x,y) given at the first frame of the bank `feats` (T,HW,C')."""
        g = self.test_cfg.get
        T, dev, P = feats.shape[0], feats.device, pts.shape[0]
        labels = torch.zeros((T, Hf * Wf, P), device=dev)
        ops.gaussian_labels(pts, Hf, Wf, h // Hf, 6.0, out=labels[0])
        R, k, tau = self.infer_radius, int(g("topk", 10)), float(g("temperature", 1))
        pre, with_first = int(g("precede_frames", 5)), bool(g("with_first", True))
        for f in range(1, T):
            # save_mem (:537-545): the single key frame f - 1 (features re-extracted there, the same values here), no first-frame slot
            ks = [f - 1] if self.save_mem else engine.key_slots(f, 0, pre, with_first)
            # `normalized` must be the flag that controlled the normalisation of the bank: the bf16-pipe kernel's fixed-point
            # keys assume |q.k| <= 1 and raw ResNet dot products are not (they go through fgvc_local_corr_topk_f32)
            idx, _, weight = ops.local_corr_topk(feats[f:f + 1], feats[ks], Hf, Wf, R, k, tau, normalized=norm)
            ops.propagate_topk(labels, torch.tensor(ks, dtype=torch.int32, device=dev), idx, weight, Hf, Wf, Hf, Wf,
                               window_L=2 * R + 1, out=labels[f])
        return ops.softargmax_top5(labels, Hf, Wf, h, w, gauss_points=pts)

    @torch.no_grad()
    def forward_test_main(self, rgbs, query_points, trajectories, visibilities):
        """"backward warping" (:492-585): labels of frame f = top-k softmax over the (2R+1)^2 windows of its key slots."""
        h, w = rgbs.shape[-2], rgbs.shape[-1]
        occ = self._occlusion()
        self.last_cycle_error = None
        feats, Hf, Wf, norm = self._feats_hwc(rgbs[0])
        pts = query_points[0, :, 1:].to(rgbs.device, torch.float32)
        coords = self._sweep(feats, Hf, Wf, norm, h, w, pts)
        vis = torch.zeros_like(visibilities) if visibilities is not None else None
        if occ is not None:
            fields, scale = self._cycle_fields(feats, Hf, Wf, w, occ, norm)
            v, e, _ = engine.cycle_check(fields, coords, 0, pts, scale, occ.cycle_thresh, Hf, Wf)
            vis = self._visibility_like(visibilities, v, e)
        self._check_kernels()
        return trajectories, visibilities, coords.unsqueeze(0), vis, query_points

    def _cycle_fields(self, feats, Hf, Wf, w, occ: engine.OcclusionConfig, norm: bool = True):
        """The clip's backward coordinate fields from _feats_hwc's f32 rows, with the keys get_coord reads (`topk`, `temperature`, `withnorm`):
        fields[g - 1] is _coord_field(frame g, frame g - 1) for every g in chunked launches.  Returns (fields (T-1, HW, 2), scale)."""
        g = self.test_cfg.get
        pp = g("pair_precision", "auto")
        lc = engine.LocalConfig(temperature=float(g("temperature", 1)), topk=int(g("topk", 10)), precede_frames=1, radius=occ.radius,
                                with_first=False, with_norm=bool(norm), pair_precision="f32" if pp == "f32" else "auto",
                                pair_budget=int(g("pair_budget", engine.LOCAL_PAIR_BUDGET)))
        scale = w // Wf                                                                # :609
        self.cycle_stats = {}
        return engine.backward_fields(feats, Hf, Wf, lc, scale, self.cycle_stats), scale

    def _coord_field(self, qrow, krow, H, W, scale, norm):
        idx, _, weight = ops.local_corr_topk(qrow, krow, H, W, self.infer_radius, int(self.test_cfg.get("topk", 10)),
                                             float(self.test_cfg.get("temperature", 1)), normalized=norm)
        return ops.topk_coord(idx, weight, H, W, self.infer_radius, scale).t().reshape(1, 2, H, W)

    @torch.no_grad()
    def get_coord(self, query_feat, key_feats, shape, scale):
        """vanilla_tracker.py:445-488: dense forward-warping field.  query_feat (1,C,H,W), key_feats (1,C,H,W) ->
        (1,2,H,W) expected (x,y) image coordinate of each query pixel's match in the key frame."""
        norm = bool(self.test_cfg.get("withnorm", True))
        H, W = query_feat.shape[-2:]
        qf = ops.normalize_to_hwc(query_feat.float(), norm, pad=True)
        kf = ops.normalize_to_hwc(key_feats.float(), norm, pad=True)
        return self._coord_field(qf, kf[:1], H, W, scale, norm)

    @torch.no_grad()
    def forward_test_forward(self, imgs, ref_seg_map=None, img_meta=None, ref=None, save_image=False, save_path=None,
                             iteration=None):
        """"forward warping" (vanilla_tracker.py:591-660): push the points `ref` (B,2,P) = rows (y,x) through the chain of
        frame-to-frame coordinate fields (query = frame max(0, f - precede_frames), key = frame f).  imgs (B,1,3,T,h,w).
        Returns what the reference returns: a list over the batch of float64 numpy arrays (2,P,T), rows (x,y)."""
        from .common import bilinear_sample
        self._refuse_occlusion("forward_test_forward (forward warping)")
        ic = self._raw_input(imgs, "imgs")
        if ic is not None and ic.yuv:                                                  # uint8 (1, 1, T, 3 h0 / 2, w0): packed NV12 / I420
            if imgs.dim() != 5 or imgs.shape[0] != 1 or imgs.shape[1] != 1:
                raise ValueError(f"imgs: {_packed_desc(ic, '1, 1, ')}, got {tuple(imgs.shape)}")
            frames = self._yuv_to_lab(ic, imgs[0, 0], "imgs", ic.size)                 # (T, 3, h, w)
        elif ic is not None:                                                           # uint8 (B, 1, T, h0, w0, 3) | (B, 1, T, 3, h0, w0): test_cfg.input
            assert imgs.dim() == 6 and imgs.shape[0] * imgs.shape[1] == 1, "batch size must be 1 (get_feats, vanilla_tracker.py:134)"
            frames = ops.frames_to_lab(imgs[0, 0], ic.size, layout=ic.layout)         # (T, 3, h, w)
        else:
            imgs = imgs.reshape((-1,) + imgs.shape[2:])                                # :599
            assert imgs.shape[0] == 1, "batch size must be 1 (get_feats, vanilla_tracker.py:134)"
            frames = imgs[0].transpose(0, 1)
        T, (h, w) = frames.shape[0], frames.shape[-2:]
        feats, Hf, Wf, norm = self._feats_hwc(frames)
        scale = w // Wf                                                                # :609
        coord = torch.flip(ref, (1,)).float()                                          # :611 (B,2,P) -> rows (x,y)
        coords = [coord]
        pre = int(self.test_cfg.get("precede_frames", 5))
        for f in range(1, T):
            start = max(0, f - pre)
            field = self._coord_field(feats[start:start + 1], feats[f:f + 1], Hf, Wf, scale, norm)
            coord = bilinear_sample(field, coord.clone().unsqueeze(-1) / scale, align_corners=True).squeeze(-1)   # :639
            coords.append(coord)
        return list(torch.stack(coords, -1).cpu().numpy().astype(float))              # :642-660

    # ---- label maps: forward_test_backward_save_mem (vanilla_tracker.py:663-830) on the local window ----------------------------------
    def _label_config(self) -> engine.LocalConfig:
        """The keys forward_test_backward_save_mem reads, as it reads them: `temperature`, `topk`, `precede_frames` as attributes with no
        default (:728, :754-755: a config without one raises), `with_norm` (:758, default True; the points path's `withnorm` is not read),
        `with_first` (:742, default True), R = neighbor_range // 2 (constructor).  `sstep` / `tstep` (:756-757), `step`, `mask_mode` and
        `with_first_neighbor` are accepted and change nothing.  hard_prop / norm_mask as VanillaTracker's mask path reads them;
        pair_precision ("auto" | "f32" | "split") and pair_budget (bytes of pair lists at once) are extension keys."""
        tc = self.test_cfg if isinstance(self.test_cfg, ConfigDict) else ConfigDict(self.test_cfg)      # (a plain dict: the same keys)
        g = tc.get
        return engine.LocalConfig(temperature=float(tc.temperature), topk=int(tc.topk), precede_frames=int(tc.precede_frames),
                                  radius=int(self.infer_radius), with_first=bool(g("with_first", True)), with_norm=bool(g("with_norm", True)),
                                  hard_prop=bool(g("hard_prop", False)), norm_mask=bool(g("norm_mask", True)),
                                  pair_precision=g("pair_precision", "auto"), pair_budget=int(g("pair_budget", engine.LOCAL_PAIR_BUDGET)))

    def _label_feats(self, frames: torch.Tensor, index_map: bool = False):
        """frames (T,3,hp,wp) padded -> f32 rows (T, HfWf, C'), L2-normalised iff `with_norm`, Hf, Wf: every frame encoded once (the reference
        re-encodes the key frames at every query frame, local_attention.py:918, :947: the same features)."""
        if self.head is not None or self.stride_sample:
            raise NotImplementedError("fgvc_amd: HRVanillaTracker's label maps are encoded by the backbone alone (feat_extractor=self.backbone, "
                                      "vanilla_tracker.py:753); a head or stride_sample is not supported there")
        return self.get_feats_hwc(frames, split=False)

    def _window_rows(self, feats, Hf, Wf, radius: int, key: str = "flow"):
        """_label_feats' f32 rows as they are, and the LocalConfig of single-slot pairs on the keys the label-map path reads
        (_label_config: `temperature`, `topk`, `with_norm`).  (The points call's cycle check has its own: _cycle_fields.)"""
        c = self._label_config()
        return feats, engine.LocalConfig(temperature=c.temperature, topk=c.topk, precede_frames=1, radius=radius, with_first=False,
                                         with_norm=c.with_norm, pair_precision="f32" if c.pair_precision == "f32" else "auto",
                                         pair_budget=c.pair_budget)

    def _pad_unit(self) -> int:
        """The tracker's own `stride` (vanilla_tracker.py:671-672), not the encoder's output stride; the feature grid is whatever the encoder
        makes of the padded frame."""
        return self.stride

    @torch.no_grad()
    def forward_test(self, rgbs=None, query_points=None, trajectories=None, visibilities=None, save_image=False, save_path=None,
                     iteration=None, imgs=None, ref_seg_map=None, img_meta=None, **kw):
        """Points: rgbs / query_points / trajectories / visibilities (below).  Label maps (imgs= / ref_seg_map= / img_meta=, what the
        reference's mask and pose datasets pass): forward_test_seg, on this tracker's local-window affinity."""
        if self._flow_call(rgbs, query_points, imgs, ref_seg_map):
            return self.forward_test_flow(imgs, img_meta)
        if self._label_call(rgbs, query_points, imgs, ref_seg_map, img_meta):
            return self.forward_test_seg(imgs, ref_seg_map, img_meta, save_image=save_image, save_path=save_path, iteration=iteration)
        if self.chain_cfg is not None:
            return self.forward_test_chain(rgbs, query_points, trajectories, visibilities)
        rgbs = self._points_frames(rgbs)
        if not self.test_cfg.get("with_first", False):
            return self.forward_test_main(rgbs, query_points, trajectories, visibilities)
        # inherited regrouping (vanilla_tracker.py:246-299): one sweep per distinct query time over the tail of the clip; the
        # frames are encoded ONCE (the reference re-encodes rgbs[:, t:] per group, :284 -- same features)
        h, w = rgbs.shape[-2], rgbs.shape[-1]
        occ = self._occlusion()
        self.last_cycle_error = None
        times = query_points[0, :, 0].to(torch.int64)
        t_min = int(times.min())
        feats, Hf, Wf, norm = self._feats_hwc(rgbs[0, t_min:])
        order, col = [], 0
        traj_pred = torch.zeros_like(trajectories)
        T, P = rgbs.shape[1], query_points.shape[1]
        if occ is not None:
            fields, scale = self._cycle_fields(feats, Hf, Wf, w, occ, norm)            # once per clip, shared by every query-time group
            vis = torch.zeros((T, P), device=rgbs.device, dtype=torch.bool)
            err = torch.full((T, P), float("inf"), device=rgbs.device, dtype=torch.float32)
        for t in sorted(set(times.tolist())):
            sel = (times == t).nonzero().flatten()
            pts = query_points[0, sel, 1:].to(rgbs.device, torch.float32)
            coords = self._sweep(feats[t - t_min:], Hf, Wf, norm, h, w, pts)
            traj_pred[0, t:, col:col + sel.numel()] = coords.to(traj_pred.dtype)
            if occ is not None:
                v, e, _ = engine.cycle_check(fields, coords, t - t_min, pts, scale, occ.cycle_thresh, Hf, Wf)
                vis[t:, col:col + sel.numel()], err[t:, col:col + sel.numel()] = v, e
            order.extend(sel.tolist())
            col += sel.numel()
        order = torch.tensor(order, device=rgbs.device)
        vis_pred = self._visibility_like(visibilities, vis, err) if occ is not None else torch.zeros_like(visibilities)
        self._check_kernels()
        return (trajectories[:, :, order], visibilities[:, :, order], traj_pred, vis_pred, query_points[:, order])
