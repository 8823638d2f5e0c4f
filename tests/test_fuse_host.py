"""CPU tests of the fused forward / backward label sweeps (test_cfg.refs fuse='linear'): the key and its refusals, the rule
(engine.fuse_refs_host) on hand-made lists, next_frame_to_annotate_by, what the GPU tests can decide (from the oracle's lists and the
float64 restatements alone), the C surface and argument refusals of the fuse kernel, and its code-object notes."""
import importlib.util
import os
import re
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

from tests import fuse_cases as FC
from tests import refs_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the key ------------------------------------------------------------------------------------------------------------------------------
def test_parse_refs_takes_fuse_and_refuses_by_name():
    from fgvc_amd import engine
    rc = engine.parse_refs(dict(direction="both", override="all", fuse="linear"))
    assert rc == engine.RefsConfig("both", "all", False, "linear") and rc.fuse == "linear"
    assert engine.parse_refs(dict(direction="both", override="all", confidence=True)) == engine.RefsConfig("both", "all", True)
    assert engine.parse_refs(dict(fuse=None)) == engine.RefsConfig("forward", "new", False) and engine.RefsConfig().fuse is None
    with pytest.raises(ValueError, match="fuse='linear'.*direction.*override"):
        engine.parse_refs(dict(direction="forward", override="all", fuse="linear"))
    with pytest.raises(ValueError, match="fuse='linear'.*direction.*override"):
        engine.parse_refs(dict(direction="both", override="new", fuse="linear"))
    with pytest.raises(ValueError, match="fuse='cubic'"):
        engine.parse_refs(dict(direction="both", override="all", fuse="cubic"))
    with pytest.raises(ValueError, match="unknown key.*frames.*fuse"):
        engine.parse_refs(dict(frames=3))


def test_tracker_reads_the_key_and_keeps_its_refusals():
    import fgvc_amd.mmpt_api as api
    from fgvc_amd import engine

    def model(typ, **test_cfg):
        cfg = dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True)
        cfg.update(test_cfg)
        return api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,),
                                                            pool_type="none")), test_cfg=cfg)

    spec = dict(direction="both", override="all", fuse="linear")
    assert model("VanillaTracker", refs=spec).refs_cfg == engine.RefsConfig("both", "all", False, "linear")
    with pytest.raises(ValueError, match="fuse"):
        model("VanillaTracker", refs=dict(fuse="linear"))
    imgs, meta = torch.zeros(1, 1, 3, 4, 16, 16), [dict(original_shape=(16, 16))]
    refs = {0: torch.zeros(16, 16, dtype=torch.uint8), 3: torch.zeros(16, 16, dtype=torch.uint8)}
    with pytest.raises(NotImplementedError, match="test_cfg.refs"):
        model("HRVanillaTracker", refs=spec)(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    for key in ("coords", "return_maps"):
        with pytest.raises(NotImplementedError, match="test_cfg.refs"):
            model("VanillaTracker", refs=spec, **{key: True})(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)


# ---- the rule on hand-made lists: 4 cells, k = 1, one key slot (the previous frame), as test_refs_host._shift_lists ------------------------
def _shift_lists(n, HW=4, step=1):
    """Sub-clip lists that copy cell p of frame j - 1 to cell (p + step) % HW of frame j."""
    idx = torch.tensor([[(p - step) % HW] for p in range(HW)])
    return SimpleNamespace(slot_frame=torch.arange(n - 1).view(-1, 1), idx=idx[None].repeat(n - 1, 1, 1),
                           weight=torch.ones(n - 1, HW, 1, dtype=torch.float64))


def _onehot(ids, C):
    return F.one_hot(torch.tensor(ids), C).double()


def test_fuse_weights_at_a_gap_of_three():
    from fgvc_amd import engine
    T = 5
    # frames 0 and 3 annotated; the forward lists move the object one cell up per frame, the backward lists keep it in place, so the two
    # passes disagree about where it is at frames 1 and 2
    small = {0: torch.tensor([1, 0, 0, 0]), 3: torch.tensor([0, 0, 0, 1])}
    rows, dis = engine.fuse_refs_host(small, T, fw=_shift_lists(T), bw=_shift_lists(4, step=0))
    assert rows.shape == (T, 4, 2) and rows.dtype == torch.float64 and dis.dtype == torch.int64 and dis.shape == (T,)
    f1, f2, b = _onehot([0, 1, 0, 0], 2), _onehot([0, 0, 1, 0], 2), _onehot([0, 0, 0, 1], 2)
    assert torch.equal(rows[1], (2 / 3) * f1 + (1.0 - 2 / 3) * b)                    # w = (3 - 1) / 3
    assert torch.equal(rows[2], (1 / 3) * f2 + (1.0 - 1 / 3) * b)                    # w = (3 - 2) / 3
    assert rows[1].argmax(-1).tolist() == [0, 1, 0, 0] and rows[2].argmax(-1).tolist() == [0, 0, 0, 1]   # the nearer annotation wins
    assert torch.equal(rows[0], _onehot([1, 0, 0, 0], 2)) and torch.equal(rows[3], _onehot([0, 0, 0, 1], 2))   # annotated: their maps
    assert dis.tolist() == [0, 2, 2, 0, 0]                                          # cells 1 and 3, then cells 2 and 3
    # beyond s_m: the forward rule alone
    fwd = engine.sweep_refs_host(small, T, fw=_shift_lists(T), direction="forward", override="all")
    assert torch.equal(rows[3:], fwd[3:]) and rows[4].argmax(-1).tolist() == [1, 0, 0, 0]


def test_fuse_midpoint_tie_goes_to_the_lower_id_and_frames_before_s0_are_backward():
    from fgvc_amd import engine
    T = 6
    # frames 1 and 5: a gap of 4, its midpoint frame 3 has w = 1 / 2.  Forward: id 2 travels from cell 0 one cell per frame; backward: id 1
    # stays at cell 2.  At frame 3 cell 2 holds id 2 in the forward pass and id 1 in the backward pass: an exact tie.
    small = {1: torch.tensor([2, 0, 0, 0]), 5: torch.tensor([0, 0, 1, 0])}
    rows, dis = engine.fuse_refs_host(small, T, fw=_shift_lists(T - 1), bw=_shift_lists(6, step=0))
    assert rows.shape == (T, 4, 3)
    assert torch.equal(rows[3][2], torch.tensor([0.0, 0.5, 0.5], dtype=torch.float64))
    assert int(rows[3].argmax(-1)[2]) == 1                                          # the first maximum: the lower id
    assert dis.tolist() == [0, 0, 2, 1, 2, 0]        # frame 2: cells 1, 2; frame 3: cell 2 (2 against 1); frame 4: cells 2, 3
    # frame 0 lies before s_0: the backward pass alone, which took frame 1's map on its way (id 2 at cell 0), not the forward rule's
    # background
    assert torch.equal(rows[0], _onehot([2, 0, 0, 0], 3))
    assert torch.equal(rows[1], _onehot([2, 0, 0, 0], 3)) and torch.equal(rows[5], _onehot([0, 0, 1, 0], 3))


def test_fuse_hard_prop_fuses_the_soft_rows():
    from fgvc_amd import engine
    T = 4
    fw, bw = _shift_lists(T), _shift_lists(T, step=0)
    fw.weight = torch.full((T - 1, 4, 1), 0.5, dtype=torch.float64)                   # soft forward rows: 0.5 x the (hard) bank's row
    small = {0: torch.tensor([1, 0, 0, 0]), 3: torch.tensor([0, 0, 1, 0])}
    rows, _ = engine.fuse_refs_host(small, T, fw=fw, bw=bw, hard_prop=True)
    # frame 2: the forward bank of frame 1 is hard (a one-hot), so the soft row is 0.5 x one-hot -- not 0.25 x as without hard_prop
    want = (1 / 3) * 0.5 * _onehot([0, 0, 1, 0], 2) + (1.0 - 1 / 3) * _onehot([0, 0, 1, 0], 2)
    assert torch.equal(rows[2], want)
    soft, _ = engine.fuse_refs_host(small, T, fw=fw, bw=bw, hard_prop=False)
    assert torch.equal(soft[2], (1 / 3) * 0.25 * _onehot([0, 0, 1, 0], 2) + (1.0 - 1 / 3) * _onehot([0, 0, 1, 0], 2))


def test_fuse_with_one_annotated_frame_is_direction_both():
    from fgvc_amd import engine
    T, s0 = 5, 3
    small = {3: torch.tensor([0, 2, 0, 0])}
    fw, bw = _shift_lists(T - s0), _shift_lists(s0 + 1)
    rows, dis = engine.fuse_refs_host(small, T, fw=fw, bw=bw)
    assert torch.equal(rows, engine.sweep_refs_host(small, T, fw=fw, bw=bw, direction="both", override="all"))
    assert dis.tolist() == [0] * T


def test_next_frame_to_annotate_by():
    from fgvc_amd import engine
    assert engine.next_frame_to_annotate_by([0, 7, 9, 9, 0], [0, 4]) == 2             # the lowest index among equals
    assert engine.next_frame_to_annotate_by(torch.tensor([50, 7, 9]), {0}) == 2        # an annotated frame is never suggested
    assert engine.next_frame_to_annotate_by([0, 0, 0], [1]) == 0
    assert engine.next_frame_to_annotate_by([3, 4], [0, 1]) is None


# ---- what the GPU tests can decide, from the restatements alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("frames", FC.FUSE_SETS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("hard", [False, True])
def test_fused_clip_is_decidable_on_the_oracles_lists(frames, hard):
    from fgvc_amd import engine
    T, h, w, (hp, wp), pad, Hf, Wf = FC.late_geometry()
    _, small = FC.small_maps(frames, pad, Hf, Wf)
    fw, bw = FC.oracle_sweep(frames[0], "fw"), FC.oracle_sweep(frames[-1], "bw")
    rows, dis = engine.fuse_refs_host(small, T, fw=fw, bw=bw, hard_prop=hard)
    _, gap = R.readout_f64(rows, Hf, Wf, (hp, wp), pad, (h, w))
    free = [t for t in range(T) if t not in frames]
    share = float((gap[free] > R.DECIDE).double().mean())
    Fp, Bp = FC.passes_f64(small, T, fw, bw, hard)
    mid = FC.between(frames)
    loose = torch.stack([(FC.row_gap(Fp[t]) <= R.DECIDE) | (FC.row_gap(Bp[t]) <= R.DECIDE) for t in mid])
    print(f"fused {frames} hard={hard}: decidable share {share:.4f} of the un-annotated frames' pixels; {int(loose.sum())} of {loose.numel()} "
          f"between-annotation cells undecided by a pass; disagree {dis.tolist()}")
    assert share > 0.95
    assert float(loose.double().mean()) <= 0.05
    lo, hi = FC.disagree_bounds(Fp, Bp, frames, T)
    assert bool((lo <= dis).all()) and bool((dis <= hi).all()) and int(dis[mid].sum()) > 0 and int(dis[list(frames)].sum()) == 0


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------
def test_fuse_export_in_header_and_bindings():
    from fgvc_amd import _lib, build
    assert "fuse.hip" in build.SOURCES
    hdr = open(os.path.join(ROOT, "include", "fgvc_hip.h")).read()
    lib = _lib.load()
    decl = re.search(r"\bint fgvc_seg_fuse_rows_f32\s*\(([^;]*)\);", hdr, re.S)
    assert decl and len(decl.group(1).split(",")) == len(_lib.SIGNATURES["fgvc_seg_fuse_rows_f32"][1])
    assert hasattr(lib, "fgvc_seg_fuse_rows_f32")


def test_fuse_export_checks_its_arguments():
    import ctypes
    from fgvc_amd import _lib
    lib = _lib.load()
    p, nul = ctypes.c_void_p(8), ctypes.c_void_p(0)
    ok = (2, 3, 3, 3, 16, 4)                                                         # n_items, n_fw, n_bw, n_out, HW, C
    for i in range(4):
        ptrs = [p, p, p, p]
        ptrs[i] = nul
        assert lib.fgvc_seg_fuse_rows_f32(*ptrs, *ok, p, nul) == _lib.ERR_INVALID_ARG and b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_seg_fuse_rows_f32(p, p, p, p, *ok, nul, nul) == _lib.ERR_INVALID_ARG and b"null pointer" in lib.fgvc_last_error()
    for bad in ((-1, 3, 3, 3, 16, 4), (65536, 3, 3, 3, 16, 4), (2, 0, 3, 3, 16, 4), (2, 3, 0, 3, 16, 4), (2, 3, 3, 0, 16, 4),
                (2, 3, 3, 3, 0, 4), (2, 3, 3, 3, 16, 0), (2, 3, 3, 3, 16, 257)):
        assert lib.fgvc_seg_fuse_rows_f32(p, p, p, p, *bad, p, nul) == _lib.ERR_INVALID_ARG and b"bad shape" in lib.fgvc_last_error(), bad
    assert lib.fgvc_seg_fuse_rows_f32(p, p, p, p, 0, 3, 3, 3, 16, 4, p, nul) == _lib.FGVC_OK       # no items: nothing to launch


def test_seg_fuse_rows_refuses_bad_calls_before_any_launch():
    """Every refusal needs no device: host tensors get through the argument checks and are refused last, by name."""
    from fgvc_amd import _lib, ops
    fw, bw = torch.zeros(4, 6, 3), torch.zeros(5, 6, 3)
    good = dict(fw_index=[1, 3], bw_index=[4, 0], weights=[0.25, 0.75])
    with pytest.raises(_lib.FgvcHipError, match="on the GPU"):
        ops.seg_fuse_rows(fw, bw, **good)
    with pytest.raises(TypeError, match="fw: expected torch.float32"):
        ops.seg_fuse_rows(fw.double(), bw, **good)
    with pytest.raises(TypeError, match="bw: expected torch.float32"):
        ops.seg_fuse_rows(fw, bw.half(), **good)
    with pytest.raises(ValueError, match="fw is not contiguous"):
        ops.seg_fuse_rows(torch.zeros(4, 3, 6).transpose(1, 2), bw, **good)
    with pytest.raises(ValueError, match="bw is not contiguous"):
        ops.seg_fuse_rows(fw, torch.zeros(5, 6, 6)[:, :, ::2], **good)
    with pytest.raises(ValueError, match="a stack"):
        ops.seg_fuse_rows(fw[0], bw, **good)
    with pytest.raises(ValueError, match="bw .* against fw"):
        ops.seg_fuse_rows(fw, torch.zeros(5, 7, 3), **good)
    with pytest.raises(ValueError, match="C=257"):
        ops.seg_fuse_rows(torch.zeros(2, 2, 257), torch.zeros(2, 2, 257), [0], [0], [0.5])
    for key, bad, name in (("fw_index", [1, 4], "fw_index 4"), ("fw_index", [-1, 3], "fw_index -1"), ("bw_index", [5, 0], "bw_index 5"),
                           ("bw_index", [0, 1.5], "bw_index 1.5")):
        with pytest.raises(ValueError, match=name + " outside"):
            ops.seg_fuse_rows(fw, bw, **dict(good, **{key: bad}))
    for w in (-0.01, 1.01, float("nan"), float("inf"), "0.5", True):
        with pytest.raises(ValueError, match="0 <= w <= 1"):
            ops.seg_fuse_rows(fw, bw, **dict(good, weights=[0.5, w]))
    import numpy as np
    with pytest.raises(_lib.FgvcHipError, match="on the GPU"):                       # numpy and 0-d tensor scalars are numbers too
        ops.seg_fuse_rows(fw, bw, **dict(good, weights=[np.float32(0.25), torch.tensor(0.75)]))
    with pytest.raises(ValueError, match="0 <= w <= 1"):
        ops.seg_fuse_rows(fw, bw, **dict(good, weights=[np.float32(0.25), torch.tensor(1.5)]))
    with pytest.raises(ValueError, match="one of each per item"):
        ops.seg_fuse_rows(fw, bw, [1, 3], [4], [0.25, 0.75])
    with pytest.raises(ValueError, match="one of each per item"):
        ops.seg_fuse_rows(fw, bw, [], [], [])
    with pytest.raises(ValueError, match="names a block twice"):
        ops.seg_fuse_rows(fw, bw, **dict(good, fw_index=[1, 1]))
    out = torch.zeros(3, 6, 3)
    with pytest.raises(ValueError, match="out_index is needed"):
        ops.seg_fuse_rows(fw, bw, out=out, **good)
    with pytest.raises(ValueError, match="out_index 3 outside"):
        ops.seg_fuse_rows(fw, bw, out=out, out_index=[0, 3], **good)
    with pytest.raises(ValueError, match="names a block twice"):
        ops.seg_fuse_rows(fw, bw, out=out, out_index=[2, 2], **good)
    with pytest.raises(ValueError, match="out_index == fw_index"):
        ops.seg_fuse_rows(fw, bw, out=fw, out_index=[3, 1], **good)
    with pytest.raises(ValueError, match="shares memory with fw"):
        ops.seg_fuse_rows(fw, bw, out=fw[1:], out_index=[0, 1], **good)
    with pytest.raises(ValueError, match="shares memory with bw"):
        ops.seg_fuse_rows(fw, bw, out=bw[:3], out_index=[0, 1], **good)
    with pytest.raises(TypeError, match="out: expected torch.float32"):
        ops.seg_fuse_rows(fw, bw, out=out.double(), out_index=[0, 1], **good)
    with pytest.raises(_lib.FgvcHipError, match="on the GPU"):
        ops.seg_fuse_rows(fw, bw, out=out, out_index=[0, 1], **good)


# ---- the code object -----------------------------------------------------------------------------------------------------------------------
def test_fuse_kernel_uses_no_scratch():
    """The fuse kernel in the code-object notes of the built library: one kernel, no scratch memory, no spilled register."""
    notes = _tool("kernel_notes").kernel_notes()
    ks = {k: v for k, v in notes.items() if "seg_fuse_rows_kernel" in k}
    assert len(ks) == 1, sorted(ks)
    for k, v in ks.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
