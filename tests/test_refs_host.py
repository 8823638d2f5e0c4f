"""CPU tests of annotations at any frame (test_cfg.refs): the key's and the mapping's refusals, the rule itself (engine.sweep_refs_host) on
hand-made lists, next_frame_to_annotate, the share of pixels the GPU tests can decide (from the oracle's lists and the float64 restatement
alone), the YouTube-VOS adapter on synthetic clips, and the C surface of the new exports."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import refs_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_parse_refs_defaults_and_refusals():
    from fgvc_amd import engine
    assert engine.parse_refs(None) is None
    assert engine.parse_refs({}) == engine.RefsConfig("forward", "new", False)
    assert engine.parse_refs(dict(direction="both", override="all", confidence=True)) == engine.RefsConfig("both", "all", True)
    with pytest.raises(ValueError, match="unknown key.*frames"):
        engine.parse_refs(dict(frames=3))
    with pytest.raises(ValueError, match="direction='backward'"):
        engine.parse_refs(dict(direction="backward"))
    with pytest.raises(ValueError, match="override='some'"):
        engine.parse_refs(dict(override="some"))
    with pytest.raises(ValueError, match="confidence"):
        engine.parse_refs(dict(confidence="yes"))
    with pytest.raises(TypeError, match="test_cfg.refs"):
        engine.parse_refs("both")


def test_ref_map_refusals():
    from fgvc_amd import engine
    m = torch.zeros(6, 8, dtype=torch.long)
    m[1:3, 2:5] = 2
    ok = engine.check_ref_maps({3: m, 1: m[None]}, 5, (6, 8))
    assert list(ok) == [1, 3] and all(v.dtype == torch.uint8 and v.shape == (6, 8) for v in ok.values())
    assert list(engine.check_ref_maps(m, 5, (6, 8))) == [0]                           # a tensor still means {0: tensor}
    with pytest.raises(TypeError, match="mapping"):
        engine.check_ref_maps([m], 5, (6, 8))
    with pytest.raises(ValueError, match="empty"):
        engine.check_ref_maps({}, 5, (6, 8))
    for bad in (5, -1):
        with pytest.raises(ValueError, match="outside the clip's 5 frames"):
            engine.check_ref_maps({bad: m}, 5, (6, 8))
    with pytest.raises(ValueError, match=r"size \(6, 8\)"):
        engine.check_ref_maps({0: m[:, :7]}, 5, (6, 8))
    with pytest.raises(NotImplementedError, match="255"):
        engine.check_ref_maps({0: m + 300}, 5, (6, 8))
    with pytest.raises(ValueError, match="negative"):
        engine.check_ref_maps({0: m - 1}, 5, (6, 8))
    with pytest.raises(TypeError, match="integer"):
        engine.check_ref_maps({0: m.float()}, 5, (6, 8))


def _model(typ, **test_cfg):
    import fgvc_amd.mmpt_api as api
    cfg = dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True)
    cfg.update(test_cfg)
    return api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,), pool_type="none")),
                           test_cfg=cfg)


def test_trackers_read_the_key():
    from fgvc_amd import engine
    assert _model("VanillaTracker").refs_cfg is None and _model("VanillaTracker").last_confidence is None
    assert _model("VanillaTracker", refs=dict(direction="both")).refs_cfg == engine.RefsConfig("both", "new", False)
    with pytest.raises(ValueError, match="test_cfg.refs"):
        _model("VanillaTracker", refs=dict(direction="up"))
    imgs, meta = torch.zeros(1, 1, 3, 4, 16, 16), [dict(original_shape=(16, 16))]
    refs = {0: torch.zeros(16, 16, dtype=torch.uint8)}
    with pytest.raises(TypeError, match="test_cfg.refs"):                             # the mapping without the key
        _model("VanillaTracker")(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    with pytest.raises(NotImplementedError, match="test_cfg.refs"):                   # the local-window tracker
        _model("HRVanillaTracker", refs={})(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    for key in ("coords", "return_maps"):
        with pytest.raises(NotImplementedError, match="test_cfg.refs"):
            _model("VanillaTracker", refs={}, **{key: True})(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)


# ---- the rule on hand-made lists: 4 cells, k = 1, one key slot (the previous frame) -----------------------------------------------------
def _shift_lists(n, HW=4):
    """Sub-clip lists that copy cell p of frame j - 1 to cell (p + 1) % HW of frame j: slot_frame (n-1, 1), idx / weight (n-1, HW, 1)."""
    idx = torch.tensor([[(p - 1) % HW] for p in range(HW)])
    return SimpleNamespace(slot_frame=torch.arange(n - 1).view(-1, 1), idx=idx[None].repeat(n - 1, 1, 1),
                           weight=torch.ones(n - 1, HW, 1, dtype=torch.float64))


def test_sweep_refs_host_new_object_and_override():
    from fgvc_amd import engine
    T = 5
    small = {0: torch.tensor([1, 0, 0, 0]), 2: torch.tensor([0, 1, 3, 3])}            # frame 2 re-draws id 1 at cell 1 and brings a new id 3
    soft = engine.sweep_refs_host(small, T, fw=_shift_lists(T), override="new")
    assert soft.shape == (T, 4, 4) and soft.dtype == torch.float64
    assert torch.equal(soft[:2, :, 3], torch.zeros(2, 4, dtype=torch.float64))         # the object's channel is exactly 0 before its annotation
    assert soft[0].argmax(-1).tolist() == [1, 0, 0, 0] and soft[1].argmax(-1).tolist() == [0, 1, 0, 0]
    # frame 2: id 1 has propagated to cell 2, where the new id 3 is injected; cells 0 and 1 keep their propagated rows (the re-drawn id 1 at
    # cell 1 is a known id: ignored), cells 2 and 3 become id 3
    assert soft[2].argmax(-1).tolist() == [0, 0, 3, 3]
    assert soft[3].argmax(-1).tolist() == [3, 0, 0, 3] and soft[4].argmax(-1).tolist() == [3, 3, 0, 0]
    every = engine.sweep_refs_host(small, T, fw=_shift_lists(T), override="all")
    assert torch.equal(every[2], torch.nn.functional.one_hot(small[2], 4).double())     # 'all' replaces every row
    assert every[3].argmax(-1).tolist() == [3, 0, 1, 3]
    assert torch.equal(every[:2], soft[:2])


def test_sweep_refs_host_new_leaves_known_rows_alone_on_soft_values():
    from fgvc_amd import engine
    lists = _shift_lists(3)
    lists.weight = torch.full((2, 4, 1), 0.5, dtype=torch.float64)                    # propagated rows are soft: 0.5 x the source row
    small = {0: torch.tensor([1, 0, 2, 0]), 1: torch.tensor([2, 2, 0, 3])}
    soft = engine.sweep_refs_host(small, 3, fw=lists, override="new")
    want1 = 0.5 * torch.nn.functional.one_hot(torch.tensor([0, 1, 0, 2]), 4).double()
    want1[3] = torch.tensor([0, 0, 0, 1.0])                                           # only the new id 3's cell is replaced
    assert torch.equal(soft[1], want1)
    hard = engine.sweep_refs_host(small, 3, fw=lists, override="new", hard_prop=True)
    assert torch.equal(hard[1], want1)                                                # the read-out sees the soft rows ...
    assert torch.equal(hard[2], torch.nn.functional.one_hot(torch.tensor([3, 0, 1, 0]), 4).double() * 0.5)   # ... the bank the hard ones


def test_sweep_refs_host_both_directions():
    from fgvc_amd import engine
    T, s0 = 5, 3
    small = {3: torch.tensor([0, 2, 0, 0]), 4: torch.tensor([0, 0, 0, 0])}
    fwd = engine.sweep_refs_host(small, T, fw=_shift_lists(T - s0), bw=None, direction="forward")
    assert torch.equal(fwd[:s0].argmax(-1), torch.zeros(s0, 4, dtype=torch.long))      # frames before s0: background
    assert torch.equal(fwd[:s0, :, 0], torch.ones(s0, 4, dtype=torch.float64))
    assert fwd[3].argmax(-1).tolist() == [0, 2, 0, 0] and fwd[4].argmax(-1).tolist() == [0, 0, 2, 0]
    both = engine.sweep_refs_host(small, T, fw=_shift_lists(T - s0), bw=_shift_lists(s0 + 1), direction="both")
    assert torch.equal(both[s0:], fwd[s0:])
    # the reversed sub-clip is frames 3, 2, 1, 0: its frame j is clip frame 3 - j, and the shift moves the object one cell per sub-clip frame
    assert [both[f].argmax(-1).tolist() for f in (2, 1, 0)] == [[0, 0, 2, 0], [0, 0, 0, 2], [2, 0, 0, 0]]
    with pytest.raises(ValueError):
        engine.sweep_refs_host(small, T, fw=_shift_lists(2), direction="backward")


def test_next_frame_to_annotate():
    from fgvc_amd import engine
    assert engine.next_frame_to_annotate([0.9, 0.2, 0.5, 0.2], [0]) == 1              # the lowest index among equals
    assert engine.next_frame_to_annotate([0.9, 0.2, 0.5, 0.2], [0, 1]) == 3
    assert engine.next_frame_to_annotate(torch.tensor([0.1, 0.2, 0.5]), {0}) == 1      # an annotated frame is never suggested
    assert engine.next_frame_to_annotate(np.array([0.3, 0.3]), []) == 0
    assert engine.next_frame_to_annotate([0.1, 0.2], [0, 1]) is None                  # an all-annotated clip
    s = torch.zeros(3, 2, 2, dtype=torch.int64)
    s[:, 0, 1] = torch.tensor([255 * 12, 0, 6 * 255])
    assert engine.frame_scores(s, (3, 4)).tolist() == [1.0, 0.0, 0.5]


def test_label_set_words_round_trip():
    from fgvc_amd import ops
    ids = [0, 31, 32, 200, 255]
    w = ops.label_set_words(ids)
    assert w.dtype == torch.int32 and w.shape == (8,) and ops.label_set_ids(w) == ids
    assert ops.label_set_ids(ops.label_set_words([])) == []
    with pytest.raises(ValueError):
        ops.label_set_words([256])


# ---- what the GPU tests can decide, from the restatements alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("override", ["new", "all"])
def test_late_object_clip_is_decidable_on_the_oracles_lists(override):
    from fgvc_amd import engine
    T, h, w, d = R.LATE_T, R.LATE_H, R.LATE_W, R.LATE_D
    (hp, wp), pad = engine.pad_divide_by(h, w, d)
    Hf, Wf = hp // d, wp // d
    cfg = engine.TrackerConfig(**R.LATE_KW)
    lists = R.oracle_lists(R.clip_chw(T, 64, Hf, Wf, R.LATE_SEED), cfg)
    small = {t: torch.from_numpy(R.pil_nearest(np.pad(m, ((pad[2], pad[3]), (pad[0], pad[1]))), Hf, Wf).astype(np.int64))
             for t, m in R.late_maps().items()}
    want, gap = R.restated_masks(small, T, lists, None, "forward", override, False, Hf, Wf, (hp, wp), pad, (h, w))
    share = float((gap[1:] > R.DECIDE).double().mean())
    print(f"late-object clip, override={override}: decidable share {share:.4f} on the oracle's lists")
    assert share > 0.95
    assert not bool((want[:3] == 4).any()) and bool((want[3:] == 4).any())            # the late object: absent before frame 3, present after


@pytest.mark.parametrize("case", R.CONF_CASES, ids=lambda c: f"{c[1]}x{c[2]}C{c[3]}to{c[6][0]}x{c[6][1]}")
@pytest.mark.parametrize("norm", [True, False])
def test_confidence_recipe_excludes_few_pixels(case, norm):
    n, Hf, Wf, C, pad_shape, pad, out_shape = case
    lab = R.conf_labels(n, Hf, Wf, C, Hf * 31 + C)
    assert float(lab.abs().max()) <= 1.0
    want, den_min = R.conf_f64(lab, Hf, Wf, pad_shape, pad, out_shape, norm)
    delta = R.conf_delta(case, norm, den_min)
    _, _, excluded = R.conf_verdict(torch.round(want), want, delta)
    levels = int(torch.round(want).unique().numel())
    print(f"confidence {case} norm={norm}: delta = {delta:.4f} levels (smallest denominator {den_min:.3f}), excluded share {excluded:.4f}, "
          f"{levels} distinct levels")
    assert 0 < delta < 0.5 and excluded <= R.CONF_EXCLUDED_MAX
    assert levels == 1 if C == 1 else levels > 50                                     # the recipe exercises the byte's range


# ---- the YouTube-VOS adapter (parity unpinned: synthetic clips in the format's layout) -----------------------------------------------------
def test_ytvos_round_trip(tmp_path):
    from fgvc_amd.datasets import YoutubeVos
    made = R.write_fake_ytvos(str(tmp_path), videos=2, frames=6, size=(48, 64), seed=3)
    ds = YoutubeVos(str(tmp_path))
    assert len(ds) == 2 and ds.videos == sorted(made)
    for i, name in enumerate(ds.videos):
        data, meta = ds[i]
        names, refs, maps = made[name]
        assert meta["name"] == name and meta["frames"] == names and meta["n_objects"] == 2
        assert data["imgs"].shape == (1, 1, 3, 6, 48, 64) and data["img_meta"][0]["original_shape"] == (48, 64)
        assert sorted(data["ref_seg_map"]) == [0, 2]
        for t, m in refs.items():
            assert np.array_equal(data["ref_seg_map"][t].numpy(), m)
        assert meta["has_gt"].tolist() == [True, False, True, False, False, False]
    raw = YoutubeVos(str(tmp_path), raw=True, max_frames=2)[0]
    assert raw[0]["imgs"].dtype == torch.uint8 and raw[0]["imgs"].shape == (1, 1, 2, 48, 64, 3) and sorted(raw[0]["ref_seg_map"]) == [0]


def test_ytvos_meta_that_disagrees_with_the_pngs(tmp_path):
    import json
    from fgvc_amd.datasets import YoutubeVos
    made = R.write_fake_ytvos(str(tmp_path), videos=2, frames=5, size=(32, 40), seed=4)
    path = os.path.join(str(tmp_path), "meta.json")
    meta = json.load(open(path))
    names = made["vid01"][0]
    meta["videos"]["vid01"]["objects"]["2"]["frames"] = names[1:]                     # frame 1 has no PNG
    json.dump(meta, open(path, "w"))
    ds = YoutubeVos(str(tmp_path))
    ds[0]
    with pytest.raises(ValueError, match="vid01.*does not exist"):
        ds[1]
    meta["videos"]["vid01"]["objects"]["2"]["frames"] = names                         # frame 0's PNG does not show object 2
    json.dump(meta, open(path, "w"))
    with pytest.raises(ValueError, match="vid01.*does not show it"):
        YoutubeVos(str(tmp_path))[1]


def test_ytvos_run_writes_palette_pngs(tmp_path):
    from PIL import Image
    from fgvc_amd.datasets import YoutubeVos, ytvos_run
    from fgvc_amd.viz import davis_palette
    src, out = tmp_path / "data", tmp_path / "out"
    made = R.write_fake_ytvos(str(src), videos=2, frames=5, size=(32, 40), seed=5, full_gt=True)
    ds = YoutubeVos(str(src))

    def echo(test_mode, imgs, ref_seg_map, img_meta):                                 # a stand-in tracker: every frame is its annotation
        assert sorted(ref_seg_map) == [0, 2]
        name = ds.videos[echo.calls]
        echo.calls += 1
        return [made[name][2].astype(np.float64)]
    echo.calls = 0
    res = ytvos_run(echo, ds, str(out))
    assert res["videos"] == ds.videos and res["jf"]["J&F-Mean"] == pytest.approx(1.0)
    for name, (names, _, maps) in made.items():
        for t, n in enumerate(names):
            im = Image.open(out / "Annotations" / name / (n + ".png"))
            assert im.mode == "P" and np.array_equal(np.asarray(im), maps[t])
            assert np.array_equal(np.asarray(im.getpalette()[:768], np.uint8).reshape(-1, 3), davis_palette())
    sparse = tmp_path / "sparse"
    R.write_fake_ytvos(str(sparse), videos=1, frames=4, size=(32, 40), seed=6)
    echo.calls, made = 0, {"vid00": (None, None, np.zeros((4, 32, 40), np.uint8))}
    assert ytvos_run(echo, YoutubeVos(str(sparse)))["jf"] is None                       # nothing to score beyond the given frames


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------
NEW_EXPORTS = ("fgvc_seg_label_set_u8", "fgvc_seg_inject_labels_u8", "fgvc_seg_readout_conf_u8")


def test_new_exports_in_header_and_bindings():
    from fgvc_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "fgvc_hip.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, hdr, re.S)
        assert decl, name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name     # one ctypes argument per declared parameter
        assert hasattr(lib, name)


def test_new_exports_check_their_arguments():
    import ctypes
    from fgvc_amd import _lib
    lib = _lib.load()
    p, nul = ctypes.c_void_p(8), ctypes.c_void_p(0)
    assert lib.fgvc_seg_label_set_u8(nul, 4, 4, 2, 2, p, nul) == _lib.ERR_INVALID_ARG and b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_seg_label_set_u8(p, 4, 4, 0, 2, p, nul) == _lib.ERR_INVALID_ARG and b"bad shape" in lib.fgvc_last_error()
    assert lib.fgvc_seg_label_set_u8(p, 4, 4, 20000, 2, p, nul) == _lib.ERR_UNSUPPORTED
    assert lib.fgvc_seg_inject_labels_u8(p, 4, 4, 2, 2, 3, nul, p, nul) == _lib.ERR_INVALID_ARG and b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_seg_inject_labels_u8(p, 4, 4, 2, 2, 257, p, p, nul) == _lib.ERR_INVALID_ARG and b"1 <= C <= 256" in lib.fgvc_last_error()
    args = (2, 5, 6, 3, 10, 12, 0, 0, 10, 12, 10, 12, 1)
    assert lib.fgvc_seg_readout_conf_u8(p, *args, p, nul, p, p, nul) == _lib.ERR_INVALID_ARG and b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_seg_readout_conf_u8(p, *args, p, p, p, nul, nul) == _lib.ERR_INVALID_ARG and b"workspace" in lib.fgvc_last_error()
    bad = (2, 5, 6, 3, 10, 12, 1, 0, 10, 12, 10, 12, 1)
    assert lib.fgvc_seg_readout_conf_u8(p, *bad, p, p, p, p, nul) == _lib.ERR_INVALID_ARG and b"inside the padded frame" in lib.fgvc_last_error()
    assert lib.fgvc_seg_readout_conf_u8(p, 0, *args[1:], p, p, p, nul, nul) == _lib.FGVC_OK      # no frames: nothing to launch
