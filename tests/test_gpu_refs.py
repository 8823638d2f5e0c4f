"""GPU tests of annotations at any frame (test_cfg.refs): the presence-set and injection kernels against Pillow NEAREST + torch, the
engine against propagate_masks (one map at frame 0, both time directions) and against engine.sweep_refs_host on the kernels' own lists
(late object, correction), the label session's counters, the confidence read-out against ops.seg_readout and a float64 restatement, and
the tracker API / demo tool end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import refs_cases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- fgvc_seg_label_set_u8 / fgvc_seg_inject_labels_u8 ---------------------------------------------------------------------------------------
def _id_map(hw, seed):
    rng = np.random.default_rng(seed)
    a = rng.choice(np.array([0, 1, 2, 7, 31, 32, 200, 255], np.uint8), size=hw)
    a[:2, :2] = 255                                           # the first NEAREST sample of every size used here falls into this corner: id 255 is present
    return a


@pytest.mark.parametrize("hw, Hf_Wf", [((100, 100), (33, 27)), ((7, 9), (3, 5)), ((37, 50), (37, 50))])
def test_label_set_matches_pillow(dev, hw, Hf_Wf):
    from fgvc_amd import ops
    Hf, Wf = Hf_Wf
    a = _id_map(hw, hw[0])
    small = R.pil_nearest(a, Hf, Wf)
    words = ops.seg_label_set(torch.from_numpy(a).to(dev), Hf, Wf).cpu()
    assert words.shape == (8,) and words.dtype == torch.int32
    assert ops.label_set_ids(words) == sorted(set(small.flatten().tolist()))
    assert 255 in ops.label_set_ids(words)
    one = torch.full((5, 6), 3, dtype=torch.uint8, device=dev)
    assert ops.label_set_ids(ops.seg_label_set(one, 2, 3).cpu()) == [3]


@pytest.mark.parametrize("hw, Hf_Wf", [((100, 100), (33, 27)), ((7, 9), (3, 5)), ((37, 50), (37, 50))])
@pytest.mark.parametrize("C", [1, 3, 256])
def test_inject_labels_matches_pillow_and_torch(dev, hw, Hf_Wf, C):
    from fgvc_amd import ops
    Hf, Wf = Hf_Wf
    HW = Hf * Wf
    a = _id_map(hw, hw[0] + C)
    small = torch.from_numpy(R.pil_nearest(a, Hf, Wf).astype(np.int64)).reshape(-1)
    present = sorted(set(small.tolist()))
    m = torch.from_numpy(a).to(dev)
    g = torch.Generator().manual_seed(C)
    base = torch.rand(HW, C, generator=g) + 0.25                           # a non-zero row block, written in place
    onehot = torch.zeros(HW, C)
    inside = small < C                                                      # an id >= C: a zero row, as seg_onehot_labels
    onehot[inside.nonzero().flatten(), small[inside]] = 1.0
    assert torch.equal(ops.seg_onehot_labels(m, Hf, Wf, C).cpu(), onehot)

    def run(ids):
        buf = torch.full((HW + 2, C), float("nan"))                        # a NaN guard row before and after the block
        buf[1:-1] = base
        d = buf.to(dev)
        ops.seg_inject_labels(m, Hf, Wf, C, ops.label_set_words(ids).to(dev), d[1:-1])
        out = d.cpu()
        assert bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[-1]).all())
        return out[1:-1]

    assert torch.equal(run([]), base)                                       # an empty set: the rows are untouched
    assert torch.equal(run(present), onehot)                                # every id: the one-hot kernel's result
    assert torch.equal(run(list(range(256))), onehot)
    absent = [i for i in (5, 6) if i not in present]
    some = [present[-1], present[0]] + absent                               # a set that also holds ids the map does not have
    sel = torch.isin(small, torch.tensor(some))
    want = torch.where(sel[:, None], onehot, base)
    got = run(some)
    assert torch.equal(got, want) and bool(sel.any()) and not bool(sel.all())
    assert torch.equal(run(absent), base)


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
def _late_setup(dev):
    from fgvc_amd import engine, ops
    T, h, w, d = R.LATE_T, R.LATE_H, R.LATE_W, R.LATE_D
    (hp, wp), pad = engine.pad_divide_by(h, w, d)
    Hf, Wf = hp // d, wp // d
    feats = ops.normalize_to_hwc(R.clip_chw(T, 64, Hf, Wf, R.LATE_SEED).to(dev))
    padded = {t: np.pad(m, ((pad[2], pad[3]), (pad[0], pad[1]))) for t, m in R.late_maps().items()}
    segs = {t: torch.from_numpy(m).to(dev) for t, m in padded.items()}
    small = {t: torch.from_numpy(R.pil_nearest(m, Hf, Wf).astype(np.int64)) for t, m in padded.items()}
    return SimpleClip(T=T, h=h, w=w, hp=hp, wp=wp, pad=pad, Hf=Hf, Wf=Wf, feats=feats, segs=segs, small=small)


class SimpleClip:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def late(dev):
    return _late_setup(dev)


@pytest.mark.parametrize("hard", [False, True])
def test_one_map_at_frame_0_is_propagate_masks(dev, late, hard):
    from fgvc_amd import engine
    c = late
    cfg = engine.TrackerConfig(hard_prop=hard, **R.LATE_KW)
    want = engine.propagate_masks(c.feats, c.Hf, c.Wf, c.segs[0], c.pad, (c.h, c.w), cfg)
    got = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, {0: c.segs[0]}, c.pad, (c.h, c.w), cfg, engine.RefsConfig())
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    both = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, {0: c.segs[0]}, c.pad, (c.h, c.w), cfg, engine.RefsConfig("both", "all"))
    assert torch.equal(both, want)                              # nothing lies before frame 0, nothing is injected


@pytest.mark.parametrize("hard", [False, True])
@pytest.mark.parametrize("override", ["new", "all"])
def test_late_object_and_correction_match_the_rule(dev, late, override, hard):
    from fgvc_amd import engine
    c = late
    cfg = engine.TrackerConfig(hard_prop=hard, **R.LATE_KW)
    sweeps = {}
    masks = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, c.segs, c.pad, (c.h, c.w), cfg, engine.RefsConfig("forward", override),
                                        sweeps=sweeps).cpu()
    assert masks.shape == (c.T, c.h, c.w) and list(sweeps) == [(0, "fw")]
    assert torch.equal(masks[0], torch.from_numpy(R.late_maps()[0]))
    want, gap = R.restated_masks(c.small, c.T, sweeps[(0, "fw")], None, "forward", override, hard, c.Hf, c.Wf, (c.hp, c.wp), c.pad, (c.h, c.w))
    dec = gap[1:] > R.DECIDE
    bad = int(((masks[1:].long() != want[1:]) & dec).sum())
    share = float(dec.double().mean())
    print(f"late object override={override} hard={hard}: decidable share {share:.4f}, {bad} decidable mismatches of {dec.numel()}")
    assert bad == 0 and share > 0.95
    assert not bool((masks[:3] == 4).any()) and bool((masks[3:] == 4).any())       # id 4 is absent from frames 0..2
    if override == "all" and not hard:
        # the correction: frame 3's rows are the annotation's one-hot rows, so its read-out follows the re-drawn object 2
        # (two pixels inside the rectangle 38:58 x 24:50 every tap of the stride-2 grid lies in it)
        assert bool((masks[3][40:56, 26:48] == 2).all())


def test_both_ways_is_the_forward_call_on_the_reversed_sub_clip(dev, late):
    from fgvc_amd import engine
    c = late
    cfg = engine.TrackerConfig(**R.LATE_KW)
    s0, seg = 4, c.segs[0]
    both = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, {s0: seg}, c.pad, (c.h, c.w), cfg, engine.RefsConfig("both", "new"))
    fwd = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, {s0: seg}, c.pad, (c.h, c.w), cfg, engine.RefsConfig("forward", "new"))
    tail = engine.propagate_masks(c.feats[s0:].contiguous(), c.Hf, c.Wf, seg, c.pad, (c.h, c.w), cfg)
    rev = torch.tensor([4, 3, 2, 1, 0], device=dev)
    head = engine.propagate_masks(c.feats.index_select(0, rev), c.Hf, c.Wf, seg, c.pad, (c.h, c.w), cfg)
    assert torch.equal(both[s0:], tail) and torch.equal(fwd[s0:], tail)
    assert torch.equal(both[:s0], head[1:].flip(0))                                # frames 3..0 = the reversed sub-clip's frames 1..4
    assert int(fwd[:s0].max()) == 0 and int(both[:s0].max()) > 0


# ---- the tracker API ---------------------------------------------------------------------------------------------------------------------------
def _model(dev, typ="VanillaTracker", **test_cfg):
    import fgvc_amd.mmpt_api as api
    cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True)
    cfg.update(test_cfg)
    torch.manual_seed(0)
    m = api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                        test_cfg=cfg)
    m.init_weights()
    return m.to(dev).eval()


def _api_clip(dev):
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, 5, 64, 64, generator=g).to(dev)
    a = torch.zeros(64, 64, dtype=torch.long)
    a[8:30, 8:30], a[36:58, 20:44] = 1, 2
    b = torch.zeros(64, 64, dtype=torch.long)
    b[10:28, 36:60] = 3
    return imgs, a, b, [dict(original_shape=(64, 64))]


def test_session_counters_and_results(dev):
    imgs, a, b, meta = _api_clip(dev)
    model = _model(dev, refs=dict(direction="both"))
    session = model.open_label_session(imgs, meta)
    assert session.counters == dict(encodes=1, affinity_runs=0, sweeps=0)
    first = session.propagate({0: a})
    assert session.counters == dict(encodes=1, affinity_runs=1, sweeps=1)
    second = session.propagate({0: a, 2: b})
    assert session.counters == dict(encodes=1, affinity_runs=1, sweeps=2)         # no encoder, no pair kernel, no merge
    moved = session.propagate({2: b})
    assert session.counters == dict(encodes=1, affinity_runs=2, sweeps=3)         # a new first frame: one more affinity run
    session.propagate({2: b}, direction="forward", override="all")
    assert session.counters == dict(encodes=1, affinity_runs=2, sweeps=4)
    # the model's own call gives the same arrays
    assert np.array_equal(first[0], model(test_mode=True, imgs=imgs, ref_seg_map={0: a}, img_meta=meta)[0])
    assert np.array_equal(second[0], model(test_mode=True, imgs=imgs, ref_seg_map={0: a, 2: b}, img_meta=meta)[0])
    assert np.array_equal(moved[0], model(test_mode=True, imgs=imgs, ref_seg_map={2: b}, img_meta=meta)[0])
    plain = _model(dev)(test_mode=True, imgs=imgs, ref_seg_map=a[None].to(dev), img_meta=meta)[0]
    assert np.array_equal(first[0], plain)                                         # {0: map} is the call without the key
    assert np.array_equal(model(test_mode=True, imgs=imgs, ref_seg_map=a[None].to(dev), img_meta=meta)[0], plain)   # a tensor still means {0: tensor}
    assert 3 in np.unique(second[0][2:]) and 3 not in np.unique(second[0][:2])
    session.close()
    with pytest.raises(RuntimeError, match="close"):
        session.propagate({0: a})


def test_api_device_masks_raw_input_and_confidence(dev):
    from fgvc_amd import engine
    imgs, a, b, meta = _api_clip(dev)
    refs = {0: a, 2: b}
    base = _model(dev, refs={})(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    assert base.dtype == np.float64 and base.shape == (5, 64, 64)
    model = _model(dev, refs=dict(confidence=True), masks="device")
    out = model(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    assert isinstance(out, list) and len(out) == 1 and out[0].is_cuda and out[0].dtype == torch.uint8
    assert np.array_equal(out[0].cpu().numpy().astype(np.float64), base)
    lc = model.last_confidence
    assert set(lc) == {"conf", "stats", "frame_score"} and lc["conf"].shape == (5, 64, 64) and lc["conf"].dtype == torch.uint8
    C = 4                                                                         # 1 + the largest id of any map
    assert lc["stats"].shape == (5, C, 2) and lc["stats"].dtype == torch.int64
    for f in range(5):
        assert torch.equal(lc["stats"][f, :, 0].cpu(), torch.bincount(out[0][f].flatten().long().cpu(), minlength=C))
    want_score = lc["conf"].cpu().double().flatten(1).mean(1) / 255.0
    assert lc["frame_score"].dtype == torch.float64 and torch.allclose(lc["frame_score"], want_score, rtol=0, atol=1e-12)
    assert float(lc["frame_score"][0]) == 1.0                                     # the given frame
    nxt = engine.next_frame_to_annotate(lc["frame_score"], refs)
    assert nxt in (1, 3, 4) and float(lc["frame_score"][nxt]) == float(lc["frame_score"][[1, 3, 4]].min())
    # raw rgb8 frames with a mapping
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (1, 1, 5, 64, 64, 3), generator=g, dtype=torch.uint8).to(dev)
    m_raw = _model(dev, refs={}, input=dict(type="rgb8"))
    got = m_raw(test_mode=True, imgs=raw, ref_seg_map=refs, img_meta=meta)[0]
    assert got.shape == (5, 64, 64) and np.array_equal(got[0], a.numpy().astype(np.float64)) and 3 in np.unique(got[2:])
    # refusals
    with pytest.raises(TypeError, match="test_cfg.refs"):
        _model(dev)(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    with pytest.raises(NotImplementedError, match="test_cfg.refs"):
        _model(dev, typ="HRVanillaTracker", refs={})(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)
    with pytest.raises(ValueError, match="outside the clip"):
        m_raw(test_mode=True, imgs=raw, ref_seg_map={5: a}, img_meta=meta)


# ---- fgvc_seg_readout_conf_u8 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CONF_CASES, ids=lambda c: f"{c[1]}x{c[2]}C{c[3]}to{c[6][0]}x{c[6][1]}")
@pytest.mark.parametrize("norm", [True, False])
def test_readout_conf(dev, case, norm):
    """Confidence read-out against ops.seg_readout (the same bytes), torch.bincount / per-id sums (exact) and the float64 restatement
    (within one level everywhere, equal outside refs_cases.conf_delta of a half-integer)."""
    from fgvc_amd import ops
    n, Hf, Wf, C, pad_shape, pad, out_shape = case
    lab = R.conf_labels(n, Hf, Wf, C, Hf * 31 + C)
    d = lab.to(dev)
    masks, conf, stats = ops.seg_readout_conf(d, Hf, Wf, pad_shape, pad, out_shape, norm)
    assert masks.shape == conf.shape == (n, *out_shape) and conf.dtype == torch.uint8 and stats.shape == (n, C, 2) and stats.dtype == torch.int64
    assert torch.equal(masks, ops.seg_readout(d, Hf, Wf, pad_shape, pad, out_shape, norm))
    masks, conf, stats = masks.cpu(), conf.cpu(), stats.cpu()
    for f in range(n):
        ids = masks[f].flatten().long()
        assert torch.equal(stats[f, :, 0], torch.bincount(ids, minlength=C))
        assert torch.equal(stats[f, :, 1], torch.bincount(ids, weights=conf[f].flatten().double(), minlength=C).long())
    again = ops.seg_readout_conf(d, Hf, Wf, pad_shape, pad, out_shape, norm)
    assert all(torch.equal(x.cpu(), y) for x, y in zip(again, (masks, conf, stats)))      # integer sums: the same on every run
    want, den_min = R.conf_f64(lab, Hf, Wf, pad_shape, pad, out_shape, norm)
    delta = R.conf_delta(case, norm, den_min)
    worst, bad, excluded = R.conf_verdict(conf, want, delta)
    print(f"confidence {case} norm={norm}: delta = {delta:.4f} levels, largest difference {worst:.0f} level(s), {bad} mismatches outside "
          f"delta, excluded share {excluded:.4f}")
    assert worst <= 1 and bad == 0 and excluded <= R.CONF_EXCLUDED_MAX
    if C == 1:
        assert bool((conf == 255).all())


# ---- the demo tool -----------------------------------------------------------------------------------------------------------------------------
def test_demo_tool_masks_at_two_frames(dev, tmp_path):
    from PIL import Image
    a = np.zeros((64, 64), np.uint8)
    a[8:30, 8:30] = 1
    b = np.zeros((64, 64), np.uint8)
    b[34:58, 30:56] = 2
    Image.fromarray(a).save(tmp_path / "A.png")
    Image.fromarray(b).save(tmp_path / "B.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demo.py"), "--synthetic", "5", "64", "64", "--task", "vos",
                        "--mask", "0", str(tmp_path / "A.png"), "--mask", "2", str(tmp_path / "B.png"), "--both-ways", "--confidence",
                        "--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    names = sorted(os.listdir(out))
    assert [n for n in names if n.startswith("conf_")] == [f"conf_{i:05d}.png" for i in range(5)]
    assert np.asarray(Image.open(out / "conf_00000.png")).shape == (64, 64)
    assert "frame_score" in r.stdout and "annotate next" in r.stdout
