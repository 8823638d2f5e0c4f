"""GPU tests of the fused forward / backward label sweeps (test_cfg.refs fuse='linear'): the fuse kernel alone against float64 (exact on
dyadic values, within fuse_cases.fuse_delta otherwise), one annotated frame against direction='both', the fused propagation against
engine.fuse_refs_host on the kernels' own lists, the label session's counters, and the tracker API / demo tool end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import fuse_cases as FC
from tests import refs_cases as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ---- fgvc_seg_fuse_rows_f32 alone ---------------------------------------------------------------------------------------------------------
def _guarded_call(dev, fw, bw, items, weights, in_place):
    """One ops.seg_fuse_rows call.  Separate output: the output stack and the count array lie between NaN / SENTINEL guards, and the
    blocks no item names stay NaN.  In place: the forward stack lies between NaN guard rows, and the blocks no item names keep their
    values.  Returns ([the item's output block (HW, C) on the host per item], counts (n,) on the host)."""
    from fgvc_amd import ops
    n_out, (_, HW, C), n = FC.FUSE_STACKS[2], fw.shape, len(items)
    cbuf = torch.full((n + 2,), SENTINEL, dtype=torch.int64, device=dev)
    fi, bi, oi = ([it[k] for it in items] for k in range(3))
    d_bw = bw.to(dev)
    if in_place:
        buf = torch.full((fw.shape[0] * HW + 2, C), float("nan"))
        buf[1:-1] = fw.reshape(-1, C)
        d = buf.to(dev)
        stack = d[1:-1].view(fw.shape[0], HW, C)
        out, counts = ops.seg_fuse_rows(stack, d_bw, fi, bi, weights, counts=cbuf[1:-1])
        assert out.data_ptr() == stack.data_ptr()
        got = d.cpu()
        res = got[1:-1].view(fw.shape[0], HW, C)
        for f in range(fw.shape[0]):
            if f not in fi:
                assert torch.equal(res[f], fw[f])
        blocks = [res[f] for f in fi]
    else:
        d = torch.full((n_out * HW + 2, C), float("nan"), device=dev)
        d_fw = fw.to(dev)
        out, counts = ops.seg_fuse_rows(d_fw, d_bw, fi, bi, weights, out=d[1:-1].view(n_out, HW, C), out_index=oi, counts=cbuf[1:-1])
        assert torch.equal(d_fw.cpu(), fw)                                       # the inputs are read only
        got = d.cpu()
        res = got[1:-1].view(n_out, HW, C)
        for f in range(n_out):
            if f not in oi:
                assert bool(torch.isnan(res[f]).all())
        blocks = [res[f] for f in oi]
    assert bool(torch.isnan(got[0]).all()) and bool(torch.isnan(got[-1]).all())
    assert torch.equal(d_bw.cpu(), bw)
    c = cbuf.cpu()
    assert int(c[0]) == SENTINEL and int(c[-1]) == SENTINEL and counts.data_ptr() == cbuf[1:-1].data_ptr()
    return blocks, c[1:-1]


@pytest.mark.parametrize("C", FC.FUSE_CHANNELS)
@pytest.mark.parametrize("HW", sorted(FC.FUSE_GRIDS))
def test_fuse_rows_dyadic_is_exact(dev, HW, C):
    n_fw, n_bw, _ = FC.FUSE_STACKS
    fw, bw = FC.dyadic_stack(n_fw, HW, C, 100 * HW + C), FC.dyadic_stack(n_bw, HW, C, 100 * HW + C + 50)
    for n, items in FC.FUSE_ITEMS.items():
        weights = [0.25, 0.5, 0.75][:n] if n > 1 else [0.75]
        want, want_n = FC.fuse_rows_f64(fw, bw, items, weights)
        for in_place in (False, True):
            blocks, counts = _guarded_call(dev, fw, bw, items, weights, in_place)
            for got, ref in zip(blocks, want):
                assert torch.equal(got.double(), ref)                            # every product and sum is exact in f32
            assert torch.equal(counts, want_n)
            again = _guarded_call(dev, fw, bw, items, weights, in_place)[1]
            assert torch.equal(again, counts)                                    # integer atomics: the same on every run
        if C == 1:
            assert int(want_n.sum()) == 0
        elif HW > 2:
            assert int(want_n.sum()) > 0


@pytest.mark.parametrize("C", FC.FUSE_CHANNELS)
@pytest.mark.parametrize("HW", sorted(FC.FUSE_GRIDS))
def test_fuse_rows_thirds_within_the_rounding_budget(dev, HW, C):
    n_fw, n_bw, _ = FC.FUSE_STACKS
    Hf, Wf = FC.FUSE_GRIDS[HW]
    fw = R.conf_labels(n_fw, Hf, Wf, C, 7 * HW + C)
    bw = torch.roll(R.conf_labels(n_bw, Hf, Wf, C, 7 * HW + C + 1), 1, dims=1)       # the region map one cell on: the passes disagree at its edges
    assert float(fw.abs().max()) <= 1.0 and float(bw.abs().max()) <= 1.0
    delta = FC.fuse_delta()
    for n, items in FC.FUSE_ITEMS.items():
        weights = [1 / 3, 2 / 3, 1 / 3][:n]
        want, want_n = FC.fuse_rows_f64(fw, bw, items, weights)
        for in_place in (False, True):
            blocks, counts = _guarded_call(dev, fw, bw, items, weights, in_place)
            worst = max(float((got.double() - ref).abs().max()) for got, ref in zip(blocks, want))
            print(f"fuse rows HW={HW} C={C} items={n} in_place={in_place}: largest error {worst / FC.U:.3f} U (budget {delta / FC.U:.3f} U), "
                  f"counts {counts.tolist()}")
            assert worst <= delta
            assert torch.equal(counts, want_n)          # the arg-maxima are taken on the f32 inputs themselves: no cell is undecidable
    # w = 0 and w = 1 give the backward and the forward block themselves
    from fgvc_amd import ops
    out = torch.empty((2, *fw.shape[1:]), device=dev)
    ops.seg_fuse_rows(fw.to(dev), bw.to(dev), [2, 2], [3, 3], [0.0, 1.0], out=out, out_index=[0, 1])
    assert torch.equal(out[0].cpu(), bw[3]) and torch.equal(out[1].cpu(), fw[2])


# ---- the engine ---------------------------------------------------------------------------------------------------------------------------
class Clip:
    def __init__(self, **kw):
        self.__dict__.update(kw)


@pytest.fixture(scope="module")
def late(dev):
    from fgvc_amd import ops
    T, h, w, (hp, wp), pad, Hf, Wf = FC.late_geometry()
    feats = ops.normalize_to_hwc(R.clip_chw(T, 64, Hf, Wf, R.LATE_SEED).to(dev))
    return Clip(T=T, h=h, w=w, hp=hp, wp=wp, pad=pad, Hf=Hf, Wf=Wf, feats=feats)


def _maps(dev, c, frames):
    padded, small = FC.small_maps(frames, c.pad, c.Hf, c.Wf)
    return {t: torch.from_numpy(m).to(dev) for t, m in padded.items()}, small


@pytest.mark.parametrize("hard", [False, True])
def test_one_annotated_frame_is_direction_both(dev, late, hard):
    from fgvc_amd import engine
    c = late
    cfg = engine.TrackerConfig(hard_prop=hard, **R.LATE_KW)
    segs, _ = _maps(dev, c, (4,))
    sweeps, dis = {}, []
    got = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, segs, c.pad, (c.h, c.w), cfg, engine.RefsConfig("both", "all", False, "linear"),
                                      sweeps=sweeps, disagree_out=dis)
    want = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, segs, c.pad, (c.h, c.w), cfg, engine.RefsConfig("both", "all"))
    assert torch.equal(got, want) and dis == [] and set(sweeps) == {(4, "fw"), (4, "bw")}


@pytest.mark.parametrize("frames", FC.FUSE_SETS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("hard", [False, True])
def test_fused_propagation_matches_the_rule(dev, late, frames, hard):
    from fgvc_amd import engine
    c = late
    cfg = engine.TrackerConfig(hard_prop=hard, **R.LATE_KW)
    segs, small = _maps(dev, c, frames)
    s0, sm = frames[0], frames[-1]
    sweeps, dis = {}, []
    masks = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, segs, c.pad, (c.h, c.w), cfg, engine.RefsConfig("both", "all", False, "linear"),
                                        sweeps=sweeps, disagree_out=dis).cpu()
    assert masks.shape == (c.T, c.h, c.w) and masks.dtype == torch.uint8
    assert set(sweeps) == {(s0, "fw"), (sm, "bw")}                               # no (s_m, 'fw'), no (s_0, 'bw')
    fw, bw = sweeps[(s0, "fw")], sweeps[(sm, "bw")]
    rows, _ = engine.fuse_refs_host(small, c.T, fw=fw, bw=bw, hard_prop=hard)
    want, gap = R.readout_f64(rows, c.Hf, c.Wf, (c.hp, c.wp), c.pad, (c.h, c.w))
    free = [t for t in range(c.T) if t not in frames]
    dec = gap[free] > R.DECIDE
    bad = int(((masks[free].long() != want[free]) & dec).sum())
    share = float(dec.double().mean())
    print(f"fused {frames} hard={hard}: decidable share {share:.4f}, {bad} decidable mismatches of {dec.numel()}")
    assert bad == 0 and share > 0.95
    assert torch.equal(masks[s0], torch.from_numpy(FC.rolled_maps(frames)[s0]))   # frame s_0 is its given map
    # the frames after s_m and the annotated frames: the call without the key
    plain = engine.propagate_masks_refs(c.feats, c.Hf, c.Wf, segs, c.pad, (c.h, c.w), cfg, engine.RefsConfig("both", "all")).cpu()
    same = list(frames) + list(range(sm + 1, c.T))
    assert torch.equal(masks[same], plain[same])
    mid = FC.between(frames)
    assert not torch.equal(masks[mid], plain[mid])                               # and the frames between two maps did change
    # the disagreement counts
    assert len(dis) == 1 and dis[0].is_cuda and dis[0].dtype == torch.int64 and dis[0].shape == (c.T,)
    got = dis[0].cpu()
    lo, hi = FC.disagree_bounds(*FC.passes_f64(small, c.T, fw, bw, hard), frames, c.T)
    print(f"fused {frames} hard={hard}: disagree {got.tolist()} within {lo.tolist()} .. {hi.tolist()}")
    assert bool((lo <= got).all()) and bool((got <= hi).all())
    assert int(got[mid].sum()) > 0 and int(got.sum()) == int(got[mid].sum())


# ---- the tracker API ------------------------------------------------------------------------------------------------------------------------
FUSE = dict(direction="both", override="all", fuse="linear")
READOUT = dict(type="guided", radius=2, sigma_space=1.0, sigma_range=0.1)


def _model(dev, **test_cfg):
    import fgvc_amd.mmpt_api as api
    cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True)
    cfg.update(test_cfg)
    torch.manual_seed(0)
    m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                  pool_type="none")), test_cfg=cfg)
    m.init_weights()
    return m.to(dev).eval()


def _api_clip(dev, T=7):
    """A 7-frame 64 x 64 clip and a complete two-object map that moves 2 pixels a frame."""
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, T, 64, 64, generator=g).to(dev)
    a = torch.zeros(64, 64, dtype=torch.long)
    a[8:30, 8:30], a[36:58, 20:44] = 1, 2
    return imgs, {t: torch.roll(a, (2 * t, 2 * t), dims=(0, 1)) for t in range(T)}, [dict(original_shape=(64, 64))]


def test_session_counters_results_and_next_frame(dev):
    from fgvc_amd import engine
    imgs, m, meta = _api_clip(dev)
    model = _model(dev, refs=FUSE)
    session = model.open_label_session(imgs, meta)
    assert session.last_disagree is None
    first = session.propagate({0: m[0], 6: m[6]})
    assert session.counters == dict(encodes=1, affinity_runs=1, sweeps=1) and set(session._sweeps) == {(0, "fw"), (6, "bw")}
    d1 = session.last_disagree
    assert d1.dtype == torch.int64 and d1.shape == (7,) and not d1.is_cuda and d1[0] == 0 and d1[6] == 0 and int(d1.sum()) > 0
    nxt = engine.next_frame_to_annotate_by(d1, {0, 6})
    assert nxt in range(1, 6) and int(d1[nxt]) == int(d1.max()) and nxt == int(d1.argmax())
    second = session.propagate({0: m[0], 3: m[3], 6: m[6]})
    assert session.counters == dict(encodes=1, affinity_runs=1, sweeps=2)        # a map strictly between: no encoder, no pair kernel, no merge
    assert set(session._sweeps) == {(0, "fw"), (6, "bw")}
    d2 = session.last_disagree
    assert int(d2[3]) == 0 and not torch.equal(d1, d2)
    fresh = model(test_mode=True, imgs=imgs, ref_seg_map={0: m[0], 3: m[3], 6: m[6]}, img_meta=meta)
    assert np.array_equal(second[0], fresh[0]) and model.last_confidence is None
    assert np.array_equal(first[0], model(test_mode=True, imgs=imgs, ref_seg_map={0: m[0], 6: m[6]}, img_meta=meta)[0])
    # the argument overrides the key, both ways
    off = _model(dev, refs=dict(direction="both", override="all"))
    s2 = off.open_label_session(imgs, meta)
    assert np.array_equal(s2.propagate({0: m[0], 3: m[3], 6: m[6]}, fuse="linear")[0], second[0]) and torch.equal(s2.last_disagree, d2)
    unfused = s2.propagate({0: m[0], 3: m[3], 6: m[6]})
    assert s2.last_disagree is None and not np.array_equal(unfused[0], second[0])
    with pytest.raises(ValueError, match="fuse='linear' needs direction='both' and override='all'"):
        s2.propagate({0: m[0], 3: m[3]}, fuse="linear", direction="forward")
    # one annotated frame: direction='both' itself, and nothing disagrees
    assert np.array_equal(session.propagate({3: m[3]})[0], s2.propagate({3: m[3]})[0])
    assert torch.equal(session.last_disagree, torch.zeros(7, dtype=torch.int64))
    session.close()
    s2.close()


def test_api_device_masks_raw_input_confidence_and_guided(dev):
    _, m, meta = _api_clip(dev)
    refs = {0: m[0], 3: m[3], 6: m[6]}
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (1, 1, 7, 64, 64, 3), generator=g, dtype=torch.uint8).to(dev)
    model = _model(dev, refs=dict(FUSE, confidence=True), masks="device", input=dict(type="rgb8"), readout=READOUT)
    out = model(test_mode=True, imgs=raw, ref_seg_map=refs, img_meta=meta)
    assert isinstance(out, list) and len(out) == 1 and out[0].is_cuda and out[0].dtype == torch.uint8 and out[0].shape == (7, 64, 64)
    assert torch.equal(out[0][0].cpu(), m[0].to(torch.uint8))
    lc = model.last_confidence
    assert set(lc) == {"conf", "stats", "frame_score", "disagree"}
    assert lc["conf"].shape == (7, 64, 64) and lc["stats"].shape == (7, 3, 2) and lc["frame_score"].shape == (7,)
    for f in range(7):
        assert torch.equal(lc["stats"][f, :, 0].cpu(), torch.bincount(out[0][f].flatten().long().cpu(), minlength=3))
    session = model.open_label_session(raw, meta)
    masks, conf, stats = session.propagate(refs, confidence=True)
    assert torch.equal(masks, out[0]) and torch.equal(conf, lc["conf"]) and torch.equal(stats, lc["stats"])
    d = session.last_disagree
    assert d.dtype == torch.int64 and not d.is_cuda and torch.equal(lc["disagree"], d) and int(d.sum()) > 0
    assert d[[0, 3, 6]].tolist() == [0, 0, 0]
    # the same call with the plain read-outs: other masks between the maps' edges, the same counts (they are taken on the rows)
    plain = _model(dev, refs=dict(FUSE, confidence=True), masks="device", input=dict(type="rgb8"))
    got = plain(test_mode=True, imgs=raw, ref_seg_map=refs, img_meta=meta)[0]
    assert torch.equal(plain.last_confidence["disagree"], d) and not torch.equal(got, out[0])
    bare = _model(dev, refs=FUSE, masks="device", input=dict(type="rgb8"))
    assert torch.equal(bare(test_mode=True, imgs=raw, ref_seg_map=refs, img_meta=meta)[0], got) and bare.last_confidence is None
    session.close()


def test_demo_tool_fuse(dev, tmp_path):
    from PIL import Image
    a = np.zeros((64, 64), np.uint8)
    a[8:30, 8:30], a[36:58, 20:44] = 1, 2
    for t in (0, 4):
        Image.fromarray(np.roll(a, (2 * t, 2 * t), axis=(0, 1))).save(tmp_path / f"M{t}.png")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demo.py"), "--synthetic", "6", "64", "64", "--task", "vos",
                        "--mask", "0", str(tmp_path / "M0.png"), "--mask", "4", str(tmp_path / "M4.png"), "--fuse", "--confidence",
                        "--strides", "1", "1", "1", "4", "--neighbor-range", "8", "--out", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert [f for f in sorted(os.listdir(out)) if f.startswith("frame_")] == [f"frame_{t:05d}.png" for t in range(6)]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("disagree: ")]
    assert len(line) == 1 and len(line[0].split()) == 7 and "annotate next by disagreement: frame" in r.stdout
    counts = [int(v) for v in line[0].split()[1:]]
    assert counts[0] == counts[4] == counts[5] == 0
    assert [f for f in sorted(os.listdir(out)) if f.startswith("conf_")] == [f"conf_{t:05d}.png" for t in range(6)]
    assert "frame_score: " in r.stdout and "annotate next: frame" in r.stdout
