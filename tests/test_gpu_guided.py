"""GPU tests of the edge-aware read-out (test_cfg.readout = dict(type='guided')): the kernels against the float64 rule
(engine.guided_readout_host) within the bound derived in tests/guided_cases.py, written between guard bands; the C entry's refusals; and
the tracker API (both trackers, test_cfg.refs, masks='device', raw input, the label session's counters, the refusals)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import guided_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 4096


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def test_library_constants_are_the_cases(dev):
    from fgvc_amd import _lib
    lib = _lib.load()
    assert lib.fgvc_guided_channel_chunk() == G.CHUNK
    assert (lib.fgvc_guided_tile_rows(), lib.fgvc_guided_tile_cols()) == G.TILE
    tiles = [c for c in G.CASES if c["out"][0] % G.TILE[0] and c["out"][1] % G.TILE[1]]
    assert len(tiles) >= 6                                                  # outputs that are no multiple of the tile in either direction
    assert {c["C"] for c in G.CASES} >= {1, 2, 5, G.CHUNK + 1, 256} and {c["radius"] for c in G.CASES} == {1, 2, 3}


def _banded(n, h0, w0, dev):
    """(whole buffer, the (n, h0, w0) view between two guard bands of 0xAB bytes)"""
    buf = torch.full((n * h0 * w0 + 2 * GUARD,), 0xAB, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + n * h0 * w0].view(n, h0, w0)


def _bands_untouched(buf):
    b = buf.cpu()
    return bool((b[:GUARD] == 0xAB).all()) and bool((b[-GUARD:] == 0xAB).all())


@pytest.mark.parametrize("case", G.CASES, ids=lambda c: c["name"])
def test_kernel_matches_the_float64_rule(dev, case):
    """Ids equal wherever the float64 margin exceeds 2 B (B: guided_cases.value_bound, derived there from the kernel's f32 arithmetic),
    confidence bytes within 1 there, statistics equal to what was written, guard bands untouched, at most 0.5 % of the pixels excluded."""
    from fgvc_amd import ops
    lab, guide, ref, B = G.reference(case)
    Hf, Wf, pad_shape, pad, out = G.geometry(case)
    n, C = case["n"], case["C"]
    kw = dict(norm=case["norm"], radius=case["radius"], sigma_space=case["sigma_space"], sigma_range=case["sigma_range"])
    d_lab, d_guide = lab.to(dev), guide.to(dev)
    mbuf, mview = _banded(n, *out, dev)
    cbuf, cview = _banded(n, *out, dev)
    masks, conf, stats = ops.seg_readout_guided(d_lab, d_guide, Hf, Wf, pad_shape, pad, out, conf=True, out=(mview, cview), **kw)
    assert masks.data_ptr() == mview.data_ptr() and conf.data_ptr() == cview.data_ptr()
    assert stats.shape == (n, C, 2) and stats.dtype == torch.int64
    assert _bands_untouched(mbuf) and _bands_untouched(cbuf)
    pbuf, pview = _banded(n, *out, dev)
    plain = ops.seg_readout_guided(d_lab, d_guide, Hf, Wf, pad_shape, pad, out, out=pview, **kw)
    assert _bands_untouched(pbuf) and torch.equal(plain, masks)            # one body: the form without confidence writes the same ids
    masks, conf, stats = masks.cpu(), conf.cpu(), stats.cpu()
    for f in range(n):
        ids = masks[f].flatten().long()
        assert int(ids.max()) < C
        assert torch.equal(stats[f, :, 0], torch.bincount(ids, minlength=C))
        assert torch.equal(stats[f, :, 1], torch.bincount(ids, weights=conf[f].flatten().double(), minlength=C).long())
    dec = G.decided(case, ref, B)
    excluded = 1.0 - float(dec.double().mean())
    bad = int(((masks != ref.ids) & dec).sum())
    worst = int((conf.int() - ref.conf.int()).abs()[dec].max()) if bool(dec.any()) else 0
    anywhere = int((masks != ref.ids).sum())
    print(f"{case['name']}: B = {B:.3e}, excluded share {excluded:.5f}, {bad} decided id mismatches ({anywhere} anywhere) of {dec.numel()}, "
          f"largest decided confidence difference {worst} level(s)")
    assert excluded <= G.EXCLUDED_MAX
    assert bad == 0
    assert worst <= 1
    if C == 1:
        assert bool((conf == 255).all()) and bool((masks == 0).all())
    if case["labels"] == "ties":
        assert not bool((masks == 2).any())                                 # channel 2 copies channel 1: the first maximum wins


@pytest.mark.parametrize("shape", [(1, 5, 7, 4), (3, 16, 24, 4), (2, 8, 12, 8), (1, 6, 10, 3)])
def test_guide_cells_are_the_block_means(dev, shape):
    """Each cell within (sy + sx - 1) roundings of the float64 mean (two in-order sums and one division)."""
    from fgvc_amd import ops
    n, Hf, Wf, s = shape
    g = torch.Generator().manual_seed(Hf)
    guide = torch.randn(n, 3, Hf * s, Wf * s, generator=g)
    buf = torch.full((n * Hf * Wf * 3 + 64,), float("nan"), device=dev)
    out = buf[32:-32].view(n, Hf * Wf, 3)
    got = ops.guide_cells(guide.to(dev), Hf, Wf, out=out).cpu()
    assert bool(torch.isnan(buf[:32]).all()) and bool(torch.isnan(buf[-32:]).all())
    want = guide.double().reshape(n, 3, Hf, s, Wf, s).mean((3, 5)).permute(0, 2, 3, 1).reshape(n, Hf * Wf, 3)
    bound = (2 * s - 1) * G.U * float(guide.abs().max())
    assert float((got.double() - want).abs().max()) <= bound


def test_entry_refusals(dev):
    from fgvc_amd import _lib, ops
    lab = torch.rand(1, 35, 2, device=dev)
    guide = torch.rand(1, 3, 20, 28, device=dev)
    geo = (5, 7, (20, 28), (0, 0, 0, 0), (20, 28))
    ops.seg_readout_guided(lab, guide, *geo)                                # the call itself is fine
    with pytest.raises(_lib.FgvcHipError, match="does not divide"):
        ops.seg_readout_guided(torch.rand(1, 42, 2, device=dev), guide, 6, 7, (20, 28), (0, 0, 0, 0), (20, 28),
                               cells=torch.rand(1, 42, 3, device=dev))
    with pytest.raises(_lib.FgvcHipError, match="does not divide"):
        ops.guide_cells(guide, 6, 7)
    for radius in (0, 4):
        with pytest.raises(_lib.FgvcHipError, match="radius"):
            ops.seg_readout_guided(lab, guide, *geo, radius=radius)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(_lib.FgvcHipError, match="sigma_space"):
            ops.seg_readout_guided(lab, guide, *geo, sigma_space=bad)
        with pytest.raises(_lib.FgvcHipError, match="sigma_range"):
            ops.seg_readout_guided(lab, guide, *geo, sigma_range=bad)
    with pytest.raises(_lib.FgvcHipError, match="outside 1..256"):
        ops.seg_readout_guided(torch.rand(1, 35, 257, device=dev), guide, *geo)
    with pytest.raises(_lib.FgvcHipError, match="inside the padded frame"):
        ops.seg_readout_guided(lab, guide, 5, 7, (20, 28), (0, 30, 0, 0), (20, 28))
    with pytest.raises(ValueError, match="guide"):
        ops.seg_readout_guided(lab, guide[:, :, :16], *geo)                 # a guide of another size than pad_shape
    with pytest.raises(ValueError, match="cells"):
        ops.seg_readout_guided(lab, guide, *geo, cells=torch.rand(1, 34, 3, device=dev))
    with pytest.raises(_lib.FgvcHipError, match="footprint"):
        ops.seg_readout_guided(torch.rand(1, 64 * 256, 2, device=dev), torch.rand(1, 3, 256, 1024, device=dev), 64, 256, (256, 1024),
                               (0, 0, 0, 0), (8, 32))                       # a 32-column tile would span the whole 256-cell row
    import ctypes
    null, one = ctypes.c_void_p(0), ctypes.c_void_p(lab.data_ptr())
    head = (1, 5, 7, 2, 20, 28, 0, 0, 20, 28, 20, 28, 1, 2, 1.0, 0.1)
    with pytest.raises(_lib.FgvcHipError, match="null pointer"):
        _lib.call("fgvc_seg_readout_guided_u8", one, null, one, *head, one, one, null)
    with pytest.raises(_lib.FgvcHipError, match="null conf / stats"):
        _lib.call("fgvc_seg_readout_guided_conf_u8", one, one, one, *head, one, null, one, one, null)
    with pytest.raises(_lib.FgvcHipError, match="one buffer"):
        _lib.call("fgvc_seg_readout_guided_conf_u8", one, one, one, *head, one, one, one, one, null)
    with pytest.raises(_lib.FgvcHipError, match="workspace"):
        _lib.call("fgvc_seg_readout_guided_u8", one, one, one, *head, one, null, null)


# ---- the tracker API ---------------------------------------------------------------------------------------------------------------------------
VT = dict(typ="VanillaTracker", strides=(1, 1, 1, 4), cfg=dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True,
                                                               with_first_neighbor=True))
HR = dict(typ="HRVanillaTracker", strides=(1, 1, 1, 4), cfg=dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8))
READOUT = dict(type="guided", radius=2, sigma_space=1.0, sigma_range=0.1)


def _model(dev, spec=VT, strides=None, **test_cfg):
    import fgvc_amd.mmpt_api as api
    torch.manual_seed(0)
    m = api.build_model(dict(type=spec["typ"], backbone=dict(type="ResNet", depth=18, strides=strides or spec["strides"], out_indices=(2,),
                                                             pool_type="none")), test_cfg=dict(spec["cfg"], **test_cfg))
    m.init_weights()
    return m.to(dev).eval()


def _clip(dev, h=48, w=64):
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, 5, h, w, generator=g).to(dev)
    a = torch.zeros(h, w, dtype=torch.long)
    a[6:22, 8:30], a[26:44, 20:44] = 1, 2
    b = torch.zeros(h, w, dtype=torch.long)
    b[10:28, 36:60] = 3
    return imgs, a, b, [dict(original_shape=(h, w))]


@pytest.mark.parametrize("spec", [VT, HR], ids=lambda s: s["typ"])
def test_bilinear_is_the_call_without_the_key_and_guided_is_the_kernel(dev, spec):
    from fgvc_amd import engine, ops
    imgs, a, _, meta = _clip(dev)
    seg = a[None].to(dev)
    base = _model(dev, spec)(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)[0]
    same = _model(dev, spec, readout=dict(type="bilinear"))(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)[0]
    assert base.dtype == np.float64 and np.array_equal(base, same)
    model = _model(dev, spec, readout=READOUT, masks="device")
    got = model(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)[0]
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (5, 48, 64)
    assert np.array_equal(got[0].cpu().numpy(), base[0])                    # frame 0 stays the given map
    # the same bank and frames through the op
    cfg = model._label_config()
    frames, _, pad = model._label_frames(imgs)
    feats, Hf, Wf = model._label_feats(frames, index_map=True)
    segp = torch.nn.functional.pad(seg[0].to(torch.uint8), pad).contiguous()
    C = int(ops.seg_max_label(segp, Hf, Wf).item()) + 1
    bank = torch.zeros((5, Hf * Wf, C), device=dev)
    ops.seg_onehot_labels(segp, Hf, Wf, C, out=bank[0])
    sw = engine.label_affinity(feats, Hf, Wf, 5, cfg, model.feat_channels)
    engine._sweep_labels(bank, bank, sw, Hf, Wf, False)
    guide = frames.float().contiguous()
    want = ops.seg_readout_guided(bank[1:], guide[1:], Hf, Wf, tuple(frames.shape[-2:]), pad, (48, 64), cfg.norm_mask, 2, 1.0, 0.1)
    assert torch.equal(got[1:], want)
    assert C == 3 and not torch.equal(got[1:], torch.from_numpy(base[1:]).to(dev, torch.uint8))    # and it is another read-out than the plain one


def test_refs_device_masks_raw_input_and_session(dev):
    imgs, a, b, meta = _clip(dev)
    refs = {0: a, 2: b}
    model = _model(dev, readout=READOUT, refs=dict(direction="both", confidence=True), masks="device")
    out = model(test_mode=True, imgs=imgs, ref_seg_map={2: b}, img_meta=meta)
    assert out[0].is_cuda and out[0].dtype == torch.uint8 and int(out[0][:2].max()) > 0       # frames before the annotated one are labelled
    lc = model.last_confidence
    assert lc["conf"].shape == (5, 48, 64) and lc["stats"].shape == (5, 4, 2)
    for f in range(5):
        assert torch.equal(lc["stats"][f, :, 0].cpu(), torch.bincount(out[0][f].flatten().long().cpu(), minlength=4))
    fwd = _model(dev, readout=READOUT, refs=dict(direction="forward"))
    plain = _model(dev, refs=dict(direction="forward"))
    got = fwd(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    base = plain(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    assert got.shape == base.shape == (5, 48, 64) and np.array_equal(got[0], base[0]) and 3 in np.unique(got[2:])
    assert not np.array_equal(got[1:], base[1:])
    one = _model(dev, readout=READOUT)(test_mode=True, imgs=imgs, ref_seg_map=a[None].to(dev), img_meta=meta)[0]
    assert np.array_equal(fwd(test_mode=True, imgs=imgs, ref_seg_map={0: a}, img_meta=meta)[0], one)    # {0: map} is the call without refs
    # a session: the second propagate launches no encoder, no pair kernel and no merge
    session = fwd.open_label_session(imgs, meta)
    first = session.propagate({0: a})
    assert session.counters == dict(encodes=1, affinity_runs=1, sweeps=1) and np.array_equal(first[0], one)
    second = session.propagate(refs)
    assert session.counters == dict(encodes=1, affinity_runs=1, sweeps=2) and np.array_equal(second[0], got)
    session.close()
    assert session.guide is None and session.cells is None
    # raw rgb8 frames
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (1, 1, 5, 48, 64, 3), generator=g, dtype=torch.uint8).to(dev)
    m_raw = _model(dev, readout=READOUT, input=dict(type="rgb8"))
    r = m_raw(test_mode=True, imgs=raw, ref_seg_map=a[None].to(dev), img_meta=meta)[0]
    assert r.shape == (5, 48, 64) and np.array_equal(r[0], a.numpy().astype(np.float64))
    r_plain = _model(dev, input=dict(type="rgb8"))(test_mode=True, imgs=raw, ref_seg_map=a[None].to(dev), img_meta=meta)[0]
    assert not np.array_equal(r[1:], r_plain[1:])


def _tool(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_demo_tool_edge_aware(dev, tmp_path):
    """tools/demo.py --task vos --edge-aware runs end to end (one process); its flags are refused elsewhere (the parser, in this process)."""
    from PIL import Image
    a = np.zeros((48, 64), np.uint8)
    a[8:30, 8:30] = 1
    Image.fromarray(a).save(tmp_path / "A.png")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "demo.py"), "--synthetic", "4", "48", "64", "--task", "vos",
                        "--first-mask", str(tmp_path / "A.png"), "--strides", "1", "1", "1", "4", "--neighbor-range", "8",
                        "--edge-aware", "--edge-radius", "1", "--edge-sigma-range", "0.2", "--out", str(tmp_path / "edge")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert [f for f in sorted(os.listdir(tmp_path / "edge")) if f.endswith(".png")] == [f"frame_{t:05d}.png" for t in range(4)]
    demo = _tool("demo")
    ok = demo.parse_args(["--synthetic", "4", "48", "64", "--task", "vos", "--first-mask", "A.png", "--edge-aware", "--out", "o"])
    assert ok.edge_aware and ok.edge_radius == 2 and ok.edge_sigma_range == 0.1
    for argv in (["--task", "points", "--query-points", "0", "5", "5", "--edge-aware"], ["--task", "vos", "--first-mask", "A.png", "--edge-radius", "3"]):
        with pytest.raises(SystemExit):
            demo.parse_args(["--synthetic", "4", "48", "64", "--out", "o", *argv])


def test_test_tool_readout_guided(dev, tmp_path):
    """tools/test.py --task vos --readout guided scores a fake DAVIS tree."""
    _tool("make_fake_davis").make(str(tmp_path / "davis"), sequences=1, frames=4, size=(48, 64), objects=2, seed=1)
    out = tmp_path / "out.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "test.py"), "--task", "vos", "--data-root", str(tmp_path / "davis"),
                        "--readout", "guided", "--out", str(out)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert 0.0 <= json.loads(out.read_text())["J&F-Mean"] <= 1.0


def test_api_refusals(dev):
    imgs, a, _, meta = _clip(dev)
    heat = torch.rand(1, 2, 48, 64, device=dev)
    with pytest.raises(ValueError, match="type='box'"):
        _model(dev, readout=dict(type="box"))
    with pytest.raises(ValueError, match="sigma"):
        _model(dev, readout=dict(type="guided", sigma=2))
    for key in ("coords", "return_maps"):
        with pytest.raises(NotImplementedError, match="readout"):
            _model(dev, readout=READOUT, **{key: True})(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
    with pytest.raises(NotImplementedError, match="readout.*save_np"):
        _model(dev, readout=READOUT, save_np=True)(test_mode=True, imgs=imgs, ref_seg_map=a[None].to(dev), img_meta=meta)
    # HRVanillaTracker's grid is what its encoder makes of the frame: 50 x 66 at stride 4 gives 13 x 17, which does not divide it
    imgs2, a2, _, meta2 = _clip(dev, 50, 66)
    with pytest.raises(NotImplementedError, match="does not divide"):
        _model(dev, HR, strides=(1, 2, 1, 1), readout=READOUT)(test_mode=True, imgs=imgs2, ref_seg_map=a2[None].to(dev), img_meta=meta2)
