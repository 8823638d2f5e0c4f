"""GPU tests of the object statistics kernel (fgvc_seg_object_stats_u8) against metrics.object_stats_host with `==`
on every case of tests/objects_cases.py, and of the tracker key test_cfg.objects = dict(stats=True): every word is an integer sum, minimum or
maximum, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import objects_cases as OC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _report(name, got, want):
    bad = (got != want).nonzero()
    first = tuple(bad[0].tolist()) if len(bad) else ()
    return f"{name}: {bad.shape[0]} words differ; first (frame, id, word) {bad[:4].tolist()}: got {got[first] if first else ''}, want {want[first] if first else ''}"


@pytest.mark.parametrize("h", OC.HEIGHTS)
@pytest.mark.parametrize("w", OC.WIDTHS)
def test_every_size_and_id_count_equals_the_contract(dev, w, h):
    from fgvc_amd import ops
    m = OC.sized(w, h)
    d = torch.from_numpy(np.array(m)).to(dev)
    for n in OC.N_IDS:
        got = ops.object_stats(d, n)
        assert got.dtype == torch.int64 and tuple(got.shape) == (m.shape[0], n, 8)
        want = torch.from_numpy(np.array(OC.expected_sized(w, h)[:, :n]))
        assert torch.equal(got.cpu(), want), _report(f"{m.shape} n_ids={n}", got.cpu(), want)


@pytest.mark.parametrize("name", list(OC.cases()))
def test_named_cases_equal_the_contract(dev, name):
    from fgvc_amd import ops
    m, n = OC.cases()[name]
    got = ops.object_stats(torch.from_numpy(np.array(m)).to(dev), n).cpu()
    want = torch.from_numpy(np.array(OC.expected(name)))
    assert torch.equal(got, want), _report(name, got, want)
    if "2p32" in name:
        assert int(got[0, 1, 5]) > 2 ** 32
    if name.startswith("middle_frame"):
        assert got[:, 3, 0].tolist() == [0, int(want[1, 3, 0]), 0] and not bool(got[0, 3].any()) and not bool(got[2, 3].any())


def test_strided_views_are_read_in_place(dev):
    from fgvc_amd import metrics, ops
    m = OC.run_map(4, 21, 83, 11)
    want = torch.from_numpy(metrics.object_stats_host(m, 6))
    big = torch.full((4, 21 + 5, 83 + 9), 4, dtype=torch.uint8, device=dev)         # id 4 all around the window: a stray read would count it
    big[:, 2:-3, 4:-5] = torch.from_numpy(m).to(dev)
    crop = big[:, 2:-3, 4:-5]
    assert not crop.is_contiguous()
    assert torch.equal(ops.object_stats(crop, 6).cpu(), want)
    assert torch.equal(ops.object_stats(crop[::2], 6).cpu(), want[::2])              # every second frame of the window
    two = torch.from_numpy(m).to(dev).repeat_interleave(2, 0)
    assert torch.equal(ops.object_stats(two[::2], 6).cpu(), want)
    unaligned = torch.from_numpy(m).to(dev).flatten()[1:1 + 3 * 21 * 83].view(3, 21, 83)       # rows that start at odd addresses
    assert torch.equal(ops.object_stats(unaligned, 6).cpu(),
                       torch.from_numpy(metrics.object_stats_host(unaligned.cpu().numpy(), 6)))


def test_out_between_guard_words_and_a_second_call(dev):
    from fgvc_amd import ops
    m, n = OC.cases()["ids_beyond_n_ids_2x9x63"]
    want = torch.from_numpy(np.array(OC.expected("ids_beyond_n_ids_2x9x63")))
    d = torch.from_numpy(np.array(m)).to(dev)
    buf = torch.full((2 * n * 8 + 16,), -7, device=dev, dtype=torch.int64)
    out = buf[8:-8].view(2, n, 8)
    assert ops.object_stats(d, n, out=out) is out
    host = buf.cpu()
    assert torch.equal(host[8:-8].view(2, n, 8), want) and bool((host[:8] == -7).all()) and bool((host[-8:] == -7).all())
    # the same buffer again with another map: nothing of the first call is left (an id that is absent now reads eight zeros)
    other = torch.zeros_like(d)
    other[1, 3:5, 10:20] = 2
    ops.object_stats(other, n, out=out)
    from fgvc_amd import metrics
    assert torch.equal(out.cpu(), torch.from_numpy(metrics.object_stats_host(other.cpu().numpy(), n)))
    assert not bool(out[:, 1].any()) and not bool(out[0, 2].any())
    with pytest.raises(ValueError, match="out"):
        ops.object_stats(d, n, out=torch.empty((2, n, 8), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="n_ids"):
        ops.object_stats(d, 257)
    with pytest.raises(ValueError, match="n_ids"):
        ops.object_stats(d, 0)
    with pytest.raises(TypeError, match="ids"):
        ops.object_stats(d.float(), n)
    assert tuple(ops.object_stats(d[:0], n).shape) == (0, n, 8)


# ---- the tracker key test_cfg.objects -------------------------------------------------------------------------------------------------------
def _model(dev, typ="VanillaTracker", **test_cfg):
    import fgvc_amd.mmpt_api as api
    cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True)
    cfg.update(test_cfg)
    torch.manual_seed(0)
    m = api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                        test_cfg=cfg)
    m.init_weights()
    return m.to(dev).eval()


def _clip(dev):
    """test_gpu_refs.py's clip: 5 frames of 64 x 64, objects 1 and 2 on frame 0, object 3 given on frame 2"""
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, 5, 64, 64, generator=g).to(dev)
    a = torch.zeros(64, 64, dtype=torch.long)
    a[8:30, 8:30], a[36:58, 20:44] = 1, 2
    b = torch.zeros(64, 64, dtype=torch.long)
    b[10:28, 36:60] = 3
    return imgs, a, b, [dict(original_shape=(64, 64))]


def _same_as_contract(model, masks, n_ids):
    from fgvc_amd import engine, metrics
    tr = model.last_objects
    assert isinstance(tr, engine.ObjectTracks) and tr.stats.is_cuda and tr.stats.dtype == torch.int64
    ids = masks.cpu().numpy() if torch.is_tensor(masks) else masks
    want = metrics.object_stats_host(ids.astype(np.uint8), n_ids)
    assert tuple(tr.stats.shape) == want.shape and np.array_equal(tr.stats.cpu().numpy(), want)
    return tr


@pytest.mark.parametrize("form", ["plain", "guided", "device"])
def test_key_on_the_plain_call(dev, form):
    imgs, a, _, meta = _clip(dev)
    extra = dict(guided=dict(readout=dict(type="guided")), device=dict(masks="device"), plain={})[form]
    ref = a[None].to(dev)
    base_model = _model(dev, **extra)
    base = base_model(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0]
    assert base_model.last_objects is None
    model = _model(dev, objects=dict(stats=True), **extra)
    assert model.last_objects is None
    out = model(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0]
    assert type(out) is type(base) and out.dtype == base.dtype                     # the return value does not change
    assert torch.equal(out, base) if torch.is_tensor(out) else np.array_equal(out, base)
    tr = _same_as_contract(model, out, 3)
    assert tr.present[0].tolist() == [True, True, True] and tr.boxes[0, 1].tolist() == [8, 8, 30, 30] and tr.boxes[0, 2].tolist() == [20, 36, 44, 58]


def test_key_with_refs_and_a_late_object(dev):
    imgs, a, b, meta = _clip(dev)
    refs = {0: a, 2: b}
    base = _model(dev, refs={})(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    model = _model(dev, refs=dict(confidence=True), objects=dict(stats=True))
    out = model(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    assert np.array_equal(out, base)
    tr = _same_as_contract(model, out, 4)
    assert tr.present[:2, 3].tolist() == [False, False] and tr.present[2, 3] and tr.boxes[2, 3].tolist() == [36, 10, 60, 28]
    assert np.isnan(tr.centroids[0, 3]).all() and tr.boxes[1, 3].tolist() == [0, 0, 0, 0]
    assert np.array_equal(tr.area, torch.as_tensor(model.last_confidence["stats"])[..., 0].cpu().numpy())
    # a session's propagate leaves the view on its model too; a call without the key clears nothing it never set
    session = model.open_label_session(imgs, meta)
    got = session.propagate({0: a}, confidence=False)[0]
    _same_as_contract(model, got, 3)
    with pytest.raises(ValueError, match="outside the clip"):
        session.propagate({7: a})
    assert model.last_objects is None                                  # a refused call does not leave the previous call's view behind
    session.close()
    fused = _model(dev, refs=dict(direction="both", override="all", fuse="linear"), objects=dict(stats=True), masks="device")
    out_f = fused(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    _same_as_contract(fused, out_f, 4)


def test_key_with_raw_input_and_its_refusals(dev):
    imgs, a, _, meta = _clip(dev)
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (1, 1, 5, 64, 64, 3), generator=g, dtype=torch.uint8).to(dev)
    model = _model(dev, input=dict(type="rgb8"), objects=dict(stats=True))
    out = model(test_mode=True, imgs=raw, ref_seg_map=a[None].to(dev), img_meta=meta)[0]
    _same_as_contract(model, out, 3)
    hr = _model(dev, typ="HRVanillaTracker", objects=dict(stats=True))
    out = hr(test_mode=True, imgs=imgs, ref_seg_map=a[None].to(dev), img_meta=meta)[0]
    _same_as_contract(hr, out, 3)
    with pytest.raises(ValueError, match="colour"):
        _model(dev, objects=dict(stats=True, colour=1))
    heat = torch.rand(1, 2, 64, 64).to(dev)
    for key in ("coords", "return_maps"):
        with pytest.raises(NotImplementedError, match="test_cfg.objects"):
            _model(dev, objects=dict(stats=True), **{key: True})(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)


# ---- the scorer and the demo tool ------------------------------------------------------------------------------------------------------------
def test_mean_box_iou_is_the_same_on_both_backends(dev):
    from fgvc_amd import metrics
    gt = OC.run_map(4, 33, 65, 21, ids=(0, 0, 1, 2, 3), max_run=12)
    pred = np.roll(gt, (1, 2), (1, 2))
    pred[3][pred[3] == 2] = 0                                          # an object the prediction lost: IoU 0 there
    host = metrics.mean_box_iou(gt, pred.astype(np.float64), 4)
    assert 0.0 < host < 1.0
    assert metrics.mean_box_iou(gt, pred.astype(np.float64), 4, backend="hip") == host
    assert metrics.mean_box_iou(torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev), 4, backend="hip") == host
    assert metrics.mean_box_iou(gt, gt, 4, backend="hip") == 1.0
    assert np.isnan(metrics.mean_box_iou(np.zeros((3, 5, 5), np.uint8), np.zeros((3, 5, 5), np.uint8), 2, backend="hip"))


def test_demo_tool_boxes_labels_trails_and_mot(dev, tmp_path):
    import importlib.util
    import os
    from PIL import Image
    from fgvc_amd import datasets, metrics, viz
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(root, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    a = np.zeros((64, 64), np.uint8)
    a[8:30, 8:30], a[36:58, 20:44] = 1, 2
    Image.fromarray(a).save(tmp_path / "A.png")
    argv = ["--synthetic", "5", "64", "64", "--task", "vos", "--first-mask", str(tmp_path / "A.png"), "--strides", "1", "1", "1", "4",
            "--neighbor-range", "8", "--box-labels", "--object-trails", "3", "--radius", "2", "--mot", str(tmp_path / "mot.txt"),
            "--out", str(tmp_path / "out")]
    r = demo.main(argv)
    tr = r["objects"]
    assert np.array_equal(tr.stats.cpu().numpy(), metrics.object_stats_host(r["ids"], 3))
    back = datasets.read_mot(tmp_path / "mot.txt")
    assert set(back) == {1, 2} and back[1][0] == (8, 8, 30, 30) and back[2][0] == (20, 36, 44, 58)
    # the painted frames are the host painter's: boxes with the overlay in one call, the centroid trails in a second one
    want = viz.render(r["frames"], ids=r["ids"], boxes=tr.boxes[:, 1:], box_visibles=tr.present[:, 1:], box_labels=[1, 2],
                      box_colors=viz.davis_palette()[1:3])
    tracks, vis = tr.centroid_tracks()
    want = viz.paint_trails(want, tracks[1:], vis[1:], colors=viz.davis_palette()[1:3], trail=3, radius=2)
    assert np.array_equal(r["rendered"], want)
    assert sorted(n for n in os.listdir(tmp_path / "out") if n.startswith("frame_")) == [f"frame_{i:05d}.png" for i in range(5)]
