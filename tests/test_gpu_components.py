"""GPU tests of the connected-component kernels (fgvc_seg_components_i32, fgvc_seg_clean_u8) against
metrics.components_host and metrics.clean_masks_host with `==` on every case of tests/components_cases.py, and of the tracker key
test_cfg.clean: labels, maps and statistics are integers, so there is no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

from tests import components_cases as CC

pytestmark = pytest.mark.gpu

KEY = dict(min_area=4, keep="largest", fill_holes=True)         # the spec of the tracker-key tests


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _same_labels(dev, m, want, conn, bg, what):
    from fgvc_amd import ops
    got = ops.seg_components(torch.from_numpy(np.array(m)).to(dev), conn, bg)
    assert got.dtype == torch.int32 and tuple(got.shape) == m.shape
    got = got.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.shape[0] == 0, f"{what} connectivity={conn} background={bg}: {bad.shape[0]} labels differ; first (t, y, x) {bad[:4].tolist()}: " \
                              f"got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"


def _same_clean(dev, m, n_ids, what, **kw):
    from fgvc_amd import metrics, ops
    want, want_stats = metrics.clean_masks_host(m, n_ids, **kw)
    dkw = dict(kw)
    if dkw.get("frames") is not None:
        dkw["frames"] = torch.from_numpy(np.asarray(dkw["frames"], bool)).to(dev)
    out, stats = ops.seg_clean(torch.from_numpy(np.array(m)).to(dev), n_ids, **dkw)
    assert out.dtype == torch.uint8 and stats.dtype == torch.int64 and tuple(stats.shape) == (m.shape[0], n_ids, 4)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    bad = np.argwhere(out != want)
    assert bad.shape[0] == 0, f"{what} {kw}: {bad.shape[0]} pixels differ; first (t, y, x) {bad[:4].tolist()}: got {out[tuple(bad[0])]}, " \
                              f"want {want[tuple(bad[0])]}"
    assert np.array_equal(stats, want_stats), f"{what} {kw}: stats differ at (t, id, word) {np.argwhere(stats != want_stats)[:4].tolist()}"
    return out, stats


def test_the_tile_is_the_one_the_cases_were_built_for(dev):
    from fgvc_amd import _lib, ops
    lib = _lib.load()
    assert (lib.fgvc_seg_ccl_tile_rows(), lib.fgvc_seg_ccl_tile_cols()) == (CC.TR, CC.TC) == ops.CCL_TILE


@pytest.mark.parametrize("h", CC.HEIGHTS)
@pytest.mark.parametrize("w", CC.WIDTHS)
def test_every_size_equals_the_contract(dev, w, h):
    m = CC.sized(w, h)
    for conn, bg in CC.VARIANTS:
        _same_labels(dev, m, CC.expected_sized(w, h, conn, bg), conn, bg, f"{m.shape}")
    for kw in CC.CLEAN_SWEEP:
        _same_clean(dev, m, 4, f"{m.shape}", **kw)                               # id 255 >= n_ids = 4: copied, takes part in nothing


@pytest.mark.parametrize("name", list(CC.cases()))
def test_named_component_cases_equal_the_contract(dev, name):
    m = CC.cases()[name]
    for conn, bg in CC.VARIANTS:
        _same_labels(dev, m, CC.expected(name, conn, bg), conn, bg, name)
    n_ids = 256 if name == "all_256_ids" else 8
    for kw in CC.CLEAN_SWEEP:
        _same_clean(dev, m, n_ids, name, **kw)


@pytest.mark.parametrize("name", list(CC.clean_cases()))
def test_clean_cases_equal_the_written_answers_and_the_contract(dev, name):
    c = CC.clean_cases()[name]
    out, stats = _same_clean(dev, c["ids"], c["n_ids"], name, **CC.clean_kwargs(c["kw"]))
    assert np.array_equal(out, c["want"]) and np.array_equal(stats, c["stats"])
    for keep in ("all", "largest"):
        for fill in (False, True):
            _same_clean(dev, c["ids"], c["n_ids"], name, **{**CC.clean_kwargs(c["kw"]), "keep": keep, "fill_holes": fill})


def test_strided_views_are_read_in_place(dev):
    from fgvc_amd import metrics, ops
    m = CC.run_map(4, CC.TR + 5, CC.TC + 19, 11, ids=(0, 0, 1, 2, 3))
    h, w = m.shape[1:]
    big = torch.full((4, h + 5, w + 9), 2, dtype=torch.uint8, device=dev)           # a live id all around the window: a stray read would join it
    big[:, 2:-3, 4:-5] = torch.from_numpy(m).to(dev)
    crop = big[:, 2:-3, 4:-5]
    assert not crop.is_contiguous()
    kw = dict(min_area=3, keep="largest", fill_holes=True)
    want_l = metrics.components_host(m, 8, True)
    want_o, want_s = metrics.clean_masks_host(m, 4, **kw)

    def check(view, sel):
        assert np.array_equal(ops.seg_components(view, 8, True).cpu().numpy(), want_l[sel])
        out, stats = ops.seg_clean(view, 4, **kw)
        assert np.array_equal(out.cpu().numpy(), want_o[sel]) and np.array_equal(stats.cpu().numpy(), want_s[sel])
    check(crop, slice(None))
    check(crop[::2], slice(None, None, 2))                                           # every second frame of the window
    assert bool((big[:, :2] == 2).all()) and bool((big[:, :, :4] == 2).all())        # the surround is as it was
    flat = torch.from_numpy(m).to(dev).flatten()
    odd = flat[1:1 + 3 * h * w].view(3, h, w)                                         # rows that start at odd addresses
    mo = odd.cpu().numpy()
    assert np.array_equal(ops.seg_components(odd, 4, False).cpu().numpy(), metrics.components_host(mo, 4, False))
    out, stats = ops.seg_clean(odd, 4, **kw)
    wo, ws = metrics.clean_masks_host(mo, 4, **kw)
    assert np.array_equal(out.cpu().numpy(), wo) and np.array_equal(stats.cpu().numpy(), ws)


def test_outputs_between_guard_bands_in_place_and_a_reused_workspace(dev):
    from fgvc_amd import metrics, ops
    T, h, w, n = 2, CC.TR + 3, CC.TC + 7, 4
    m = CC.run_map(T, h, w, 21, ids=(0, 0, 1, 2, 3, 255))
    d = torch.from_numpy(m).to(dev)
    kw = dict(min_area=3, keep="largest", fill_holes=True, max_hole_area=6)
    want_o, want_s = metrics.clean_masks_host(m, n, **kw)
    assert not np.array_equal(want_o, m)                                              # the rule changes this map
    px = T * h * w
    obuf = torch.full((px + 128,), 77, device=dev, dtype=torch.uint8)
    sbuf = torch.full((T * n * 4 + 16,), -7, device=dev, dtype=torch.int64)
    lbuf = torch.full((px + 32,), -9, device=dev, dtype=torch.int32)
    need = ops.seg_clean_workspace_bytes(T, h, w, n)
    assert need == T * n * 8 + px * 12
    ws = torch.full((need + 64,), 0xAB, device=dev, dtype=torch.uint8)                # stale contents must not matter
    out, stats = obuf[64:-64].view(T, h, w), sbuf[8:-8].view(T, n, 4)
    got = ops.seg_clean(d, n, out=out, stats=stats, workspace=ws[:need], **kw)
    assert got[0] is out and got[1] is stats
    assert np.array_equal(out.cpu().numpy(), want_o) and np.array_equal(stats.cpu().numpy(), want_s)
    assert bool((obuf[:64] == 77).all()) and bool((obuf[-64:] == 77).all()) and bool((sbuf[:8] == -7).all()) and bool((sbuf[-8:] == -7).all())
    assert bool((ws[need:] == 0xAB).all())
    labels = lbuf[16:-16].view(T, h, w)
    assert ops.seg_components(d, 8, False, out=labels) is labels
    assert np.array_equal(labels.cpu().numpy(), metrics.components_host(m, 8, False))
    assert bool((lbuf[:16] == -9).all()) and bool((lbuf[-16:] == -9).all())
    # the same workspace and outputs again for another map: nothing of the first call is left
    other = CC.run_map(T, h, w, 22, ids=(0, 1, 1, 2), max_run=4)
    ops.seg_clean(torch.from_numpy(other).to(dev), n, out=out, stats=stats, workspace=ws[:need], **kw)
    wo, wst = metrics.clean_masks_host(other, n, **kw)
    assert np.array_equal(out.cpu().numpy(), wo) and np.array_equal(stats.cpu().numpy(), wst)
    # in place
    same = d.clone()
    got = ops.seg_clean(same, n, out=same, **kw)
    assert got[0] is same and np.array_equal(same.cpu().numpy(), want_o) and np.array_equal(got[1].cpu().numpy(), want_s)
    # refusals
    with pytest.raises(ValueError, match="workspace"):
        ops.seg_clean(d, n, workspace=ws[:need - 1], **kw)
    with pytest.raises(ValueError, match="out"):
        ops.seg_clean(d, n, out=torch.empty((T, h, w + 1), device=dev, dtype=torch.uint8))
    with pytest.raises(ValueError, match="stats"):
        ops.seg_clean(d, n, stats=torch.empty((T, n, 4), device=dev, dtype=torch.int32))
    with pytest.raises(ValueError, match="out"):
        ops.seg_components(d, out=torch.empty((T, h, w), device=dev, dtype=torch.int64))
    for bad, word in ((dict(n_ids=0), "n_ids"), (dict(n_ids=257), "n_ids"), (dict(connectivity=6), "connectivity"), (dict(keep="biggest"), "keep"),
                      (dict(min_area=-1), "min_area"), (dict(max_hole_area=-1), "max_hole_area"),
                      (dict(frames=torch.ones(T + 1, dtype=torch.bool, device=dev)), "frames")):
        with pytest.raises(ValueError, match=word):
            ops.seg_clean(d, **{"n_ids": n, **bad})
    with pytest.raises(ValueError, match="connectivity"):
        ops.seg_components(d, 6)
    with pytest.raises(TypeError, match="ids"):
        ops.seg_clean(d.float(), n)
    with pytest.raises(TypeError, match="ids"):
        ops.seg_components(d.int())
    assert tuple(ops.seg_components(d[:0]).shape) == (0, h, w) and tuple(ops.seg_components(d[:, :0]).shape) == (T, 0, w)
    e_out, e_stats = ops.seg_clean(d[:, :, :0], n)
    assert tuple(e_out.shape) == (T, h, 0) and tuple(e_stats.shape) == (T, n, 4) and not bool(e_stats.any())


# ---- the tracker key test_cfg.clean ----------------------------------------------------------------------------------------------------------
def _model(dev, typ="VanillaTracker", **test_cfg):
    """test_gpu_objects.py's model builder"""
    import fgvc_amd.mmpt_api as api
    cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True)
    cfg.update(test_cfg)
    torch.manual_seed(0)
    m = api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")),
                        test_cfg=cfg)
    m.init_weights()
    return m.to(dev).eval()


def _clip(dev):
    """test_gpu_objects.py's clip: 5 frames of 64 x 64, objects 1 and 2 on frame 0, object 3 given on frame 2"""
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, 5, 64, 64, generator=g).to(dev)
    a = torch.zeros(64, 64, dtype=torch.long)
    a[8:30, 8:30], a[36:58, 20:44] = 1, 2
    b = torch.zeros(64, 64, dtype=torch.long)
    b[10:28, 36:60] = 3
    return imgs, a, b, [dict(original_shape=(64, 64))]


def _host(x):
    return (x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)).astype(np.uint8)


def _key_changes_something(base, produced):
    """non-vacuity: on some frame the rule covers, some id of the un-keyed output has more than one component"""
    from fgvc_amd import metrics
    lab = metrics.components_host(base)
    return any(len(np.unique(lab[t][base[t] == o])) > 1 for t in np.nonzero(produced)[0] for o in np.unique(base[t]) if o)


def _held_to_the_contract(model, out, base, n_ids, produced, objects=True):
    """the keyed call's output is the contract applied to the un-keyed output on the frames the rule covers, that output itself elsewhere;
    last_clean and last_objects describe it"""
    from fgvc_amd import engine, metrics
    base, got = _host(base), _host(out)
    want, want_stats = metrics.clean_masks_host(base, n_ids, frames=produced, **KEY)
    assert np.array_equal(got, want)
    assert np.array_equal(got[~produced], base[~produced])
    lc = model.last_clean
    assert lc["config"] == engine.CleanConfig(**KEY) and lc["stats"].is_cuda and lc["stats"].dtype == torch.int64
    assert np.array_equal(lc["stats"].cpu().numpy(), want_stats)
    if objects:
        assert np.array_equal(model.last_objects.stats.cpu().numpy(), metrics.object_stats_host(want, n_ids))
    return want


@pytest.mark.parametrize("form", ["plain", "guided", "device"])
def test_key_on_the_plain_call(dev, form):
    imgs, a, _, meta = _clip(dev)
    extra = dict(guided=dict(readout=dict(type="guided")), device=dict(masks="device"), plain={})[form]
    ref = a[None].to(dev)
    base_model = _model(dev, **extra)
    base = base_model(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0]
    assert base_model.last_clean is None                                             # without the key
    produced = np.arange(5) >= 1
    assert _key_changes_something(_host(base), produced)
    model = _model(dev, clean=dict(KEY), objects=dict(stats=True), **extra)
    assert model.last_clean is None
    out = model(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0]
    assert type(out) is type(base) and out.dtype == base.dtype and out.shape == base.shape          # the return form does not change
    want = _held_to_the_contract(model, out, base, 3, produced)
    assert not np.array_equal(want, _host(base))
    if form == "plain":
        # a spec that changes nothing: the un-keyed output, and no statistics
        idle = _model(dev, clean=dict(min_area=1))
        same = idle(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0]
        assert np.array_equal(same, base) and idle.last_clean["stats"] is None and not idle.last_clean["config"].active


def test_key_with_refs_a_late_object_and_a_session(dev):
    imgs, a, b, meta = _clip(dev)
    refs = {0: a, 2: b}
    base_model = _model(dev, refs=dict(confidence=True))
    base = base_model(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    raw_conf = base_model.last_confidence
    model = _model(dev, refs=dict(confidence=True), clean=dict(KEY), objects=dict(stats=True))
    out = model(test_mode=True, imgs=imgs, ref_seg_map=refs, img_meta=meta)[0]
    produced = np.arange(5) >= 1                                                     # frame 2's map was injected; its pixels are a read-out's
    assert _key_changes_something(_host(base), produced)
    _held_to_the_contract(model, out, base, 4, produced)
    assert np.array_equal(np.asarray(model.last_confidence["conf"]), np.asarray(raw_conf["conf"]))          # the raw read-out's
    assert np.array_equal(np.asarray(model.last_confidence["stats"]), np.asarray(raw_conf["stats"]))
    # direction='both' from a map on frame 2: frames 0 and 1 are the backward pass's, frame 2 is the given map
    both_base = _model(dev, refs=dict(direction="both"))(test_mode=True, imgs=imgs, ref_seg_map={2: a}, img_meta=meta)[0]
    both = _model(dev, refs=dict(direction="both"), clean=dict(KEY), objects=dict(stats=True))
    out = both(test_mode=True, imgs=imgs, ref_seg_map={2: a}, img_meta=meta)[0]
    _held_to_the_contract(both, out, both_base, 3, np.arange(5) != 2)
    fwd_base = _model(dev, refs={})(test_mode=True, imgs=imgs, ref_seg_map={2: a}, img_meta=meta)[0]
    fwd = _model(dev, refs={}, clean=dict(KEY))
    out = fwd(test_mode=True, imgs=imgs, ref_seg_map={2: a}, img_meta=meta)[0]
    _held_to_the_contract(fwd, out, fwd_base, 3, np.arange(5) > 2, objects=False)
    # a session's propagate
    session = model.open_label_session(imgs, meta)
    plain = _model(dev, refs={}).open_label_session(imgs, meta)
    got = session.propagate({0: a})[0]
    _held_to_the_contract(model, got, plain.propagate({0: a})[0], 3, produced)
    with pytest.raises(ValueError, match="outside the clip"):
        session.propagate({7: a})
    assert model.last_clean is None                                                  # a refused call does not leave the previous call's statistics behind
    session.close()
    plain.close()


def test_key_with_the_other_tracker_raw_input_and_its_refusals(dev):
    imgs, a, _, meta = _clip(dev)
    ref = a[None].to(dev)
    produced = np.arange(5) >= 1
    g = torch.Generator().manual_seed(5)
    raw = torch.randint(0, 256, (1, 1, 5, 64, 64, 3), generator=g, dtype=torch.uint8).to(dev)
    base = _model(dev, input=dict(type="rgb8"))(test_mode=True, imgs=raw, ref_seg_map=ref, img_meta=meta)[0]
    model = _model(dev, input=dict(type="rgb8"), clean=dict(KEY), objects=dict(stats=True))
    _held_to_the_contract(model, model(test_mode=True, imgs=raw, ref_seg_map=ref, img_meta=meta)[0], base, 3, produced)
    base = _model(dev, typ="HRVanillaTracker")(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0]
    hr = _model(dev, typ="HRVanillaTracker", clean=dict(KEY), objects=dict(stats=True))
    _held_to_the_contract(hr, hr(test_mode=True, imgs=imgs, ref_seg_map=ref, img_meta=meta)[0], base, 3, produced)
    with pytest.raises(ValueError, match="area"):
        _model(dev, clean=dict(area=3))
    with pytest.raises(ValueError, match="keep"):
        _model(dev, clean=dict(keep="biggest"))
    heat = torch.rand(1, 2, 64, 64).to(dev)
    for key in ("coords", "return_maps"):
        refused = _model(dev, clean=dict(KEY), **{key: True})
        with pytest.raises(NotImplementedError, match="test_cfg.clean"):
            refused(test_mode=True, imgs=imgs, ref_seg_map=heat, img_meta=meta)
        assert refused.last_clean is None


def test_demo_tool_clean_round_trip(dev, tmp_path):
    import importlib.util
    import os
    from PIL import Image
    from fgvc_amd import metrics
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fgvc_demo", os.path.join(root, "tools", "demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    a = np.zeros((64, 64), np.uint8)
    a[8:20, 8:20], a[8:24, 40:58], a[36:60, 16:48] = 1, 1, 2          # object 1 in two parts; object 2 with a hole
    a[44:52, 28:36] = 0
    Image.fromarray(a).save(tmp_path / "A.png")
    argv = ["--synthetic", "5", "64", "64", "--task", "vos", "--first-mask", str(tmp_path / "A.png"), "--strides", "1", "1", "1", "4",
            "--neighbor-range", "8", "--boxes"]
    raw = demo.main(argv + ["--out", str(tmp_path / "raw")])
    r = demo.main(argv + ["--clean", "--keep-largest", "--fill-holes", "--out", str(tmp_path / "clean")])
    want, want_stats = metrics.clean_masks_host(raw["ids"], 3, keep="largest", fill_holes=True, frames=np.arange(5) >= 1)
    assert np.array_equal(r["ids"], want) and not np.array_equal(want, raw["ids"])
    assert np.array_equal(r["objects"].stats.cpu().numpy(), metrics.object_stats_host(want, 3))        # the boxes are those of the cleaned ids
    assert np.array_equal(r["clean"]["stats"].cpu().numpy(), want_stats)
