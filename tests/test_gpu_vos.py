"""GPU tests of the segmentation-mask path (semi-supervised VOS): the frame-0 label kernels against Pillow + F.one_hot, the read-out
kernel against a float64 torch restatement of vanilla_tracker.py:773-802, hard propagation, the engine's whole clip against a float64
restatement driven by the same top-k lists, and the tracker API / DAVIS adapter / J&F end to end on a synthetic DAVIS set.

"Decidable" pixel: the float64 top-two (normalised) channel values differ by more than 1e-5; the kernel's f32 arithmetic must give the
float64 answer there and may differ elsewhere.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DECIDE = 1e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def pil_nearest(a: np.ndarray, Hf: int, Wf: int) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize((Wf, Hf), Image.NEAREST))


# ---- float64 restatement of the read-out (step 6) ---------------------------------------------------------------------------
def readout_f64(labels, Hf, Wf, pad_shape, pad, out_shape, norm=True):
    """labels (n, HfWf, C) -> (argmax (n, h0, w0) int64, top-two gap (n, h0, w0)) in float64 with torch's own operators."""
    n, _, C = labels.shape
    x = labels.double().reshape(n, Hf, Wf, C).permute(0, 3, 1, 2)
    x = F.interpolate(x, size=pad_shape, mode="bilinear", align_corners=False)
    lw, uw, lh, uh = pad
    x = x[:, :, lh:pad_shape[0] - uh, lw:pad_shape[1] - uw]
    x = F.interpolate(x, size=out_shape, mode="bilinear", align_corners=False)
    if norm:
        mn = x.flatten(2).min(-1)[0][..., None, None]
        mx = x.flatten(2).max(-1)[0][..., None, None]
        x = torch.where(mx > 0, (x - mn) / (mx - mn + 1e-12), x)
    top2 = x.topk(min(2, C), dim=1).values
    gap = (top2[:, 0] - top2[:, 1]) if C > 1 else torch.full_like(top2[:, 0], float("inf"))
    return x.argmax(1), gap


def _labels(n, Hf, Wf, C, g):
    lab = torch.rand(n, Hf * Wf, C, generator=g, dtype=torch.float64)
    lab = lab ** 3                                     # peaked, like propagated one-hot labels
    if C > 2:
        lab[..., -1] -= 0.9                            # a channel whose maximum is <= 0: not normalised
        lab[..., -1] = lab[..., -1].clamp_max(-1e-3)
    return lab.float()


@pytest.mark.parametrize("hw, Hf_Wf", [((64, 72), (16, 18)), ((62, 70), (31, 35)), ((100, 100), (33, 27)), ((480, 854), (240, 427)),
                                       ((7, 9), (3, 5)), ((37, 50), (37, 50))])
@pytest.mark.parametrize("n_ids", [1, 4, 12])
def test_onehot_labels_match_pillow(dev, hw, Hf_Wf, n_ids):
    from fgvc_amd import ops
    rng = np.random.default_rng(hw[0] * 7 + n_ids)
    a = rng.integers(0, n_ids, hw, dtype=np.uint8)
    Hf, Wf = Hf_Wf
    small = pil_nearest(a, Hf, Wf)
    m = torch.from_numpy(a).to(dev)
    mx = int(ops.seg_max_label(m, Hf, Wf).item())
    assert mx == int(small.max())
    C = mx + 1
    want = F.one_hot(torch.from_numpy(small.astype(np.int64)), C).reshape(Hf * Wf, C).float()
    got = ops.seg_onehot_labels(m, Hf, Wf, C).cpu()
    assert torch.equal(got, want)


def test_onehot_labels_single_channel(dev):
    from fgvc_amd import ops
    m = torch.zeros(30, 41, dtype=torch.uint8, device=dev)
    assert int(ops.seg_max_label(m, 13, 17).item()) == 0
    assert torch.equal(ops.seg_onehot_labels(m, 13, 17, 1).cpu(), torch.ones(13 * 17, 1))


def test_hard_onehot_exact(dev):
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(3)
    x = torch.rand(5, 777, 11, generator=g)
    x[0, :50, 3] = x[0, :50, 7] = 2.0                 # ties: the first maximum wins
    want = F.one_hot(x.argmax(-1), 11).float()
    xd = x.to(dev)
    assert torch.equal(ops.seg_hard_onehot(xd).cpu(), want)
    ops.seg_hard_onehot(xd, out=xd)                   # in place
    assert torch.equal(xd.cpu(), want)
    assert torch.equal(want[0, :50].argmax(-1), torch.full((50,), 3))


READOUT_CASES = [
    # (n, Hf, Wf, C, pad_shape, pad (l, r, t, b), out_shape)
    (3, 240, 427, 11, (480, 854), (0, 0, 0, 0), (480, 854)),            # DAVIS 480p, stride 2, no padding
    (2, 16, 18, 3, (64, 72), (1, 1, 1, 1), (62, 70)),                   # 62 x 70 padded to 64 x 72 (stride 4)
    (2, 16, 18, 3, (64, 72), (1, 1, 1, 1), (50, 90)),                   # original_shape different from the unpadded size
    (2, 31, 35, 1, (62, 70), (0, 0, 0, 0), (62, 70)),                   # C = 1
    (2, 20, 19, 2, (80, 76), (1, 2, 0, 1), (93, 61)),                   # C = 2, uneven padding, up- and down-sampling
]


@pytest.mark.parametrize("case", READOUT_CASES, ids=lambda c: f"{c[1]}x{c[2]}C{c[3]}to{c[6][0]}x{c[6][1]}")
@pytest.mark.parametrize("norm", [True, False])
def test_readout_matches_float64_restatement(dev, case, norm):
    from fgvc_amd import ops
    n, Hf, Wf, C, pad_shape, pad, out_shape = case
    g = torch.Generator().manual_seed(Hf * 31 + C)
    lab = _labels(n, Hf, Wf, C, g)
    got = ops.seg_readout(lab.to(dev), Hf, Wf, pad_shape, pad, out_shape, norm).cpu().long()
    want, gap = readout_f64(lab, Hf, Wf, pad_shape, pad, out_shape, norm)
    assert got.shape == want.shape == (n, *out_shape)
    dec = gap > DECIDE
    bad = int(((got != want) & dec).sum())
    print(f"read-out {case} norm={norm}: {int((~dec).sum())} undecidable of {dec.numel()} pixels, {bad} decidable mismatches")
    assert bad == 0
    assert dec.float().mean() > 0.95


# ---- the engine's whole clip against a float64 restatement on the same top-k lists --------------------------------------------
def _clip(dev, T, C_feat, Hf, Wf, seed):
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(1, C_feat, Hf, Wf, generator=g)
    feats = torch.cat([torch.roll(base, shifts=(t, t), dims=(2, 3)) + 0.3 * torch.randn(1, C_feat, Hf, Wf, generator=g)
                       for t in range(T)])
    from fgvc_amd import ops
    return ops.normalize_to_hwc(feats.to(dev))


def _restate_clip(tk, plan, bank0, T, hard):
    """Propagation in float64 from the kernels' lists: labels[f] = sum_k weight * bank[slot_frame[slot], pixel]."""
    HW, C = bank0.shape
    bank = torch.zeros(T, HW, C, dtype=torch.float64)
    soft = torch.zeros_like(bank)
    bank[0] = bank0.double()
    for f in range(1, T):
        row = tk.row(plan.out_rows[(0, f)])
        idx = tk.idx[row].cpu().long()
        w = tk.weight[row].cpu().double()
        sf = tk.slot_frame[row].cpu().long()
        slot, pix = idx // HW, idx % HW
        soft[f] = (w[..., None] * bank[sf[slot], pix]).sum(1)
        bank[f] = F.one_hot(soft[f].argmax(-1), C).double() if hard else soft[f]
    return soft


@pytest.mark.parametrize("hard", [False, True])
def test_propagate_masks_matches_restatement(dev, hard):
    from fgvc_amd import engine
    T, h, w, d = 8, 62, 70, 2
    (hp, wp), pad = engine.pad_divide_by(h, w, d)
    Hf, Wf = hp // d, wp // d
    feats = _clip(dev, T, 64, Hf, Wf, 11)
    seg = np.zeros((h, w), np.uint8)
    seg[10:30, 8:30], seg[35:55, 20:45], seg[5:25, 40:66] = 1, 2, 3
    seg_p = np.pad(seg, ((pad[2], pad[3]), (pad[0], pad[1])))
    cfg = engine.TrackerConfig(neighbor_range=8, precede_frames=3, hard_prop=hard)
    masks = engine.propagate_masks(feats, Hf, Wf, torch.from_numpy(seg_p).to(dev), pad, (h, w), cfg).cpu()
    assert masks.shape == (T, h, w) and masks.dtype == torch.uint8
    assert torch.equal(masks[0], torch.from_numpy(seg))                                   # frame 0: the given map
    plan = engine.plan_clip(T, [0], cfg)
    tk = engine.run_affinity(feats, Hf, Wf, plan, cfg)
    small = pil_nearest(seg_p, Hf, Wf)
    bank0 = F.one_hot(torch.from_numpy(small.astype(np.int64)), int(small.max()) + 1).reshape(Hf * Wf, -1)
    soft = _restate_clip(tk, plan, bank0, T, hard)
    want, gap = readout_f64(soft[1:], Hf, Wf, (hp, wp), pad, (h, w), True)
    dec = gap > DECIDE
    bad = int(((masks[1:].long() != want) & dec).sum())
    print(f"propagate_masks hard={hard}: {int((~dec).sum())} undecidable, {bad} decidable mismatches of {dec.numel()}")
    assert bad == 0                                   # hard propagation included (it re-quantises every frame's bank row)


def test_highest_id_vanishing_at_feature_resolution(dev):
    """C = 1 + the largest id of the DOWNSAMPLED map: an object too small to survive the Pillow-nearest sample never appears."""
    from fgvc_amd import engine
    T, h, w = 4, 40, 48
    (hp, wp), pad = engine.pad_divide_by(h, w, 2)
    Hf, Wf = hp // 2, wp // 2
    seg = np.zeros((h, w), np.uint8)
    seg[4:20, 4:20] = 1
    seg[30, 32] = 2                                   # even row and column: the stride-2 nearest sample reads odd ones
    assert pil_nearest(seg, Hf, Wf).max() == 1
    feats = _clip(dev, T, 64, Hf, Wf, 2)
    masks = engine.propagate_masks(feats, Hf, Wf, torch.from_numpy(seg).to(dev), pad, (h, w),
                                   engine.TrackerConfig(neighbor_range=8)).cpu()
    assert int(masks[1:].max()) <= 1 and int(masks[0].max()) == 2


# ---- tracker API, DAVIS adapter, J&F ------------------------------------------------------------------------------------------
def _model(dev, **test_cfg):
    import fgvc_amd.mmpt_api as api
    cfg = dict(precede_frames=3, topk=10, temperature=0.07, neighbor_range=8, with_first=True, with_first_neighbor=True)
    cfg.update(test_cfg)
    torch.manual_seed(0)
    m = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                   pool_type="none")), test_cfg=cfg)
    m.init_weights()
    return m.to(dev).eval()


def test_api_and_davis_adapter_end_to_end(dev, tmp_path):
    import importlib.util
    import os
    from fgvc_amd import engine, metrics
    from fgvc_amd.datasets import Davis2017, davis_evaluate
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_fake_davis", os.path.join(root, "tools", "make_fake_davis.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    mk.make(str(tmp_path), sequences=2, frames=6, size=(61, 75), objects=3, seed=1)
    ds = Davis2017(str(tmp_path), device=dev)
    model = _model(dev)
    assert model.output_stride() == 2
    data, meta = ds[0]
    out = model(test_mode=True, **data)
    assert isinstance(out, list) and len(out) == 1
    pred = out[0]
    assert pred.dtype == np.float64 and pred.shape == meta["gt"].shape
    assert np.array_equal(pred[0], meta["gt"][0].astype(np.float64))
    # the engine's uint8 masks are the API's float64 ids
    cfg = model.engine_config()
    (hp, wp), pad = engine.pad_divide_by(61, 75, 2)
    frames = F.pad(data["imgs"][0, 0], pad).transpose(0, 1)
    feats, Hf, Wf = model.get_feats_hwc(frames, split=True)
    seg = F.pad(data["ref_seg_map"][0], pad).contiguous()
    masks = engine.propagate_masks(feats, Hf, Wf, seg, pad, (61, 75), cfg, channels=model.feat_channels)
    assert np.array_equal(masks.cpu().numpy().astype(np.float64), pred)
    # the tracker follows the moving objects: far better than the all-background answer
    jf = davis_evaluate(model, ds)
    print("J&F on the synthetic set:", jf)
    assert 0.0 <= jf["J&F-Mean"] <= 1.0 and set(jf["sequences"]) == set(ds.sequences)
    none = metrics.davis_jf({meta["name"]: (meta["gt"], np.zeros_like(meta["gt"]))})
    assert jf["sequences"][meta["name"]]["J&F"] > none["J&F-Mean"] + 0.3


def test_api_hard_prop_and_norm_mask_keys(dev):
    from fgvc_amd import engine
    model = _model(dev, hard_prop=True, norm_mask=False)
    cfg = model.engine_config()
    assert cfg.hard_prop is True and cfg.norm_mask is False
    g = torch.Generator().manual_seed(4)
    imgs = torch.randn(1, 1, 3, 5, 40, 44, generator=g).to(dev)
    seg = torch.zeros(1, 40, 44, dtype=torch.long)
    seg[0, 5:20, 5:20], seg[0, 22:38, 20:40] = 1, 2
    out = model(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(40, 44))])[0]
    assert out.shape == (5, 40, 44) and set(np.unique(out)) <= {0.0, 1.0, 2.0}
    # the points path is unchanged by the dispatch
    with pytest.raises(TypeError):
        model(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(40, 44))],
              rgbs=imgs[0, 0].transpose(0, 1)[None], query_points=torch.zeros(1, 1, 3, device=dev))
    assert engine.TrackerConfig().hard_prop is False and engine.TrackerConfig().norm_mask is True


# ---- end to end against the reference's own mask path (tests/golden/vos_*.npz, tests/golden/gen_golden_vos.py) --------------------
VOS_FIXTURES = ["vos_8x62x70", "vos_hard_8x62x70", "vos_vanish_5x41x47"]
# Mismatched pixels of frames 1.. under the DEFAULT arithmetic (f16 + FP6 encoder trunk, f16 + FP6 pair kernel with the refining
# merge), which is not index-exact on every top-k list: the bound is the figure of the first MI355X run of this test, per fixture
# (0 of 30 380, 0 of 30 380, 0 of 9 360 pixels; the f16x3 run of the same fixtures: 0 decidable mismatches, 0 undecidable pixels).
DEFAULT_MISMATCH_BOUND = {"vos_8x62x70": 0, "vos_hard_8x62x70": 0, "vos_vanish_5x41x47": 0}


def _fixture_run(dev, golden, name, arith, pair_split_fmt=None):
    import json
    from oracle import fgvc_oracle as O
    import fgvc_amd.mmpt_api as api
    g = golden(name)
    cfg = json.loads(str(g["test_cfg"]))
    if pair_split_fmt is not None:
        cfg["pair_split_fmt"] = pair_split_fmt
    model = api.build_model(dict(type="VanillaTracker", backbone=dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,),
                                                                       pool_type="none")), train_cfg=None, test_cfg=api.ConfigDict(**cfg))
    model.backbone.load_state_dict(O.seeded_resnet_state(int(g["seed"]), (1, 1, 1, 4), "none"), strict=False)
    model = model.to(dev).eval()
    model.backbone.set_arith(arith)
    imgs = torch.from_numpy(g["imgs"].astype(np.float32)).permute(0, 2, 1, 3, 4).unsqueeze(1).contiguous().to(dev)   # (1,1,3,T,h,w)
    seg = torch.from_numpy(g["ref_seg_map"]).unsqueeze(0).to(dev)
    meta = [dict(original_shape=tuple(int(v) for v in g["original_shape"]))]
    out = model(test_mode=True, imgs=imgs, ref_seg_map=seg, img_meta=meta)
    assert isinstance(out, list) and len(out) == 1 and out[0].shape == g["masks"].shape
    return g, out[0]


@pytest.mark.parametrize("name", VOS_FIXTURES)
def test_mask_path_f16x3_matches_reference_fixture(dev, golden, name):
    """The reference's forward_test_backward_save_mem (VanillaTracker's affinity) against the tracker API on the f16x3 arithmetic
    (set_arith('f16x3'), pair_split_fmt='f16': 1e-7-grade features and scores): frame 0 exact, every decidable pixel equal (the
    fixture's gap = the reference's top-two normalised values, > 1e-5)."""
    g, pred = _fixture_run(dev, golden, name, "f16x3", "f16")
    want = g["masks"]
    assert np.array_equal(pred[0], want[0].astype(np.float64))
    dec = g["gap"] > DECIDE
    bad = int(((pred[1:] != want[1:]) & dec).sum())
    print(f"{name} f16x3: {bad} decidable mismatches of {dec.size} pixels ({int((~dec).sum())} undecidable)")
    assert bad == 0
    if name == "vos_vanish_5x41x47":
        assert int(want[0].max()) == 3 and int(pred[1:].max()) == 2          # the id lost at feature resolution never comes back


@pytest.mark.parametrize("name", VOS_FIXTURES)
def test_mask_path_default_arithmetic_against_reference_fixture(dev, golden, name):
    """The same on the DEFAULT arithmetic (f16 + FP6 encoder, f16 + FP6 pair kernel + refining merge).  Frame 0 exact; the mismatched
    pixels of the later frames are counted and held to DEFAULT_MISMATCH_BOUND, the figure of the first MI355X run (0 on all three)."""
    g, pred = _fixture_run(dev, golden, name, "f16f6")
    want = g["masks"]
    assert np.array_equal(pred[0], want[0].astype(np.float64))
    bad = int((pred[1:] != want[1:]).sum())
    print(f"{name} default arithmetic: {bad} mismatched pixels of {want[1:].size}")
    assert bad <= DEFAULT_MISMATCH_BOUND[name]
