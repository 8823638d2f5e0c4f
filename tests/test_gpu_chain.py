"""GPU: point tracks in both time directions by chaining the dense flow (test_cfg.chain).  The kernel against the
fixtures recorded from the reference (tests/golden/gen_golden_chain.py) and against engine.chain_points_host, both with == on the bit
patterns -- the contract is equality, no tolerance appears here --, then both trackers' points call with the key set."""
import numpy as np
import pytest
import torch

from tests import chain_cases as CC
from tests.golden import clips

pytestmark = pytest.mark.gpu
T = torch.from_numpy

VA = dict(typ="VanillaTracker", strides=(1, 1, 1, 4),
          cfg=dict(precede_frames=5, topk=10, temperature=0.07, neighbor_range=12, step=512, with_first_neighbor=True, batch_step=2))
HR = dict(typ="HRVanillaTracker", strides=(1, 2, 1, 1),
          cfg=dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True, batch_step=2))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _chain(dev, fw, bw, q, ok=(None, None), visibility="frame", **kw):
    from fgvc_amd import ops
    ok = tuple(None if m is None else T(m).to(dev) for m in ok)
    return ops.flow_chain(T(fw).to(dev), T(bw).to(dev), T(q).to(dev), *ok, visibility=visibility, **kw)


def _held_to(got, want):
    """trajectories and visibility with ==, the trajectories on their bit patterns: a NaN counts where it stands, -0 is not +0."""
    (traj, vis), (wt, wv) = got, want
    assert traj.dtype == torch.float32 and vis.dtype == torch.uint8 and tuple(traj.shape) == wt.shape and tuple(vis.shape) == wv.shape
    assert torch.equal(_bits(traj).cpu(), _bits(T(np.ascontiguousarray(wt))))
    assert torch.equal(vis.cpu(), T(np.ascontiguousarray(wv)))


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CC.FIXTURES)
def test_flow_chain_reproduces_reference(dev, golden, name):
    g = golden(name)
    got = _chain(dev, g["flow_fw"], g["flow_bw"], g["query"])
    assert bool((got[0].cpu() == T(g["traj"])).all())
    _held_to(got, (g["traj"], g["vis"]))


RAGGED = dict(T=5, h=13, w=17, amp=2.5, P=257)


@pytest.fixture(scope="module")
def ragged():
    """One clip, 257 queries and masks; the host rule in both visibility modes, computed once (a point's track does not depend on the others)."""
    from fgvc_amd import engine
    c = RAGGED
    fw, bw = CC.flows(c["T"], c["h"], c["w"], c["amp"], 11)
    q = CC.queries(c["P"], c["T"], c["h"], c["w"], 12)
    ok = CC.masks(c["T"], c["h"], c["w"], 13)
    want = {v: engine.chain_points_host(fw, bw, q, *ok, visibility=v) for v in ("frame", "consistency")}
    assert (want["consistency"][1] < want["frame"][1]).any() and want["consistency"][1].any()
    return fw, bw, q, ok, want


@pytest.mark.parametrize("visibility", ("frame", "consistency"))
@pytest.mark.parametrize("P", (1, 63, 65, 257))
def test_flow_chain_equals_host_rule_on_ragged_point_counts(dev, ragged, P, visibility):
    fw, bw, q, ok, want = ragged
    wt, wv = want[visibility]
    _held_to(_chain(dev, fw, bw, q[:P], ok, visibility), (wt[:, :P], wv[:, :P]))


@pytest.mark.parametrize("visibility", ("frame", "consistency"))
def test_flow_chain_short_clips_and_no_points(dev, visibility):
    """T = 1 returns the query points (nothing to read: the masks' shape is (0, h, w)), T = 2 is a single hop either way, P = 0 returns empty
    tensors."""
    from fgvc_amd import engine
    h, w = 6, 9
    q = CC.queries(70, 1, h, w, 21)
    e, m = np.zeros((0, 2, h, w), np.float32), np.zeros((0, h, w), np.uint8)
    traj, vis = _chain(dev, e, e, q, (m, m), visibility)
    _held_to((traj, vis), engine.chain_points_host(e, e, q, m, m, visibility))
    assert torch.equal(_bits(traj[0]).cpu(), _bits(T(q[:, 1:].copy())))
    fw, bw = CC.flows(2, h, w, 2.0, 22)
    q, ok = CC.queries(70, 2, h, w, 23), CC.masks(2, h, w, 24)
    _held_to(_chain(dev, fw, bw, q, ok, visibility), engine.chain_points_host(fw, bw, q, *ok, visibility=visibility))
    traj, vis = _chain(dev, fw, bw, np.zeros((0, 3), np.float32), ok, visibility)
    assert tuple(traj.shape) == (2, 0, 2) and tuple(vis.shape) == (2, 0)


def test_flow_chain_fails_closed(dev):
    """A NaN and an inf planted in flow pixels that one track each crosses; queries that are no index; a walk that runs past 2^23."""
    from fgvc_amd import engine
    Tn, h, w = 4, 9, 11
    fw, bw, q = CC.poisoned(Tn, h, w, 7)
    want = engine.chain_points_host(fw, bw, q)
    assert np.isnan(want[0][2:, 0]).all() and np.isnan(want[0][0, 1]).all() and np.isfinite(want[0][:, 2:]).all()
    _held_to(_chain(dev, fw, bw, q), want)
    ok = CC.masks(Tn, h, w, 9)
    _held_to(_chain(dev, fw, bw, q, ok, "consistency"), engine.chain_points_host(fw, bw, q, *ok, visibility="consistency"))
    q2 = np.asarray([(1, np.nan, 2), (1, 3, np.inf), (2, 2.0 ** 23, 1), (2, -(2.0 ** 23), 1), (1.5, 3, 3), (-1, 3, 3), (Tn, 3, 3), (np.nan, 3, 3),
                     (1, 3, 3), (3, 1e30, -1e30)], np.float32)
    fw2, bw2 = CC.flows(Tn, h, w, 1.0, 8)                               # (clean flows: only the queries are bad here)
    want = engine.chain_points_host(fw2, bw2, q2)
    assert np.isnan(want[0][:, 4:8]).all() and np.isfinite(want[0][:, 8]).all() and np.isnan(want[0][:3, 9]).all()
    _held_to(_chain(dev, fw2, bw2, q2), want)
    _held_to(_chain(dev, fw, bw, q2), engine.chain_points_host(fw, bw, q2))                # ... and on the poisoned ones
    big = np.full((3, 2, 2, 2), 2.0 ** 22, np.float32)
    q3 = np.asarray([(0, 0.5, 0.5), (3, 0.5, 0.5)], np.float32)
    want = engine.chain_points_host(big, -big, q3)
    assert np.isnan(want[0][2:, 0]).all() and np.isnan(want[0][0, 1]).all() and np.isfinite(want[0][1, 1]).all()
    _held_to(_chain(dev, big, -big, q3), want)


def test_flow_chain_writes_between_guard_bands(dev, ragged):
    fw, bw, q, ok, want = ragged
    Tn, P, g = RAGGED["T"], 65, 256
    tbuf = torch.full((Tn * P * 2 + 2 * g,), float("nan"), device=dev)
    vbuf = torch.full((Tn * P + 2 * g,), 0xA5, device=dev, dtype=torch.uint8)
    out = (tbuf[g:g + Tn * P * 2].view(Tn, P, 2), vbuf[g:g + Tn * P].view(Tn, P))
    got = _chain(dev, fw, bw, q[:P], ok, "consistency", out=out)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    assert bool(torch.isnan(tbuf[:g]).all()) and bool(torch.isnan(tbuf[g + Tn * P * 2:]).all())
    assert bool((vbuf[:g] == 0xA5).all()) and bool((vbuf[g + Tn * P:] == 0xA5).all())
    _held_to(got, (want["consistency"][0][:, :P], want["consistency"][1][:, :P]))
    assert bool(((vbuf[g:g + Tn * P] == 0) | (vbuf[g:g + Tn * P] == 1)).all())
    with pytest.raises(ValueError, match="out"):
        _chain(dev, fw, bw, q[:P], out=(out[0], out[1][:, :P - 1]))


def test_flow_chain_takes_strided_queries_and_refuses_bad_arguments(dev, ragged):
    from fgvc_amd import ops
    fw, bw, q, ok, want = ragged
    fwd, bwd = T(fw).to(dev), T(bw).to(dev)
    wide = torch.zeros((RAGGED["P"], 5), device=dev)
    wide[:, 1:4] = T(q).to(dev)
    _held_to(ops.flow_chain(fwd, bwd, wide[:, 1:4]), want["frame"])                        # a column slice: rows 20 bytes apart
    _held_to(ops.flow_chain(fwd, bwd, T(q).to(dev)[::2]), (want["frame"][0][:, ::2], want["frame"][1][:, ::2]))
    qd = T(q).to(dev)
    with pytest.raises(ValueError, match="consistency"):
        ops.flow_chain(fwd, bwd, qd, visibility="consistency")
    with pytest.raises(ValueError, match="visibility"):
        ops.flow_chain(fwd, bwd, qd, visibility="cycle")
    with pytest.raises(ValueError, match="flow_fw"):
        ops.flow_chain(fwd, bwd[1:], qd)
    with pytest.raises(ValueError, match="query"):
        ops.flow_chain(fwd, bwd, qd[:, :2])
    with pytest.raises(ValueError, match="ok_fw"):
        ops.flow_chain(fwd, bwd, qd, T(ok[0]).to(dev), T(ok[1]).to(dev)[:, 1:], "consistency")
    with pytest.raises(TypeError, match="float32"):
        ops.flow_chain(fwd, bwd, qd.double())
    with pytest.raises(RuntimeError):
        ops.flow_chain(fwd, bwd, T(q))


# ---- 2. the trackers --------------------------------------------------------------------------------------------------------------------
def _tracker(dev, spec, **extra):
    import fgvc_amd.mmpt_api as api
    model = api.build_model(dict(type=spec["typ"], backbone=dict(type="ResNet", depth=18, strides=spec["strides"], out_indices=(2,),
                                                                 pool_type="none")),
                            train_cfg=None, test_cfg=api.ConfigDict(**{**spec["cfg"], **extra}))
    torch.manual_seed(4)
    model.init_weights()                                                # Kaiming
    return model.to(dev).eval()


def _clip(dev, seed=6):
    tex = clips.moving_texture(3, 64, 96, seed)                         # (T, 3, h, w) int8, drifting by (3, -2) px a frame
    floats = (T(tex).float() / 32).to(dev)
    u8 = T((tex.astype(np.int16) + 128).astype(np.uint8)).permute(0, 2, 3, 1).contiguous().to(dev)      # (T, h, w, 3)
    return floats, u8


def _points(dev, Tn=3, h=64, w=96, P=24, seed=3):
    g = torch.Generator().manual_seed(seed)
    qp = torch.stack([(torch.arange(P) % Tn).float(), 16 + torch.rand(P, generator=g) * (w - 32), 16 + torch.rand(P, generator=g) * (h - 32)], -1).float()
    qp[0, 1:], qp[1, 1:] = torch.tensor([40.0, 30.0]), torch.tensor([17.0, 45.0])               # integer positions too
    return qp[None].to(dev), torch.zeros(1, Tn, P, 2, device=dev, dtype=torch.float64), torch.zeros(1, Tn, P, device=dev, dtype=torch.bool)


@pytest.mark.parametrize("visibility", ("frame", "consistency"))
@pytest.mark.parametrize("spec", [VA, HR], ids=["vanilla", "hr"])
def test_model_chain_call(dev, spec, visibility):
    from fgvc_amd import engine, ops
    floats, u8 = _clip(dev)
    qp, tr, vi = _points(dev)
    Tn, P = 3, qp.shape[1]
    model = _tracker(dev, spec, chain=dict(type="flow", visibility=visibility), input=dict(type="rgb8"))
    out = model(test_mode=True, rgbs=floats[None], query_points=qp, trajectories=tr, visibilities=vi)
    assert len(out) == 5 and out[0] is tr and out[1] is vi and out[4] is qp               # the points keep their order: nothing is regrouped
    traj, vis = out[2], out[3]
    assert traj.shape == tr.shape and traj.dtype == tr.dtype and vis.shape == vi.shape and vis.dtype == vi.dtype and traj.is_cuda
    assert bool(torch.isfinite(traj).all())
    tq = qp[0, :, 0].long()
    at = traj[0, tq, torch.arange(P, device=dev)]
    assert torch.equal(at, qp[0, :, 1:].double())                                          # the query frame holds the query point exactly
    before = torch.arange(Tn, device=dev).view(Tn, 1) < tq.view(1, P)
    assert int(before.sum()) == P and bool((traj[0][before] != 0).all())                   # frames before the query time are tracked
    # ... the kernel called by hand on the flows the call left behind, bit for bit
    flow = model.last_flow
    want = ["flow_bw", "flow_fw", "valid_bw", "valid_fw"] + (["occ_bw", "occ_fw"] if visibility == "consistency" else [])
    assert sorted(flow) == sorted(want) and flow["flow_fw"].shape == (Tn - 1, 2, 64, 96)
    ok = engine.chain_masks(flow) if visibility == "consistency" else (None, None)
    ht, hv = ops.flow_chain(flow["flow_fw"], flow["flow_bw"], qp[0], *ok, visibility=visibility)
    assert torch.equal(traj[0], ht.double()) and torch.equal(vis[0], hv.bool())
    if visibility == "consistency":
        ft, fv = ops.flow_chain(flow["flow_fw"], flow["flow_bw"], qp[0])
        assert torch.equal(_bits(ft), _bits(ht)) and bool((hv <= fv).all())
    # ... the flows are the flow call's own
    fmodel = _tracker(dev, spec, flow=dict(type="window", occlusion="consistency" if visibility == "consistency" else None))
    own = fmodel(test_mode=True, imgs=floats.transpose(0, 1)[None, None])
    for key in flow:
        assert torch.equal(flow[key], own[key]), key
    # ... raw uint8 frames through test_cfg.input: the call on ops.frames_to_lab of them
    raw = model(test_mode=True, rgbs=u8[None], query_points=qp, trajectories=tr, visibilities=vi)
    same = model(test_mode=True, rgbs=ops.frames_to_lab(u8)[None], query_points=qp, trajectories=tr, visibilities=vi)
    assert torch.equal(raw[2], same[2]) and torch.equal(raw[3], same[3])
    # ... without trajectories / visibilities: float32 on the device
    bare = model(test_mode=True, rgbs=floats[None], query_points=qp)
    assert bare[0] is None and bare[2].dtype == torch.float32 and torch.equal(bare[2].double(), traj) and torch.equal(bare[3].bool(), vis)
    drift = torch.tensor([3.0, -2.0], device=dev, dtype=torch.float64)
    known = qp[0, :, 1:].double()[None] + (torch.arange(Tn, device=dev).view(Tn, 1) - tq.view(1, P)).double()[..., None] * drift
    dist = (traj[0] - known).norm(dim=-1)
    print(f"[chain 2] {spec['typ']} Kaiming weights, 3 x 64 x 96 moving texture, visibility={visibility}: median distance of the chained tracks "
          f"from the known drift {float(dist[before | (dist > 0)].median()):.3f} px (before the query time {float(dist[before].median()):.3f} px), "
          f"visible share {float(vis.float().mean()):.3f} (measured, not asserted)")


@pytest.mark.parametrize("spec", [VA, HR], ids=["vanilla", "hr"])
def test_model_chain_routing_and_refusals(dev, spec):
    floats, _ = _clip(dev)
    qp, tr, vi = _points(dev)
    tr, vi = tr.float(), vi.float()
    call = lambda m, q=qp, frames=floats: m(test_mode=True, rgbs=frames[None], query_points=q, trajectories=tr, visibilities=vi)
    # without the key, and with test_cfg.flow alone, the points call propagates labels as ever: nothing before the earliest query time
    plain = call(_tracker(dev, spec))
    only_flow = _tracker(dev, spec, flow=dict(type="window"))
    got = call(only_flow)
    assert torch.equal(got[2], plain[2]) and torch.equal(got[3], plain[3]) and only_flow.last_flow is None
    if spec is HR:                                                      # (with_first=True: regrouped by query time)
        late = qp.clone()
        late[0, :, 0] = 1
        assert bool((call(only_flow, late)[2][0, 0] == 0).all())
    with pytest.raises(ValueError, match="occlusion"):
        call(_tracker(dev, spec, chain=dict(type="flow"), occlusion=dict(type="cycle")))
    with pytest.raises(ValueError, match="step"):
        call(_tracker(dev, spec, chain=dict(type="flow"), flow=dict(type="window", step=2)))
    with pytest.raises(ValueError, match="chain"):
        _tracker(dev, spec, chain=dict(type="flow", visibility="cycle"))
    model = _tracker(dev, spec, chain=dict(type="flow"), flow=dict(type="window", radius=3))
    for t in (3.0, -1.0, 0.5):
        bad = qp.clone()
        bad[0, 5, 0] = t
        with pytest.raises(ValueError, match="query time"):
            call(model, bad)
    assert call(model)[2].shape == tr.shape and model.flow_stats["chunks"] == 1           # test_cfg.flow's own radius is the one used
    if spec is HR:                                                      # the flow call's whole-pitch refusal, inherited
        with pytest.raises(NotImplementedError, match="pitch"):
            call(model, frames=torch.zeros(3, 3, 64, 98, device=dev))
    # with the key set, the mask call is still the mask call
    imgs = floats.transpose(0, 1)[None, None]
    seg = torch.zeros(1, 64, 96, dtype=torch.uint8)
    seg[0, 10:30, 20:50] = 1
    masks = model(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(64, 96))])
    want = _tracker(dev, spec)(test_mode=True, imgs=imgs, ref_seg_map=seg.to(dev), img_meta=[dict(original_shape=(64, 96))])
    assert isinstance(masks, list) and np.array_equal(masks[0], want[0])
