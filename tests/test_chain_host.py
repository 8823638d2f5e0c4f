"""CPU: the host side of the flow-chaining point tracker (test_cfg.chain) -- engine.chain_points_host against the
fixtures recorded from the reference (tests/golden/gen_golden_chain.py) and against the loop restatement of tests/chain_cases.py on masked
and non-finite cases, the option's parser, the refusals that need no GPU, and the query grid."""
import numpy as np
import pytest
import torch

from tests import chain_cases as CC


def _same(got, want):
    (t1, v1), (t2, v2) = got, want
    assert t1.dtype == t2.dtype == np.float32 and v1.dtype == v2.dtype == np.uint8 and t1.shape == t2.shape and v1.shape == v2.shape
    assert np.array_equal(CC.bits(t1), CC.bits(t2)) and np.array_equal(v1, v2)


@pytest.mark.parametrize("name", CC.FIXTURES)
def test_host_rule_reproduces_reference(golden, name):
    """Trajectories with == on every entry (and on the bit patterns), visibility with ==; every fixture is mixed, and tracks reach both
    sides of their query frame."""
    from fgvc_amd import engine
    g = golden(name)
    traj, vis = engine.chain_points_host(g["flow_fw"], g["flow_bw"], g["query"])
    assert (traj == g["traj"]).all()
    _same((traj, vis), (g["traj"], g["vis"]))
    _same(CC.chain_ref(g["flow_fw"], g["flow_bw"], g["query"]), (g["traj"], g["vis"]))
    assert 0.2 <= g["vis"].mean() <= 0.9
    T, q = g["traj"].shape[0], g["query"]
    for p in range(len(q)):
        assert np.array_equal(CC.bits(g["traj"][int(q[p, 0]), p]), CC.bits(q[p, 1:]))       # the query frame holds the query point
    assert (q[:, 0] == 0).any() and (q[:, 0] == T - 1).any()
    before = [g["traj"][t, p] for p in range(len(q)) for t in range(int(q[p, 0]))]
    assert len(before) and np.isfinite(before).all() and np.abs(before).max() > 0           # frames before the query time are tracked


@pytest.mark.parametrize("visibility", ("frame", "consistency"))
def test_host_rule_equals_loop_restatement_with_masks(visibility):
    from fgvc_amd import engine
    T, h, w = 5, 13, 17
    fw, bw = CC.flows(T, h, w, 2.5, 3)
    q = CC.queries(40, T, h, w, 4)
    ok = CC.masks(T, h, w, 5)
    got = engine.chain_points_host(fw, bw, q, *ok, visibility=visibility)
    _same(got, CC.chain_ref(fw, bw, q, *ok, visibility=visibility))
    frame = engine.chain_points_host(fw, bw, q)
    assert np.array_equal(CC.bits(got[0]), CC.bits(frame[0]))                               # the masks never move a point
    if visibility == "consistency":
        assert (got[1] <= frame[1]).all() and (got[1] < frame[1]).any() and got[1].any()    # ... they only take visibility away
        # sticky outwards: once invisible by a bad hop, a later in-frame position stays invisible
        none = engine.chain_points_host(fw, bw, q, np.zeros_like(ok[0]), np.zeros_like(ok[1]), visibility=visibility)[1]
        at = q[:, 0].astype(int)
        assert none.sum() == none[at, np.arange(len(q))].sum() == frame[1][at, np.arange(len(q))].sum()
        with pytest.raises(ValueError):
            engine.chain_points_host(fw, bw, q, visibility=visibility)
    else:
        assert np.array_equal(got[1], frame[1])                                             # 'frame' does not read them


def test_host_rule_fails_closed():
    from fgvc_amd import engine
    T, h, w = 4, 9, 11
    fw, bw, q = CC.poisoned(T, h, w, 7)
    traj, vis = engine.chain_points_host(fw, bw, q)
    _same((traj, vis), CC.chain_ref(fw, bw, q))
    assert np.isnan(traj[2:, 0]).all() and not vis[2:, 0].any() and np.isfinite(traj[:2, 0]).all()        # NaN read on the hop 1 -> 2
    assert np.isnan(traj[0, 1]).all() and not vis[0, 1] and np.isfinite(traj[1:, 1]).all()                # inf read on the hop 1 -> 0
    assert np.isfinite(traj[:, 2:]).all()
    # queries that are never turned into an index: a NaN, an inf and a 2^23 position keep the query frame and nothing else; a time that is
    # no integer of [0, T) gives nothing at all
    q2 = np.asarray([(1, np.nan, 2), (1, 3, np.inf), (2, 2.0 ** 23, 1), (2, -(2.0 ** 23), 1), (1.5, 3, 3), (-1, 3, 3), (T, 3, 3), (np.nan, 3, 3),
                     (1, 3, 3)], np.float32)
    fw2, bw2 = CC.flows(T, h, w, 1.0, 8)
    traj, vis = engine.chain_points_host(fw2, bw2, q2)
    _same((traj, vis), CC.chain_ref(fw2, bw2, q2))
    for p in range(4):
        tq = int(q2[p, 0])
        assert np.array_equal(CC.bits(traj[tq, p]), CC.bits(q2[p, 1:])) and np.isnan(np.delete(traj[:, p], tq, 0)).all() and not vis[:, p].any()
    assert np.isnan(traj[:, 4:8]).all() and not vis[:, 4:8].any()
    assert np.isfinite(traj[:, 8]).all() and vis[1, 8]
    # a walk that leaves the usable range on its own: a constant flow of 2^22 px
    big = np.full((3, 2, 2, 2), 2.0 ** 22, np.float32)
    traj, vis = engine.chain_points_host(big, -big, np.asarray([(0, 0.5, 0.5), (3, 0.5, 0.5)], np.float32))
    _same((traj, vis), CC.chain_ref(big, -big, np.asarray([(0, 0.5, 0.5), (3, 0.5, 0.5)], np.float32)))
    assert traj[1, 0, 0] == 2.0 ** 22 + 0.5 and np.isnan(traj[2:, 0]).all()               # 2^23 + 0.5 rounds to 2^23: out
    assert traj[2, 1, 0] == 0.5 - 2.0 ** 22 and traj[1, 1, 0] == 0.5 - 2.0 ** 23 and np.isnan(traj[0, 1]).all()      # 0.5 - 2^23 is still inside


def test_host_rule_degenerate_shapes():
    from fgvc_amd import engine
    q = np.asarray([(0, 1.5, 0.5), (0, -1, 0)], np.float32)
    traj, vis = engine.chain_points_host(np.zeros((0, 2, 3, 4), np.float32), np.zeros((0, 2, 3, 4), np.float32), q)     # T = 1
    assert traj.shape == (1, 2, 2) and np.array_equal(traj[0], q[:, 1:]) and vis.tolist() == [[1, 0]]
    fw, bw = CC.flows(3, 4, 5, 1.0, 1)
    traj, vis = engine.chain_points_host(fw, bw, np.zeros((0, 3), np.float32))                                             # P = 0
    assert traj.shape == (3, 0, 2) and vis.shape == (3, 0)
    with pytest.raises(ValueError):
        engine.chain_points_host(fw, bw, q, visibility="cycle")


def test_parse_chain():
    from fgvc_amd import engine
    assert engine.parse_chain(None) is None
    assert engine.parse_chain(dict(type="flow")) == engine.ChainConfig("frame")
    assert engine.parse_chain(dict(type="flow", visibility="consistency")).visibility == "consistency"
    for bad in (dict(), dict(type="window"), dict(type="raft"), dict(type="flow", visibility="cycle"), dict(type="flow", visibility=None),
                dict(type="flow", step=1)):
        with pytest.raises(ValueError):
            engine.parse_chain(bad)
    for bad in ("flow", 1, ["flow"]):
        with pytest.raises(TypeError):
            engine.parse_chain(bad)
    engine.check_query_times(torch.tensor([0.0, 2.0, 4.0]), 5)
    engine.check_query_times(torch.tensor([], dtype=torch.float32), 5)
    for bad in ([5.0], [-1.0], [1.5], [float("nan")], [float("inf")]):
        with pytest.raises(ValueError, match="query time"):
            engine.check_query_times(torch.tensor(bad), 5)


def test_grid_queries():
    from fgvc_amd import engine
    q = engine.grid_queries(2, 5, 7, 3)
    assert q.dtype == torch.float32 and q.tolist() == [[2, 1, 1], [2, 4, 1], [2, 1, 4], [2, 4, 4]]
    q = engine.grid_queries(0, 4, 6, 2, offset=(0, 1))
    assert q.tolist() == [[0, 0, 1], [0, 2, 1], [0, 4, 1], [0, 0, 3], [0, 2, 3], [0, 4, 3]]
    assert engine.grid_queries(0, 480, 854, 4).shape == (120 * 213, 3)                      # x = 2, 6, ..., 850
    assert engine.grid_queries(1, 9, 9, 8).tolist() == [[1, 4, 4]]
    for bad in (lambda: engine.grid_queries(1, 3, 3, 8),               # the default offset, stride // 2, lies outside a 3 x 3 frame
lambda: engine.grid_queries(0, 4, 6, 0), lambda: engine.grid_queries(-1, 4, 6, 2), lambda: engine.grid_queries(0, 4, 6, 2, offset=(6, 0)),
                lambda: engine.grid_queries(0, 0, 6, 2)):
        with pytest.raises(ValueError):
            bad()


def _model(typ, **test_cfg):
    import fgvc_amd.mmpt_api as api
    return api.build_model(dict(type=typ, backbone=dict(type="ResNet", depth=18, strides=(1, 2, 1, 1), out_indices=(2,), pool_type="none")),
                           train_cfg=None, test_cfg=api.ConfigDict(**test_cfg)).eval()


@pytest.mark.parametrize("typ", ("VanillaTracker", "HRVanillaTracker"))
def test_trackers_read_the_key_and_refuse_what_is_out_of_scope(typ):
    from fgvc_amd import dist, engine
    base = dict(precede_frames=2, topk=6, temperature=0.07, neighbor_range=8, with_first=True)
    assert _model(typ, **base).chain_cfg is None and _model(typ, **base, chain=None).chain_cfg is None
    m = _model(typ, **base, chain=dict(type="flow", visibility="consistency"))
    assert m.chain_cfg == engine.ChainConfig("consistency") and m.last_flow is None
    for bad in (dict(type="raft"), dict(type="flow", visibility="cycle")):
        with pytest.raises(ValueError, match="chain"):
            _model(typ, **base, chain=bad)
    rgbs, qp = torch.zeros(1, 3, 3, 16, 16), torch.tensor([[[0.0, 4.0, 4.0], [2.0, 5.0, 5.0]]])
    tr, vi = torch.zeros(1, 3, 2, 2), torch.zeros(1, 3, 2)
    call = lambda model, q=qp: model(test_mode=True, rgbs=rgbs, query_points=q, trajectories=tr, visibilities=vi)
    with pytest.raises(ValueError, match="occlusion"):
        call(_model(typ, **base, chain=dict(type="flow"), occlusion=dict(type="cycle")))
    with pytest.raises(ValueError, match="step"):
        call(_model(typ, **base, chain=dict(type="flow"), flow=dict(type="window", step=2)))
    for t in (3.0, -1.0, 0.5, float("nan")):
        with pytest.raises(ValueError, match="query time"):
            call(m, torch.tensor([[[t, 4.0, 4.0]]]))
    with pytest.raises(RuntimeError, match="GPU only"):                 # every refusal above comes before any device work
        call(m)
    with pytest.raises(TypeError):                                      # a mixture of the two call forms is still refused first
        m(test_mode=True, rgbs=rgbs, query_points=qp, imgs=torch.zeros(1, 1, 3, 3, 16, 16))

    class Backend:
        model = m
    with pytest.raises(NotImplementedError, match="chain"):
        dist.track_points_sharded(Backend(), torch.zeros(2, 3, 16, 16), torch.zeros(1, 3), m.engine_config())


def test_library_declares_and_checks_the_chain_kernel():
    """The symbol is exported, and bad arguments come back as error codes before any launch."""
    import ctypes
    from fgvc_amd import _lib, build
    assert "chain.hip" in build.SOURCES and "fgvc_flow_chain_f32" in _lib.SIGNATURES
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fgvc_flow_chain_f32(p, p, None, None, p, 0, 1, 4, 4, 0, p, p, None) == 1 and b"bad shape" in lib.fgvc_last_error()
    assert lib.fgvc_flow_chain_f32(p, p, None, None, p, 2, 1, 4, 4, 2, p, p, None) == 1 and b"visibility" in lib.fgvc_last_error()
    assert lib.fgvc_flow_chain_f32(p, None, None, None, p, 2, 1, 4, 4, 0, p, p, None) == 1 and b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_flow_chain_f32(p, p, None, p, p, 2, 1, 4, 4, 1, p, p, None) == 1 and b"masks" in lib.fgvc_last_error()
    assert lib.fgvc_flow_chain_f32(p, p, None, None, p, 2, 1, 4, 4, 0, ctypes.c_void_p(p.value + 4), p, None) == 1 and b"alignment" in lib.fgvc_last_error()
    assert lib.fgvc_flow_chain_f32(None, None, None, None, None, 2, 0, 4, 4, 0, None, None, None) == 0        # P = 0: nothing to do
