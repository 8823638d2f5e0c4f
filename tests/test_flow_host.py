"""CPU: the host side of dense optical flow (test_cfg.flow) -- the float64 restatements of tests/flow_cases.py against
the fixtures recorded from the reference (tests/golden/gen_golden_flow.py), the option's parser, the pair schedule, the .flo format, the
end-point error, the colour wheel and the registry names."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import flow_cases as FC

FLOWS = ("flow_2x37x53", "flow_2x64x96")
WARP = "flow_warp_2x3x37x53"


@pytest.mark.parametrize("name", FLOWS)
@pytest.mark.parametrize("mode", ("consistency", "fb_abs"))
def test_consistency_restatement_reproduces_reference_masks(golden, name, mode):
    """The float64 restatement equals the reference's float32 masks on every decided pixel; the undecided share is the recorded one, at
    most 1 %; every mask is mixed."""
    g = golden(name)
    of, ob, df, db = FC.consistency_both_ref(g["flow_fw"], g["flow_bw"], mode, float(g["diff"]))
    for key, occ, decided in (("occ_fw", of, df), ("occ_bw", ob, db)):
        want = g[f"{mode}_{key}"]
        assert want.shape == occ.shape and 0.2 <= want.mean() <= 0.8
        assert int(((occ != want) & decided).sum()) == 0
        share = 1.0 - decided.mean()
        assert share == float(g[f"{mode}_{key}_undecided"]) and share <= 0.01


def test_warp_restatement_reproduces_reference(golden):
    g = golden(WARP)
    for ac in (False, True):
        for um in (False, True):
            out, ones, mag = FC.warp_ref(g["feat"], g["flow"], ac, um)
            want = g[f"out_ac{int(ac)}_m{int(um)}"]
            decided = np.broadcast_to((np.abs(ones - 0.9999) >= FC.MASK_MARGIN)[:, None], want.shape) if um else np.ones(want.shape, bool)
            assert 1.0 - decided.mean() == float(g[f"undecided_ac{int(ac)}_m{int(um)}"]) <= 0.01
            assert float(np.abs(out - want)[decided].max()) <= 1e-5
            assert (want == 0).mean() > 0.05 and (want != 0).mean() > 0.5            # some of it warped from outside the plane, most of it not
    # use_mask changes something, align_corners changes something
    assert (g["out_ac0_m0"] != g["out_ac0_m1"]).any() and (g["out_ac0_m1"] != g["out_ac1_m1"]).any()


def test_flow_from_lists_restatement_on_hand_made_lists():
    """One cell grid small enough to check by hand: 2 x 2 cells, R = 1, scale 4."""
    L = 3
    tap = lambda dy, dx: (dy + 1) * L + dx + 1
    idx = np.full((1, 4, 2), -1, np.int32)
    w = np.zeros((1, 4, 2), np.float32)
    idx[0, 0], w[0, 0] = (tap(0, 1), tap(-1, 0)), (0.5, 0.5)          # cell (0,0): the right neighbour, and a tap above the image (dropped)
    idx[0, 1], w[0, 1] = (tap(0, 0), tap(1, 0)), (0.25, 0.75)         # cell (0,1): itself and the cell below
    idx[0, 2], w[0, 2] = (tap(0, 0), -1), (1.0, 9.0)                  # cell (1,0): itself; an empty entry's weight is not read
    # cell (1,1): all empty -> invalid
    flow, valid, bound = FC.flow_from_lists_ref(idx, w, 2, 2, 1, 4, (8, 8), (0, 0), renorm=True)
    assert flow.shape == (1, 2, 8, 8) and valid.shape == (1, 8, 8) and bound.shape == (1, 8, 8)
    assert np.allclose(flow[0, :, 0, 0], (4.0, 0.0))                  # C / S = (4, 0) * 0.5 / 0.5
    assert np.allclose(flow[0, :, 0, 4], (0.0, 3.0)) and np.allclose(flow[0, :, 4, 0], (0.0, 0.0))
    assert np.allclose(flow[0, :, 0, 2], (2.0, 1.5))                  # half way between the cells (0,0) and (0,1)
    assert np.allclose(flow[0, :, 0, 7], flow[0, :, 0, 4])            # past the last cell: the upper neighbour is the last cell itself
    assert valid.sum() == 0                                           # 2 x 2 cells: the invalid cell (1,1) is among every pixel's four
    idx[0, 3], w[0, 3] = (tap(0, 0), -1), (1.0, 0.0)
    assert FC.flow_from_lists_ref(idx, w, 2, 2, 1, 4, (8, 8))[1].all()
    idx[0, 3] = -1
    raw, _, _ = FC.flow_from_lists_ref(idx, w, 2, 2, 1, 4, (8, 8), (0, 0), renorm=False)
    assert np.allclose(raw[0, :, 0, 0], (2.0, 0.0))                   # get_coord's own sum: the dropped tap pulls towards the origin
    padded, _, _ = FC.flow_from_lists_ref(idx, w, 2, 2, 1, 4, (6, 5), (2, 1), renorm=True)
    assert np.array_equal(padded[0], flow[0, :, 1:7, 2:7])            # the pad is cropped on the way out


def test_parse_flow():
    from fgvc_amd import engine
    assert engine.parse_flow(None, 12) is None
    c = engine.parse_flow(dict(type="window"), 12)
    assert (c.radius, c.step, c.renorm, c.occlusion, c.diff) == (12, 1, True, None, 1.5)
    c = engine.parse_flow(dict(type="window", radius=3, step=2, renorm=False, occlusion="fb_abs", diff=2), 12)
    assert (c.radius, c.step, c.renorm, c.occlusion, c.diff) == (3, 2, False, "fb_abs", 2.0)
    assert engine.parse_flow(dict(type="window", radius=None, occlusion="consistency"), 7).radius == 7
    for bad in (dict(), dict(type="raft"), dict(type="window", radius=-1), dict(type="window", step=0), dict(type="window", step=1.5),
                dict(type="window", renorm="yes"), dict(type="window", occlusion="cycle"), dict(type="window", diff=-1.0),
                dict(type="window", diff=float("nan")), dict(type="window", levels=3)):
        with pytest.raises(ValueError):
            engine.parse_flow(bad, 12)
    for bad in ("window", 3, ["window"]):
        with pytest.raises(TypeError):
            engine.parse_flow(bad, 12)
    with pytest.raises(NotImplementedError, match="range_map"):
        engine.parse_flow(dict(type="window", occlusion="range_map"), 12)


def _plan(T, step, budget_pairs, HW=48, k=10):
    from fgvc_amd import engine
    cfg = engine.LocalConfig(temperature=0.07, topk=k, precede_frames=1, radius=3, with_first=False, pair_budget=budget_pairs * HW * k * 8)
    return engine.flow_plan(T, step, HW, cfg), cfg


def test_flow_plan_pairs_rows_and_chunks():
    from fgvc_amd import engine
    p, _ = _plan(2, 1, 100)
    assert p.pairs == [(0, 1), (1, 0)] and p.chunks == [(0, 2, 0, 2)] and p.t_max == 1
    p, _ = _plan(5, 1, 100)
    assert p.pairs == [(0, 1), (1, 2), (2, 3), (3, 4), (1, 0), (2, 1), (3, 2), (4, 3)]
    assert p.slot_pair == [[i] for i in range(8)] and p.slot_frame == [[1], [2], [3], [4], [0], [1], [2], [3]]
    assert p.chunks == [(0, 8, 0, 8)] and p.pair_bytes == 48 * 10 * 8
    p, _ = _plan(5, 2, 100)
    assert p.pairs == [(0, 2), (1, 3), (2, 4), (2, 0), (3, 1), (4, 2)] and p.slot_frame == [[2], [3], [4], [0], [1], [2]]
    p, cfg = _plan(5, 1, 5)                                           # a budget of five pairs: two chunks
    assert p.chunks == [(0, 5, 0, 5), (5, 8, 5, 8)]
    # ... the chunking plan_local_clip gives single-slot rows under the same budget
    q = engine.plan_local_clip(9, cfg, 48)
    assert [c[1] - c[0] for c in q.chunks] == [c[1] - c[0] for c in p.chunks]
    p, _ = _plan(3, 3, 100)                                           # no pair that far apart
    assert p.pairs == [] and p.chunks == []
    with pytest.raises(ValueError):
        _plan(3, 1, 0.5)
    with pytest.raises(ValueError):
        _plan(3, 0, 10)


def test_flo_round_trip(tmp_path):
    from fgvc_amd import datasets
    rng = np.random.default_rng(0)
    f = rng.standard_normal((2, 7, 5)).astype(np.float32)
    p = str(tmp_path / "a.flo")
    datasets.write_flo(p, f)
    assert os.path.getsize(p) == 12 + 7 * 5 * 8
    raw = open(p, "rb").read()
    assert raw[:4] == b"PIEH" and np.frombuffer(raw[4:12], "<i4").tolist() == [5, 7]
    assert np.frombuffer(raw[12:20], "<f4").tolist() == [f[0, 0, 0], f[1, 0, 0]]          # (u, v) of the first pixel
    assert np.array_equal(datasets.read_flo(p), f)
    datasets.write_flo(p, f.transpose(1, 2, 0))                                           # (h, w, 2) is taken too
    assert np.array_equal(datasets.read_flo(p), f)
    open(p, "wb").write(raw[:-4])
    with pytest.raises(ValueError):
        datasets.read_flo(p)
    open(p, "wb").write(b"XXXX" + raw[4:])
    with pytest.raises(ValueError):
        datasets.read_flo(p)


def test_flow_epe_on_hand_made_values():
    from fgvc_amd import metrics
    gt = torch.zeros(1, 2, 2, 2)
    pred = torch.tensor([[[[0.0, 3.0], [0.0, 0.0]], [[0.0, 4.0], [0.0, 0.5]]]])          # errors 0, 5, 0, 0.5
    r = metrics.flow_epe(pred, gt)
    assert r == {"epe": 1.375, "1px": 0.75, "3px": 0.75, "5px": 0.75, "n": 4}
    r = metrics.flow_epe(pred, gt, valid=torch.tensor([[[1, 0], [1, 1]]], dtype=torch.uint8))
    assert r["n"] == 3 and abs(r["epe"] - 0.5 / 3) < 1e-12 and r["1px"] == 1.0
    r = metrics.flow_epe(pred, gt, valid=torch.zeros(1, 1, 2, 2))
    assert r["n"] == 0 and np.isnan(r["epe"])
    with pytest.raises(ValueError):
        metrics.flow_epe(pred, gt[:, :1])


def test_flow_to_rgb():
    from fgvc_amd import viz
    z = viz.flow_to_rgb(np.zeros((2, 4, 5), np.float32))
    assert z.shape == (4, 5, 3) and z.dtype == np.uint8 and (z == 255).all()             # zero flow is white
    f = np.zeros((3, 2, 2, 2), np.float32)
    f[0, 0], f[1, 1], f[2, 0, 0, 0] = 2.0, 2.0, np.nan
    c = viz.flow_to_rgb(torch.from_numpy(f), max_mag=2.0)
    assert c.shape == (3, 2, 2, 3) and (c[0] == c[0, 0, 0]).all() and (c[0, 0, 0] != c[1, 0, 0]).any()       # direction picks the hue
    assert tuple(c[0, 0, 0]) == (255, 0, 0)                                              # +x at full magnitude: the wheel's first colour
    assert (c[2, 0, 0] == 0).all() and (c[2, 1, 1] == 255).all()                         # not finite: black
    half = viz.flow_to_rgb(f[0] / 2, max_mag=2.0)
    assert tuple(half[0, 0]) == (255, 127, 127)                                          # half the magnitude: half way to white
    assert viz.flow_wheel().shape == (55, 3)


def test_registry_and_mmpt_names():
    import fgvc_amd.mmpt_api as api
    from fgvc_amd import _lib, build
    assert api.OPERATORS.get("Warp") is api.common.Warp
    w = api.build_operators(dict(type="Warp", align_corners=True, use_mask=False))
    assert (w.mode, w.padding_mode, w.align_corners, w.use_mask) == ("bilinear", "zeros", True, False)
    assert "flow.hip" in build.SOURCES
    for name in ("fgvc_flow_from_lists_f32", "fgvc_flow_consistency_f32", "fgvc_warp_f32"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    code = ("import fgvc_amd; fgvc_amd.install_as_mmpt();"
            "from mmpt.models.common import Warp, occlusion_estimation, forward_backward_consistency, forward_backward_absdiff, "
            "flow_to_coords, coords_grid_warp;"
            "from mmpt.models import OPERATORS, build_operators;"
            "assert OPERATORS.get('Warp') is Warp and isinstance(build_operators(dict(type='Warp')), Warp); print('ok')")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr


def test_flow_operators_refuse_cpu_and_f64_and_range_map():
    from fgvc_amd import ops
    import fgvc_amd.mmpt_api as api
    C = api.common
    f = torch.zeros(1, 2, 4, 4)
    with pytest.raises(TypeError, match="float32"):
        C.occlusion_estimation(f.double(), f.double())
    with pytest.raises(TypeError, match="float32"):
        C.Warp()(f.double(), f.double())
    with pytest.raises(RuntimeError):
        C.occlusion_estimation(f, f)
    with pytest.raises(NotImplementedError, match="range_map"):
        C.occlusion_estimation(f, f, "range_map")
    with pytest.raises(NotImplementedError, match="range_map"):
        ops.flow_consistency(f, f, "range_map")
    with pytest.raises(AssertionError):
        C.occlusion_estimation(f, f, "cycle")
    g = C.coords_grid_warp(torch.zeros(1, 2, 3, 5))
    assert g.shape == (1, 3, 5, 2) and float(g[0, 0, 0, 0]) == -1.0 and float(g[0, 2, 4, 0]) == 1.0 and float(g[0, 2, 4, 1]) == 1.0
    assert torch.equal(C.flow_to_coords(torch.zeros(1, 2, 3, 5))[0, 0, 1], torch.arange(5.0))


def test_library_rejects_bad_flow_arguments():
    """Bad arguments come back as error codes before any launch."""
    import ctypes
    from fgvc_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.fgvc_flow_from_lists_f32(None, p, 1, 2, 2, 1, 2, 4, 1, 8, 8, 0, 0, p, p, None) == 1 and b"null pointer" in lib.fgvc_last_error()
    assert lib.fgvc_flow_from_lists_f32(p, p, 0, 2, 2, 1, 2, 4, 1, 8, 8, 0, 0, p, p, None) == 1 and b"bad shape" in lib.fgvc_last_error()
    assert lib.fgvc_flow_from_lists_f32(p, p, 1, 2, 2, 1, 2, 4, 1, 8, 8, -1, 0, p, p, None) == 1 and b"bad output" in lib.fgvc_last_error()
    assert lib.fgvc_flow_consistency_f32(p, p, 1, 4, 4, 2, ctypes.c_float(1.5), p, p, None) == 1 and b"mode" in lib.fgvc_last_error()
    assert lib.fgvc_flow_consistency_f32(p, p, 70000, 4, 4, 0, ctypes.c_float(1.5), p, p, None) == 1
    assert lib.fgvc_warp_f32(p, None, 1, 1, 4, 4, 0, 1, p, None) == 1 and lib.fgvc_warp_f32(p, p, 1, 0, 4, 4, 0, 1, p, None) == 1
