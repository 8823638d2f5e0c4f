"""CPU tests of the pose renderer's contract (viz.render(skeleton=..., heat=...)): known answers from the rule with
dyadic numbers, the refusals, test_cfg.pose, pose_visibles / pose_tracks, the skeleton table, the demo's arguments, and the code-object notes
of fgvc_render_pose_u8."""
import importlib.util
import os

import numpy as np
import pytest

from fgvc_amd import viz
from tests import pose_cases as PC
from tests import render_cases as RC
from tests import trails_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"fgvc_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- defaults change nothing ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.cases()))
def test_no_pose_is_todays_render(name):
    c = RC.cases()[name]
    got = viz.render(skeleton=None, limb_colors=None, limb_width=2.0, limb_alpha=1.0, heat=None, heat_colors=None, heat_gain=1.0,
                     heat_alpha=0.5, **c)
    assert np.array_equal(got, RC.expected(name))


@pytest.mark.parametrize("name", [n for n, c in TC.cases().items() if c.get("dots", True)])        # (a case without dots is paint_trails')
def test_no_pose_is_todays_trails(name):
    assert np.array_equal(viz.render(skeleton=None, heat=None, **TC.cases()[name]), TC.expected(name))


@pytest.mark.parametrize("name", list(TC.cases()))
def test_shared_segment_arithmetic_is_still_the_restated_rule(name):
    """A guard on moving the per-segment arithmetic into viz._segment_host (it holds before the move too)."""
    assert np.array_equal(TC.expected(name), TC.restated(name))


# ---- known answers ----------------------------------------------------------------------------------------------------------------------
def test_hand_checked_limb():
    """A horizontal limb from (2, 3) to (6, 3), width 2, alpha 1, colour 200 on grey 100.  The + 0.5 of the rule puts its axis at y = 3.5,
    so the tracks are (1.5, 2.5) and (5.5, 2.5) for an axis on the pixel row 3.  ro = 1.5, ri = 0.5, ro2 = 2.25, g = 0.5: on the axis
    cov = min(2.25 * 0.5, 1) = 1 -> 200; one pixel off d2 = 1, cov = (2.25 - 1) * 0.5 = 0.625 -> int(0.375 * 100 + 0.625 * 200) = 162; two
    pixels off d2 = 4 > ro2 -> 100."""
    frames = np.full((1, 8, 10, 3), 100, np.uint8)
    tracks = np.array([[(1.5, 2.5)], [(5.5, 2.5)]])
    got = viz.paint_pose(frames, tracks, skeleton=[(0, 1)], limb_colors=np.full((1, 3), 200), limb_width=2.0, limb_alpha=1.0, dots=False)
    assert (got[0, 3, 2:7] == 200).all()
    assert (got[0, 2, 2:7] == 162).all() and (got[0, 4, 2:7] == 162).all()
    assert (got[0, 1, :] == 100).all() and (got[0, 5, :] == 100).all()
    assert (got[0, 3, 0] == 100).all() and (got[0, 3, 8] == 100).all()          # two pixels beyond either end
    assert (got[0, 3, 1] == 162).all() and (got[0, 3, 7] == 162).all()          # one pixel beyond: the same ramp round the end
    half = viz.paint_pose(frames, tracks, skeleton=[(0, 1)], limb_colors=np.full((1, 3), 200), limb_alpha=0.5, dots=False)
    assert (half[0, 3, 2:7] == 150).all() and (half[0, 2, 4] == int((1 - 0.3125) * 100 + 0.3125 * 200)).all()
    same = viz.render(frames, tracks=tracks, skeleton=[(0, 1)], limb_colors=np.full((1, 3), 200), radius=1)
    assert np.array_equal(same, viz.render(got, tracks=tracks, radius=1))       # the dots go on top of the limbs


def test_hand_checked_heat():
    frames = np.full((1, 4, 5, 3), 100, np.uint8)
    heat = np.zeros((1, 2, 4, 5), np.float32)
    heat[0, 0, 1, 2] = 0.5
    col = np.array([(200, 200, 200), (0, 40, 255)])
    got = viz.render(frames, heat=heat[:, :1], heat_colors=col[:1], heat_gain=1.0, heat_alpha=0.5)
    assert (got[0, 1, 2] == 125).all()                                          # a = 0.25: 0.75 * 100 + 0.25 * 200
    got[0, 1, 2] = 100
    assert (got == 100).all()
    heat[0, 1, 1, 2] = 1.0                                                      # a second map on the same pixel, a = 0.5
    ab = viz.render(frames, heat=heat, heat_colors=col)
    ba = viz.render(frames, heat=heat[:, ::-1], heat_colors=col[::-1])
    assert ab[0, 1, 2].tolist() == [int(0.5 * 125 + 0.5 * 0), int(0.5 * 125 + 0.5 * 40), int(0.5 * 125 + 0.5 * 255)] == [62, 82, 190]
    assert ba[0, 1, 2].tolist() == [int(0.75 * 50 + 0.25 * 200), int(0.75 * 70 + 0.25 * 200), int(0.75 * 177 + 0.25 * 200)] == [87, 102, 182]
    for v, want in ((-1.0, 100), (np.nan, 100), (0.0, 100), (np.inf, 150), (7.0, 150), (-np.inf, 100), (1e-45, 100)):
        h = np.full((1, 1, 4, 5), v, np.float32)
        assert (viz.render(frames, heat=h, heat_colors=col[:1]) == want).all(), v
    assert (viz.render(frames, heat=np.full((1, 1, 4, 5), 0.25), heat_colors=col[:1], heat_gain=4.0, heat_alpha=1.0) == 200).all()
    assert (viz.render(frames, heat=np.full((1, 1, 4, 5), 0.25), heat_colors=col[:1], heat_alpha=0.0) == 100).all()


def test_stage_order_is_overlay_heat_limbs_dots():
    c = PC.cases()["all_3x35x57"]
    step = viz.render(c["frames"], ids=c["ids"], palette=c.get("palette"), alpha=c.get("alpha", 128), contour=c.get("contour", True))
    step = viz.render(step, heat=c["heat"], heat_gain=c["heat_gain"], heat_alpha=c["heat_alpha"])
    step = viz.paint_pose(step, c["tracks"], c["visibles"], c["colors"], skeleton=c["skeleton"], limb_width=c["limb_width"],
                          limb_alpha=c["limb_alpha"], dots=False)
    step = viz.render(step, tracks=c["tracks"], visibles=c["visibles"], colors=c["colors"], radius=c["radius"])
    assert np.array_equal(step, PC.expected("all_3x35x57"))


def test_cases_reach_what_they_are_for():
    c = PC.cases()
    assert not np.array_equal(PC.expected("rounds_2x20x40"), PC.expected("rounds_2x20x40_reversed"))        # the edge order is kept
    r = c["rounds_2x20x40"]
    assert r["skeleton"].shape[0] == 300 > 256 and (r["tracks"][..., 1] > TILE_ROWS).all() and (r["tracks"][..., 1] < 2 * TILE_ROWS - 1).all()
    assert np.array_equal(PC.expected("rounds_2x20x40_e0"), viz.render(r["frames"], tracks=r["tracks"], colors=r["colors"], radius=1))
    assert np.array_equal(PC.expected("rounds_2x20x40_p0"), r["frames"])
    d = c["degenerate_2x12x24_a1"]
    assert np.array_equal(PC.expected("degenerate_2x12x24_a0"), viz.render(d["frames"], tracks=d["tracks"], visibles=d["visibles"],
                                                                           colors=d["colors"], radius=1))
    drawn = dict(d, skeleton=d["skeleton"][8:])                                 # the eight refused limbs change nothing
    assert np.array_equal(PC.render(drawn), PC.expected("degenerate_2x12x24_a1"))
    for lw in ("1", "2", "16"):
        t = c[f"tiles_3x20x300_w{lw}"]
        assert t["frames"].shape == (3, 20, 300, 3)
        assert (PC.expected(f"tiles_3x20x300_w{lw}") != viz.render(t["frames"], tracks=t["tracks"], visibles=t["visibles"], colors=t["colors"],
                                                                    radius=1)).any()
    for K in (1, 3, 17):
        h = c[f"heat_2x11x261_k{K}_float32"]["heat"]
        assert np.isnan(h).any() and np.isposinf(h).any() and np.isneginf(h).any() and (h < 0).any() and (h > 1).any()
        assert ((h != 0) & (np.abs(h) < np.finfo(np.float32).tiny)).any()        # denormals
    assert np.array_equal(PC.expected("heat_2x11x261_k3_alpha0"), c["heat_2x11x261_k3_alpha0"]["frames"])


TILE_ROWS = PC.TILE[0]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    f = np.zeros((2, 6, 7, 3), np.uint8)
    tr = np.zeros((3, 2, 2))
    heat = np.zeros((2, 2, 6, 7), np.float32)
    sk = np.array([(0, 1), (1, 2)])
    with pytest.raises(ValueError, match="trail: not together with skeleton= or heat="):
        viz.render(f, tracks=tr, trail=2, skeleton=sk, radius=1)
    with pytest.raises(ValueError, match="trail: not together with skeleton= or heat="):
        viz.render(f, tracks=tr, trail=2, heat=heat, radius=1)
    with pytest.raises(ValueError, match="skeleton: needs tracks"):
        viz.render(f, skeleton=sk)
    with pytest.raises(ValueError, match=r"skeleton: edge 1 = \(1, 3\) names a joint outside 0 .. 2"):
        viz.render(f, tracks=tr, skeleton=[(0, 1), (1, 3)], radius=1)
    with pytest.raises(ValueError, match=r"skeleton: edge 0 = \(-1, 0\)"):
        viz.render(f, tracks=tr, skeleton=[(-1, 0)], radius=1)
    with pytest.raises(ValueError, match="skeleton"):
        viz.render(f, tracks=tr, skeleton=np.zeros((2, 3), np.int64), radius=1)
    with pytest.raises(TypeError, match="skeleton"):
        viz.render(f, tracks=tr, skeleton=np.zeros((2, 2)), radius=1)
    for bad in (0.5, 17.0, "x"):
        with pytest.raises(ValueError, match="limb_width"):
            viz.render(f, tracks=tr, skeleton=sk, limb_width=bad, radius=1)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="limb_alpha"):
            viz.render(f, tracks=tr, skeleton=sk, limb_alpha=bad, radius=1)
    with pytest.raises(ValueError, match="limb_colors"):
        viz.render(f, tracks=tr, skeleton=sk, limb_colors=np.zeros((3, 3), np.uint8), radius=1)
    with pytest.raises(ValueError, match="limb_colors"):
        viz.render(f, tracks=tr, skeleton=sk, limb_colors=np.full((2, 3), 256), radius=1)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="heat_gain"):
            viz.render(f, heat=heat, heat_gain=bad)
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="heat_alpha"):
            viz.render(f, heat=heat, heat_alpha=bad)
    with pytest.raises(ValueError, match=r"heat: \(2, K, 6, 7\) to go with the frames"):
        viz.render(f, heat=np.zeros((2, 2, 6, 8), np.float32))
    with pytest.raises(ValueError, match=r"heat: \(2, K, 6, 7\)"):
        viz.render(f, heat=np.zeros((2, 6, 7), np.float32))
    with pytest.raises(ValueError, match="K=0"):
        viz.render(f, heat=np.zeros((2, 0, 6, 7), np.float32))
    with pytest.raises(ValueError, match="K=257"):
        viz.render(f, heat=np.zeros((2, 257, 6, 7), np.float32))
    with pytest.raises(TypeError, match="heat: expected float32 or float64"):
        viz.render(f, heat=np.zeros((2, 2, 6, 7), np.float16))
    with pytest.raises(ValueError, match="heat_colors"):
        viz.render(f, heat=heat, heat_colors=np.zeros((3, 3), np.uint8))
    with pytest.raises(ValueError, match="joints"):
        viz.paint_pose(f)
    before = f.copy()
    with pytest.raises(ValueError):
        viz.render(f, tracks=tr, heat=np.ones_like(heat), skeleton=[(0, 5)], radius=1)
    assert np.array_equal(f, before)


# ---- test_cfg.pose ----------------------------------------------------------------------------------------------------------------------
def test_parse_pose():
    from fgvc_amd import engine
    assert engine.parse_pose(None) is None
    assert engine.parse_pose({}) == engine.PoseConfig(True, False)
    assert engine.parse_pose(dict(confidence=False, keep_field=True)) == engine.PoseConfig(False, True)
    with pytest.raises(ValueError, match=r"unknown key\(s\) \['min_conf'\]"):
        engine.parse_pose(dict(min_conf=0.1))
    with pytest.raises(ValueError, match="confidence"):
        engine.parse_pose(dict(confidence=1))
    with pytest.raises(ValueError, match="keep_field"):
        engine.parse_pose(dict(keep_field="yes"))
    for bad in (True, "on", [("confidence", True)]):
        with pytest.raises(TypeError, match="test_cfg.pose"):
            engine.parse_pose(bad)


def test_pose_visibles_and_tracks():
    c = np.zeros((2, 4, 3))
    c[:, 0, 1] = -1.0                                      # the reference's empty map
    c[0, 1, 0] = np.nan
    c[1, 2, 2] = np.inf
    c[0, 3, 0], c[1, 3, 0] = -1.0, 5.0                     # x == -1 alone is a coordinate
    want = np.ones((4, 3), bool)
    want[0, 1] = want[1, 0] = want[2, 2] = False
    assert np.array_equal(viz.pose_visibles(c), want) and viz.pose_visibles(c).dtype == np.bool_
    peak = np.full((4, 3), 0.5)
    peak[3, 1], peak[3, 2], peak[0, 0] = 0.25, np.nextafter(0.25, 0), np.nan
    assert np.array_equal(viz.pose_visibles(c, peak), want)                     # without min_conf the peaks are not read
    assert np.array_equal(viz.pose_visibles(c, None, 0.25), want)
    got = viz.pose_visibles(c, peak, 0.25)
    want2 = want.copy()
    want2[3, 2] = want2[0, 0] = False                      # just below; NaN.  peak == min_conf stays visible
    assert np.array_equal(got, want2) and got[3, 1]
    with pytest.raises(ValueError, match="peak"):
        viz.pose_visibles(c, peak[:3], 0.25)
    with pytest.raises(ValueError, match="coords"):
        viz.pose_visibles(np.zeros((4, 3, 2)))
    t = viz.pose_tracks(np.arange(24.0).reshape(2, 4, 3))
    assert t.shape == (4, 3, 2) and t.dtype == np.float64 and t[1, 2].tolist() == [5.0, 17.0]


def test_jhmdb_skeleton_is_a_tree_over_15_joints():
    sk = viz.JHMDB_SKELETON
    assert sk.shape == (14, 2) and sk.dtype == np.int32 and not sk.flags.writeable
    assert sk.tolist() == [[0, 1], [0, 2], [0, 3], [0, 4], [1, 5], [1, 6], [3, 7], [7, 11], [4, 8], [8, 12], [5, 9], [9, 13], [6, 10], [10, 14]]
    seen = {0}
    for a, b in sk.tolist():                               # every edge hangs a new joint onto the part already reached: connected, no cycle
        assert a in seen and b not in seen, (a, b)
        seen.add(b)
    assert seen == set(range(15))


# ---- the tools --------------------------------------------------------------------------------------------------------------------------
def test_demo_takes_the_pose_task():
    demo = _tool("demo")
    a = demo.parse_args(["--synthetic", "3", "32", "48", "--task", "pose", "--joints", "10", "8", "30", "20", "--skeleton", "0-1", "--heat",
                         "--min-conf", "0.1", "--heat-gain", "2", "--limb-width", "3", "--out", "o"])
    assert a.task == "pose" and a.joints == [10.0, 8.0, 30.0, 20.0] and a.skeleton == ["0-1"] and a.heat and a.min_conf == 0.1
    assert a.heat_gain == 2.0 and a.limb_width == 3.0
    assert demo.parse_skeleton(a.skeleton, 2).tolist() == [[0, 1]]
    assert np.array_equal(demo.parse_skeleton(["jhmdb"], 15), viz.JHMDB_SKELETON) and demo.parse_skeleton(None, 3) is None
    with pytest.raises(ValueError, match="edge 0"):
        demo.parse_skeleton(["0-2"], 2)
    with pytest.raises(ValueError, match="--skeleton"):
        demo.parse_skeleton(["0_1"], 2)
    for bad in (["--task", "pose"], ["--task", "pose", "--joints", "1", "2", "3"], ["--task", "points", "--query-points", "0", "1", "1", "--heat"],
                ["--task", "pose", "--joints", "1", "2", "--heat", "--size", "16", "24"]):
        with pytest.raises(SystemExit):
            demo.parse_args(["--synthetic", "3", "32", "48", "--out", "o", *bad])


def test_library_exports_and_header():
    from fgvc_amd import _lib, build
    assert "pose.hip" in build.SOURCES
    with open(os.path.join(ROOT, "include", "fgvc_hip.h")) as f:
        text = f.read()
    for name in ("fgvc_render_pose_u8", "fgvc_heatmap_coords_peak_f32"):
        assert name in _lib.SIGNATURES and f"int {name}(" in text, name
        assert hasattr(_lib.load(), name)
    # the shared entry's refusals name the entry that was called (no launch: the arguments are refused first)
    import ctypes
    lib, buf = _lib.load(), (ctypes.c_double * 8)()
    at = ctypes.addressof(buf)
    assert lib.fgvc_heatmap_coords_peak_f32(None, at, 0, 1, 4, 4, 0, 8, 8, 8, 8, 0, 0, 8, 8, 0, at, at, at, None) == _lib.ERR_INVALID_ARG
    assert lib.fgvc_last_error().decode().startswith("fgvc_heatmap_coords_peak_f32: bad shape")      # K = 0
    assert lib.fgvc_heatmap_coords_f32(None, at, 0, 1, 4, 4, 0, 8, 8, 8, 8, 0, 0, 8, 8, 0, at, at, None) == _lib.ERR_INVALID_ARG
    assert lib.fgvc_last_error().decode().startswith("fgvc_heatmap_coords_f32: bad shape")


def test_pose_kernel_is_scratch_free():
    """fgvc_render_pose_u8's two kernels (float32 and float64 maps) in the code-object notes of the built library: no scratch memory and no
    spilled register, vector or scalar; the LDS is the trail kernel's 26.4 KB (the same list beside the same point stage); at most 80 VGPRs,
    so that six workgroups fit a compute unit as the LDS allows."""
    notes = _tool("kernel_notes").kernel_notes()
    pose = {k: v for k, v in notes.items() if "render_pose_kernel" in k}
    trail = {k: v for k, v in notes.items() if "render_trails_kernel" in k}
    assert len(pose) == 2 and len(trail) == 1, (sorted(pose), sorted(trail))
    for k, v in pose.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 26400 and v["vgpr_count"] <= 80, (k, v)
    for k, v in trail.items():                                                  # the sibling whose stage moved to segments.hpp: as it was
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["group_segment_fixed_size"] == 26400, (k, v)
        assert v["vgpr_count"] <= 80, (k, v)
