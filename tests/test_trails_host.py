"""CPU tests of the motion trails: viz's host backend -- the contract the kernel is held to in tests/test_gpu_trails.py
-- against hand-checkable bytes and against the plain restatement of tests/trails_cases.py, the tables, and every refusal."""
import numpy as np
import pytest

from fgvc_amd import viz
from tests import render_cases as RC
from tests import trails_cases as TC

NAMES = list(TC.cases())


def _one_segment(linewidth):
    """A white segment from (2.5, 4.5) to (9.5, 4.5) in track coordinates -- (3, 5) to (10, 5) on the pixel grid -- on frame 1 of a black clip."""
    frames = np.zeros((2, 10, 14, 3), np.uint8)
    tracks = np.array([[(2.5, 4.5), (9.5, 4.5)]])
    out = viz.paint_trails(frames, tracks, colors=np.array([[255, 255, 255]]), trail=1, linewidth=linewidth, fade=np.array([1.0]), dots=False)
    assert out.dtype == np.uint8 and out.shape == frames.shape and not out[0].any()            # frame 0 has no history
    assert (out[1][..., 0] == out[1][..., 1]).all() and (out[1][..., 0] == out[1][..., 2]).all()
    return out[1][..., 0]


def test_hand_checked_bytes_linewidth_1():
    img = _one_segment(1.0)                                  # ro = 1, ri = 0: cov = 1 - d2
    want = np.zeros((10, 14), np.uint8)
    want[5, 3:11] = 255                                      # d2 = 0 on the row; d2 = 1 in the rows above and below and past the caps: nothing
    assert np.array_equal(img, want), img


def test_hand_checked_bytes_linewidth_2():
    img = _one_segment(2.0)                                  # ro = 1.5, ri = 0.5: cov = (2.25 - d2) / 2
    want = np.zeros((10, 14), np.uint8)
    want[5, 3:11] = 255
    want[4, 3:11] = want[6, 3:11] = int(0.625 * 255)         # d2 = 1: 159
    want[5, 2] = want[5, 11] = 159                           # past the end caps d2 is the distance to the end point: 1 ...
    for y in (4, 6):
        want[y, 2] = want[y, 11] = int(0.125 * 255)          # ... 2 on the diagonal: 31 ...
    assert int(0.625 * 255) == 159 and np.array_equal(img, want), img                          # ... and 4 two pixels out: nothing


@pytest.mark.parametrize("name", NAMES)
def test_host_backend_equals_the_restatement(name):
    got, want = TC.expected(name), TC.restated(name)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{name}: {len(bad)} bytes differ; first (t, y, x, c) {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    c = TC.cases()[name]
    if c["tracks"].shape[0] and c["frames"].shape[0] > 1:
        assert (got != TC.render(c, trail=None) if c.get("dots", True) else got != c["frames"]).any(), "the case draws no trail"


def test_pixels_beyond_the_box_keep_their_value():
    """the restatement over every pixel of the image, not only those near a segment: the same bytes"""
    for name in ("degenerate_4x12x20", "mixed_3x35x57_no_dots"):
        assert np.array_equal(TC.restate(TC.cases()[name], whole_image=True), TC.restated(name)), name


def test_cases_reach_what_they_are_for():
    c = TC.cases()["rounds_6x20x40"]
    P, T = c["tracks"].shape[:2]
    lo, hi = c["tracks"][..., 1].min() + 0.5, c["tracks"][..., 1].max() + 0.5
    assert P * min(T - 1, c["trail"]) > 256 and TC.TILE[0] <= lo and hi < 2 * TC.TILE[0]       # more than one round of items, all in one tile
    flipped = dict(c, tracks=c["tracks"][::-1], colors=c["colors"][::-1])
    assert (TC.render(flipped) != TC.expected("rounds_6x20x40")).any(), "the order of the points does not show"
    c = TC.cases()["cross_5x17x258_w2"]
    a = c["tracks"] + 0.5
    assert (a[..., 0] == TC.TILE[1]).any() and (a[..., 1] == TC.TILE[0]).any() and (a[..., 1] == 2 * TC.TILE[0]).any()
    assert (a[..., 0] < 0).any() and (a[..., 0] > 258).any() and (a[..., 1] < 0).any() and (a[..., 1] > 17).any()
    d = TC.cases()["degenerate_4x12x20"]
    assert np.isnan(d["tracks"]).any() and np.isinf(d["tracks"]).any() and (np.abs(d["tracks"]) == 1e30).any() and not d["visibles"].all()
    assert np.array_equal(TC.expected("degenerate_1x12x20"), TC.render(TC.cases()["degenerate_1x12x20"], trail=None))      # T = 1: the dots alone
    assert np.array_equal(TC.expected("degenerate_4x12x20_p0"), d["frames"])


@pytest.mark.parametrize("name", list(RC.cases()))
def test_trail_none_is_todays_render(name):
    c = RC.cases()[name]
    assert np.array_equal(viz.render(trail=None, linewidth=3.0, trail_fade=None, trail_color_by="time", **c), RC.expected(name))


def test_paint_trails_is_render_with_a_trail():
    c = TC.cases()["mixed_3x35x57"]
    got = viz.paint_trails(c["frames"], c["tracks"], c["visibles"], c["colors"], trail=2, linewidth=2.5, radius=2)
    want = viz.render(c["frames"], tracks=c["tracks"], visibles=c["visibles"], colors=c["colors"], radius=2, trail=2, linewidth=2.5)
    assert np.array_equal(got, want)
    small = c["frames"][:, :20, :20]                        # under 34 px the default radius is 0: needed for the dots only
    assert viz.paint_trails(small, c["tracks"], dots=False).shape == small.shape
    with pytest.raises(ValueError, match="radius"):
        viz.paint_trails(small, c["tracks"])


def test_spring_colors():
    assert viz.spring_colors(1).shape == (0, 3) and viz.spring_colors(2).tolist() == [[255, 0, 255]]
    assert viz.spring_colors(4).tolist() == [[255, 0, 255], [255, 128, 127], [255, 255, 0]]
    for T in (2, 3, 8, 50, 300, 600):
        s = viz.spring_colors(T)
        assert s.dtype == np.uint8 and s.shape == (T - 1, 3)
        k = np.minimum((np.arange(T - 1) / max(1, T - 2) * 256).astype(np.int64), 255)
        assert np.array_equal(s, np.stack([np.full(T - 1, 255), k, 255 - k], -1))


def test_spring_colors_are_matplotlibs():
    matplotlib = pytest.importorskip("matplotlib")
    cm = pytest.importorskip("matplotlib.cm")
    spring = matplotlib.colormaps["spring"] if hasattr(matplotlib, "colormaps") else cm.get_cmap("spring")    # (get_cmap: deprecated in 3.7)
    for T in (2, 3, 8, 50, 300):
        want = [[int(round(v * 255)) for v in spring(s / max(1, T - 2))[:3]] for s in range(T - 1)]
        assert viz.spring_colors(T).tolist() == want, T


def test_trail_fade():
    assert viz.trail_fade(1).tolist() == [1.0] and viz.trail_fade(4).tolist() == [1.0, 0.75, 0.5, 0.25]
    f = viz.trail_fade(64)
    assert f.dtype == np.float64 and f.shape == (64,) and f[0] == 1.0 and f[63] == 1 / 64 and viz.trail_fade(64) is f
    with pytest.raises(ValueError):
        f[0] = 0.0                                           # read-only, like icon_table
    for bad in (0, 65):
        with pytest.raises(ValueError, match="trail"):
            viz.trail_fade(bad)
    ro2, g, reach = viz.trail_consts(2.0)
    assert (ro2, g, reach) == (2.25, 0.5, 2) and viz.trail_consts(1.0) == (1.0, 1.0, 1) and viz.trail_consts(3.5)[2] == 3


def test_refusals():
    c = TC.cases()["mixed_3x35x57"]
    kw = dict(frames=c["frames"], tracks=c["tracks"], radius=2)
    for bad in (0, 65, -1, 2.0, "8", True):
        with pytest.raises(ValueError, match="trail"):
            viz.render(trail=bad, **kw)
    assert viz.render(trail=64, **kw).shape == c["frames"].shape                               # longer than the clip: fine
    for bad in (0.5, 16.5, float("nan"), None):
        with pytest.raises(ValueError, match="linewidth"):
            viz.render(trail=2, linewidth=bad, **kw)
    for bad in (np.ones(3), np.ones((2, 1)), np.array([0.5, 1.5]), np.array([-0.1, 0.5]), np.array([np.nan, 0.5])):
        with pytest.raises(ValueError, match="trail_fade"):
            viz.render(trail=2, trail_fade=bad, **kw)
    with pytest.raises(ValueError, match="trail_color_by"):
        viz.render(trail=2, trail_color_by="spring", **kw)
    with pytest.raises(ValueError, match="tracks"):
        viz.render(c["frames"], trail=2)
    with pytest.raises(ValueError, match="tracks"):
        viz.render(c["frames"], ids=c["ids"], trail=2)
    with pytest.raises(ValueError, match="point_tracks"):
        viz.paint_trails(c["frames"], None)
    with pytest.raises(ValueError, match="trail"):
        viz.paint_trails(c["frames"], c["tracks"], trail=None, radius=2)
    with pytest.raises(ValueError, match="backend"):
        viz.render(trail=2, backend="cuda", **kw)
