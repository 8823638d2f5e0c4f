"""CPU tests of fgvc_amd/viz.py: the host backend is the contract the kernel is held to, so it is pinned here -- to
the reference's own painter on the two recorded fixtures with `==`, and to integer restatements of the overlay."""
import numpy as np
import pytest
import torch

from fgvc_amd import viz
from tests import render_cases as RC


@pytest.mark.parametrize("name", list(RC.FIXTURES))
def test_host_painter_equals_the_reference(name):
    g = RC.fixture(name)
    assert viz.default_radius(*g["frames"].shape[1:3]) == int(g["radius"])
    before = g["frames"].copy()
    out = viz.paint_point_track(g["frames"], g["tracks"], g["visibles"], g["colors"])
    assert out.dtype == np.uint8 and np.array_equal(out, g["out"])
    assert np.array_equal(g["frames"], before)                                    # the input is not painted on
    assert np.array_equal(RC.expected(name), g["out"])
    assert (g["out"] != g["frames"]).any() and not g["visibles"].all()
    # tensors in, and float32 tracks that hold the same values
    t32 = g["tracks"].astype(np.float32)
    want32 = viz.paint_point_track(g["frames"], t32.astype(np.float64), g["visibles"], g["colors"])
    got32 = viz.paint_point_track(torch.from_numpy(g["frames"]), torch.from_numpy(t32), torch.from_numpy(g["visibles"]), g["colors"].tolist())
    assert isinstance(got32, np.ndarray) and np.array_equal(got32, want32)


def test_order_and_truncation_decide_stacked_points():
    g = RC.fixture("ref_3x40x56")
    rev = slice(None, None, -1)
    a = viz.paint_point_track(g["frames"], g["tracks"], g["visibles"], g["colors"])
    b = viz.paint_point_track(g["frames"], g["tracks"][rev], g["visibles"][rev], g["colors"][rev])
    assert not np.array_equal(a, b)


def _case():
    c = RC.cases()["alpha_128_2x35x57"]
    return c["frames"], c["ids"], c


def test_overlay_alpha_ends_and_background():
    f, ids, _ = _case()
    pal = viz.davis_palette()
    assert np.array_equal(viz.overlay_masks(f, ids, alpha=0, contour=False), f)
    full = viz.overlay_masks(f, ids, alpha=256, contour=False)
    assert np.array_equal(full[ids > 0], pal[ids[ids > 0]])
    for alpha, contour in ((0, True), (128, True), (256, False), (37, True)):
        out = viz.overlay_masks(f, ids, alpha=alpha, contour=contour)
        assert np.array_equal(out[ids == 0], f[ids == 0])                         # id 0 is untouched
    assert (ids == 0).any() and (ids > 0).any()


def test_overlay_blend_is_exact_and_contour_is_the_4_neighbour_boundary():
    f, ids, _ = _case()
    rng = np.random.default_rng(0)
    pal = rng.integers(0, 256, (256, 3)).astype(np.uint8)
    T, H, W = ids.shape
    for alpha in (1, 128, 255):
        out = viz.overlay_masks(f, ids, palette=pal, alpha=alpha, contour=True)
        plain = viz.overlay_masks(f, ids, palette=pal, alpha=alpha, contour=False)
        n_edge = 0
        for t in range(T):
            for y in range(H):
                for x in range(W):
                    k = int(ids[t, y, x])
                    if k == 0:
                        continue
                    nb = [ids[t, yy, xx] for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)) if 0 <= yy < H and 0 <= xx < W]
                    edge = any(int(v) != k for v in nb)
                    n_edge += edge
                    blend = [(int(f[t, y, x, c]) * (256 - alpha) + int(pal[k, c]) * alpha + 128) >> 8 for c in range(3)]
                    assert plain[t, y, x].tolist() == blend
                    assert out[t, y, x].tolist() == (pal[k].tolist() if edge else blend), (t, y, x)
        assert n_edge > 20
    # per object: the contour pixels are exactly the object's pixels with a 4-neighbour outside it
    out = viz.overlay_masks(np.zeros_like(f), ids, palette=pal, alpha=0, contour=True)       # only contour pixels are non-zero (pal has no 0 row here)
    assert pal[1:].any(1).all()
    for o in range(1, int(ids.max()) + 1):
        m = np.pad(ids == o, ((0, 0), (1, 1), (1, 1)), constant_values=True)
        inner = m[:, 1:-1, :-2] & m[:, 1:-1, 2:] & m[:, :-2, 1:-1] & m[:, 2:, 1:-1]
        boundary = (ids == o) & ~inner
        assert np.array_equal(out.any(-1) & (ids == o), boundary)


def test_render_is_overlay_then_points():
    for name in ("mixed_2x35x57", "mixed_2x17x258", "no_contour_2x35x57"):
        c = RC.cases()[name]
        over = viz.overlay_masks(c["frames"], c["ids"], c.get("palette"), c.get("alpha", 128), c.get("contour", True))
        want = viz.paint_point_track(over, c["tracks"], c["visibles"], c["colors"], c["radius"])
        assert np.array_equal(RC.expected(name), want)
        assert (want != over).any() and (over != c["frames"]).any()
    c = RC.cases()["no_points_2x35x57"]
    over = viz.overlay_masks(c["frames"], c["ids"])
    assert np.array_equal(RC.expected("no_points_2x35x57"), over) and np.array_equal(RC.expected("overlay_only_2x35x57"), over)
    assert np.array_equal(RC.expected("all_invisible_2x35x57"), over)
    assert np.array_equal(RC.expected("neither_2x35x57"), c["frames"]) and RC.expected("neither_2x35x57") is not c["frames"]
    # a non-finite coordinate skips that point on that frame only
    n = RC.cases()["nan_2x35x57"]
    vis = n["visibles"] & np.isfinite(n["tracks"]).all(-1)
    assert not vis.all()
    assert np.array_equal(RC.expected("nan_2x35x57"), viz.render(**dict(n, tracks=np.nan_to_num(n["tracks"], posinf=0.0), visibles=vis)))


def test_every_case_paints_what_it_is_about():
    for name, c in RC.cases().items():
        want = RC.expected(name)
        assert want.dtype == np.uint8 and want.shape == c["frames"].shape
        changed = (want != c["frames"]).any()
        assert changed == (name not in ("neither_2x35x57",)), name
    rows, cols = RC.TILE
    c = RC.cases()["many_points_1x40x56"]
    y1, r = np.floor(c["tracks"][..., 1] + 0.5), c["radius"]                      # the windows' rows y1 - r - 1 .. y1 + r: all in one tile
    assert c["tracks"].shape[0] > 2 * 256 and y1.min() - r - 1 >= 2 * rows and y1.max() + r < 3 * rows
    assert RC.cases()["mixed_2x17x258"]["frames"].shape[2] > cols


def test_tables_are_deterministic():
    assert viz.davis_palette()[:3].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0]]
    assert viz.davis_palette().shape == (256, 3) and viz.davis_palette().dtype == np.uint8
    assert viz.davis_palette()[255].tolist() == [224, 224, 192] and len({tuple(p) for p in viz.davis_palette()}) == 256
    p = viz.davis_palette()
    p[0] = 9                                                                       # a copy: the module's table is unharmed
    assert viz.davis_palette()[0].tolist() == [0, 0, 0]
    for P in (0, 1, 2, 7, 12, 256):
        a, b = viz.track_colors(P), viz.track_colors(P)
        assert a.shape == (P, 3) and a.dtype == np.uint8 and np.array_equal(a, b)
        assert len({tuple(c) for c in a}) == P
    icon = viz.icon_table(2)
    assert icon.shape == (5, 5) and icon.dtype == np.float64 and 0.0 <= icon.min() and icon.max() == 1.0
    assert icon[3, 3] == 1.0 and icon[0, 0] == 0.0                                # off centre by one, as the reference's
    assert viz.default_radius(480, 854) == 7 and viz.default_radius(100, 104) == 2 and viz.default_radius(33, 90) == 0


def test_refusals():
    g = RC.fixture("ref_3x40x56")
    f, tr, vis, col = g["frames"], g["tracks"], g["visibles"], g["colors"]
    with pytest.raises(ValueError, match="radius"):
        viz.paint_point_track(f, tr, vis, col, radius=0)
    with pytest.raises(ValueError, match="radius"):
        viz.paint_point_track(f[:, :30], tr, vis, col)                            # under 34 px the reference's radius is 0
    with pytest.raises(ValueError, match="radius"):
        viz.paint_point_track(f, tr, vis, col, radius=32)
    with pytest.raises(TypeError, match="uint8"):
        viz.paint_point_track(f.astype(np.float32), tr, vis, col)
    with pytest.raises(ValueError, match="frames"):
        viz.paint_point_track(f[..., :2], tr, vis, col)
    with pytest.raises(ValueError, match="point_tracks"):
        viz.paint_point_track(f, tr[:, :2], vis, col)
    with pytest.raises(ValueError, match="point_tracks"):
        viz.paint_point_track(f, tr.transpose(1, 0, 2)[:, :5], vis, col)
    with pytest.raises(TypeError, match="bool"):
        viz.paint_point_track(f, tr, vis.astype(np.uint8), col)
    with pytest.raises(ValueError, match="visibles"):
        viz.paint_point_track(f, tr, vis[:5], col)
    with pytest.raises(TypeError, match="colors"):
        viz.paint_point_track(f, tr, vis, col.astype(np.float64))
    with pytest.raises(ValueError, match="colors"):
        viz.paint_point_track(f, tr, vis, col[:5])
    with pytest.raises(ValueError, match="colors"):
        viz.paint_point_track(f, tr, vis, col.astype(np.int64) + 200)
    ids = np.zeros(f.shape[:3], np.uint8)
    for alpha in (-1, 257, 12.5):
        with pytest.raises(ValueError, match="alpha"):
            viz.overlay_masks(f, ids, alpha=alpha)
    with pytest.raises(TypeError, match="ids"):
        viz.overlay_masks(f, ids.astype(np.int64))
    with pytest.raises(ValueError, match="ids"):
        viz.overlay_masks(f, ids[:, :-1])
    with pytest.raises(ValueError, match="palette"):
        viz.overlay_masks(f, ids, palette=np.zeros((4, 3), np.uint8))
    with pytest.raises(TypeError, match="palette"):
        viz.overlay_masks(f, ids, palette=np.zeros((256, 3), np.float32))
    with pytest.raises(ValueError, match="backend"):
        viz.render(f, backend="cuda")


def test_scale_tracks():
    tr = np.array([[[10.0, 20.0], [0.5, 0.25]]], np.float32)
    out = viz.scale_tracks(tr, (256, 256), (480, 854))
    assert out.dtype == np.float64 and out.shape == tr.shape
    assert np.array_equal(out, np.array([[[10.0 * (854 / 256), 20.0 * (480 / 256)], [0.5 * (854 / 256), 0.25 * (480 / 256)]]]))
    assert np.array_equal(viz.scale_tracks(torch.from_numpy(tr), (48, 64), (48, 64)), tr.astype(np.float64))
    assert tr[0, 0, 0] == 10.0                                                    # the input is not scaled in place
    with pytest.raises(ValueError, match="tracks"):
        viz.scale_tracks(np.zeros((3, 3)), (1, 1), (2, 2))
    with pytest.raises(ValueError, match="positive"):
        viz.scale_tracks(tr, (0, 4), (2, 2))


def test_tile_constants_agree():
    from fgvc_amd import _lib, ops
    lib = _lib.load()
    assert (lib.fgvc_render_tile_rows(), lib.fgvc_render_tile_cols()) == ops.RENDER_TILE == RC.TILE
    assert ops.RENDER_MAX_RADIUS == viz.MAX_RADIUS


def test_entry_refuses_bad_arguments_before_any_launch():
    """Error codes from the C entry, no GPU needed: the checks come before the launch."""
    import ctypes
    from fgvc_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    # each entry's own arguments after `icon`, valid; trails: trail, linewidth, ro2, g, fade, time_colors; pose: no limbs, no maps
    tails = {"fgvc_render_frames_u8": (), "fgvc_render_trails_u8": (1, 2.0, 2.25, 0.5, p, None),
             "fgvc_render_pose_u8": (None, 0, None, 2.0, 2.25, 0.5, 1.0, None, 0, 0, 0, 0, 0, None, 1.0, 0.5)}

    def call(entry="fgvc_render_frames_u8", frames=p, f_sy=12, out=p, o_st=48, o_sy=12, T=2, h=4, w=4, ids=None, i_sy=4, pal=None, alpha=128,
             tracks=None, colors=None, P=0, radius=2, icon=None, tail=None):
        return getattr(lib, entry)(frames, 48, f_sy, out, o_st, o_sy, T, h, w, ids, 16, i_sy, pal, alpha, 1, tracks, 4, 2, None, 0, 0, colors, P,
                                   radius, icon, *(tails[entry] if tail is None else tail), None)
    # what the three entries refuse alike, each under its own name
    for entry in tails:
        for kw, code, text in ((dict(frames=None), 1, b"null pointer"), (dict(out=None), 1, b"null pointer"), (dict(T=-1), 1, b"negative size"),
                               (dict(P=-1), 1, b"P=-1"), (dict(f_sy=11), 1, b"row stride"), (dict(o_sy=11), 1, b"overlap"),
                               (dict(o_st=47), 1, b"overlap"), (dict(ids=p), 1, b"palette"), (dict(ids=p, pal=p, alpha=257), 1, b"alpha"),
                               (dict(ids=p, pal=p, i_sy=3), 1, b"row stride"), (dict(h=1 << 15, w=1 << 14), 1, b"2^29")):
            assert call(entry, **kw) == code, (entry, kw, lib.fgvc_last_error())
            assert text in lib.fgvc_last_error() and lib.fgvc_last_error().startswith(entry.encode() + b": "), (entry, kw, lib.fgvc_last_error())
        assert call(entry, T=0) == 0 and call(entry, h=0) == 0                    # nothing to do: no launch
    # what the points need differs between the entries: frames wants the radius, colors and the icon whenever there are tracks ...
    for kw, code, text in ((dict(tracks=p, colors=p, icon=p, P=1, radius=0), 1, b"radius"),
                           (dict(tracks=p, colors=p, icon=p, P=1, radius=32), 2, b"radius"), (dict(tracks=p, P=1), 1, b"colors")):
        assert call(**kw) == code and text in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())
        assert lib.fgvc_last_error().startswith(b"fgvc_render_frames_u8: ")
    # ... trails reads the radius only with an icon (no icon: no dots), and takes time_colors in place of colors then
    trails = dict(entry="fgvc_render_trails_u8", tracks=p, P=1)
    assert call(**trails, colors=p, icon=p, radius=0) == 1 and lib.fgvc_last_error().startswith(b"fgvc_render_trails_u8: radius=0")
    assert call(**trails, colors=p, icon=p, radius=32) == 2 and b"radius" in lib.fgvc_last_error()
    assert call(**trails) == 1 and b"neither colors nor time_colors" in lib.fgvc_last_error()
    assert call(**trails, icon=p, tail=(1, 2.0, 2.25, 0.5, p, p)) == 1 and b"neither colors nor time_colors" in lib.fgvc_last_error()
    assert call(**trails, T=0, colors=p, radius=0) == 0                           # (accepted cases at T = 0: nothing is launched)
    assert call(**trails, T=0, radius=0, tail=(1, 2.0, 2.25, 0.5, p, p)) == 0
    # at T = 2 the same two get as far as the entry's last check, the alignment of `fade`: neither the radius nor the colours stopped them
    odd = ctypes.c_void_p(p.value + 4)
    for kw in (dict(colors=p, tail=(1, 2.0, 2.25, 0.5, odd, None)), dict(tail=(1, 2.0, 2.25, 0.5, odd, p))):
        assert call(**trails, radius=0, **kw) == 1 and b"8-byte aligned" in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())


def test_hip_backend_without_a_gpu_raises(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                # (this test is the same on a GPU box)
    g = RC.fixture("ref_3x40x56")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        viz.paint_point_track(g["frames"], g["tracks"], g["visibles"], g["colors"], backend="hip")
    with pytest.raises(RuntimeError, match="needs a GPU"):
        viz.render(g["frames"], backend="hip")
