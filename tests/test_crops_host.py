"""CPU tests of the two host contracts of the object crops: metrics.object_windows_host against windows worked out
by hand (tests/crops_cases.py), viz.crop_windows_host against Pillow's Image.resize(size, BILINEAR, box=window) with `==`, and the layers
around them (ObjectTracks.windows / crops on host statistics, ObjectCrops.to_crop / from_crop, viz.contact_sheet, the refusals)."""
import numpy as np
import pytest

from tests import crops_cases as CC


@pytest.mark.parametrize("name", list(CC.window_cases()))
def test_window_rule_equals_the_hand_computed_windows(name):
    from fgvc_amd import metrics
    stats, kw, want = CC.window_cases()[name]
    got = metrics.object_windows_host(stats, **kw)
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got, want), (name, got.tolist(), want.tolist())


def test_window_rule_properties_on_random_statistics():
    """the window holds every box of U, keeps the output's aspect from above, and the frame-space window holds the scaled mask-space one"""
    from fgvc_amd import metrics
    ids = CC.blob_ids(5, 64, 96, 3)
    stats = metrics.object_stats_host(ids, 4)
    for size in ((16, 16), (5, 7), (33, 48)):
        for smooth in (0, 1, 7):
            win = metrics.object_windows_host(stats, size, pad=0.3, min_side=4, smooth=smooth, mask_size=(64, 96), frame_size=(144, 216))
            assert win.shape == (5, 3, 8)
            for t in range(5):
                for j in range(3):
                    x0, y0, x1, y1, X0, Y0, X1, Y1 = win[t, j].tolist()
                    if stats[t, j + 1, 0] == 0:
                        assert not win[t, j].any()
                        continue
                    bx0, by0, bx1, by1 = stats[t, j + 1, 1:5].tolist()
                    assert x1 - x0 >= bx1 - bx0 and y1 - y0 >= by1 - by0
                    if smooth == 0:
                        assert x0 <= bx0 and bx1 <= x1 and y0 <= by0 and by1 <= y1
                    Wp, Hp = x1 - x0, y1 - y0
                    assert Wp * size[0] >= (Hp - 1) * size[1] and Hp * size[1] >= (Wp - 1) * size[0]
                    assert X0 * 96 <= x0 * 216 < (X0 + 1) * 96 and (X1 - 1) * 96 < x1 * 216 <= X1 * 96
                    assert Y0 * 64 <= y0 * 144 < (Y0 + 1) * 64 and (Y1 - 1) * 64 < y1 * 144 <= Y1 * 64


def _pillow(frame, window, size, fill, pad=0):
    from PIL import Image
    H, W, _ = frame.shape
    f = frame
    if pad:
        f = np.empty((H + 2 * pad, W + 2 * pad, 3), np.uint8)
        f[...] = fill
        f[pad:pad + H, pad:pad + W] = frame
    x0, y0, x1, y1 = (int(v) + pad for v in window)
    return np.asarray(Image.fromarray(f).resize((size[1], size[0]), Image.BILINEAR, box=(x0, y0, x1, y1)))


def _taps_inside(window, size, H, W) -> bool:
    from fgvc_amd import viz
    x0, y0, x1, y1 = (int(v) for v in window)
    (lx, kx), (ly, ky) = viz.crop_axis_coefficients(x0, x1, size[1]), viz.crop_axis_coefficients(y0, y1, size[0])
    return lx[0] >= 0 and ly[0] >= 0 and lx[-1] + len(kx[-1]) <= W and ly[-1] + len(ky[-1]) <= H


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_resampling_rule_equals_pillow_inside_the_frame(seed):
    pytest.importorskip("PIL")
    from fgvc_amd import viz
    rng = np.random.default_rng(seed)
    done = 0
    while done < 40:
        H, W = (int(v) for v in rng.integers(5, 40, 2))
        f = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        win = CC.random_windows(1, 1, H, W, int(rng.integers(1 << 30)), inside=True)
        size = tuple(int(v) for v in rng.integers(1, 24, 2))
        # on the bare frame Pillow cuts the taps at the frame's edge and renormalises; the rule reads `fill` there (the padded frame of
        # the next test).  The two agree where no tap leaves the frame: the windows drawn here are those.
        if not _taps_inside(win[0, 0], size, H, W):
            continue
        done += 1
        got = viz.crop_windows_host(f, win, size, fill=np.array([255, 0, 255], np.uint8))[0, 0]
        want = _pillow(f[0], win[0, 0], size, None)
        assert np.array_equal(got, want), (H, W, win.tolist(), size)


@pytest.mark.parametrize("seed", (4, 5, 6))
def test_resampling_rule_equals_pillow_on_a_fill_padded_frame(seed):
    pytest.importorskip("PIL")
    from fgvc_amd import viz
    rng = np.random.default_rng(seed)
    outside = 0
    for _ in range(40):
        H, W = (int(v) for v in rng.integers(5, 40, 2))
        f = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)
        win = CC.random_windows(1, 1, H, W, int(rng.integers(1 << 30)))
        x0, y0, x1, y1 = win[0, 0].tolist()
        outside += x0 < 0 or y0 < 0 or x1 > W or y1 > H
        size = tuple(int(v) for v in rng.integers(1, 24, 2))
        fill = rng.integers(0, 256, 3, dtype=np.uint8)
        got = viz.crop_windows_host(f, win, size, fill=fill)[0, 0]
        want = _pillow(f[0], win[0, 0], size, fill, pad=160)
        assert np.array_equal(got, want), (H, W, win.tolist(), size, fill.tolist())
    assert outside >= 10


@pytest.mark.parametrize("H,W", CC.FRAME_SIZES)
def test_named_windows_equal_pillow(H, W):
    """the windows of the GPU tests, through the padded frame: the device is held to a contract that Pillow confirms on these very cases"""
    pytest.importorskip("PIL")
    fill = (9, 200, 77)
    for S_h, S_w in CC.SIZES:
        got = CC.expected_crops(1, H, W, S_h, S_w, fill)
        for j, (name, win) in enumerate(CC.named_windows(H, W, S_h, S_w).items()):
            if win[2] <= win[0] or win[3] <= win[1]:
                assert (got[0, j] == np.asarray(fill, np.uint8)).all(), name
                continue
            reach = max(0, -win[0], -win[1], win[2] - W, win[3] - H) + max((win[2] - win[0]) // S_w, (win[3] - win[1]) // S_h) + 3
            want = _pillow(CC.frames(1, H, W)[0], win, (S_h, S_w), np.asarray(fill, np.uint8), pad=reach)
            assert np.array_equal(got[0, j], want), (name, (S_h, S_w))


def test_identity_window_returns_the_pixels():
    from fgvc_amd import viz
    f = CC.frames(2, 37, 53)
    for S_h, S_w in ((1, 1), (5, 7), (16, 16), (37, 53)):
        win = np.array([[[4, 2, 4 + S_w, 2 + S_h]], [[0, 0, S_w, S_h]]])
        if S_h == 37:
            win[0, 0] = (0, 0, 53, 37)
        got = viz.crop_windows_host(f, win, (S_h, S_w))
        for t in range(2):
            x0, y0, x1, y1 = win[t, 0].tolist()
            assert np.array_equal(got[t, 0], f[t, y0:y1, x0:x1])


def test_constant_frame_returns_the_constant():
    from fgvc_amd import viz
    f = np.empty((1, 120, 150, 3), np.uint8)
    f[...] = (3, 128, 255)
    colour = np.array([3, 128, 255], np.uint8)
    win = CC.random_windows(1, 30, 40, 50, 11, inside=True) + np.array([50, 40, 50, 40])       # a margin of 40 pixels all around
    for size in ((1, 1), (7, 5), (23, 19)):
        # where no tap leaves the frame the fill cannot show; with the constant as fill, any window at all returns it
        assert all(_taps_inside(w, size, 120, 150) for w in win[0])
        got = viz.crop_windows_host(f, win, size, fill=np.array([90, 90, 90], np.uint8))
        assert (got == colour).all()
        anywhere = CC.random_windows(1, 30, 120, 150, 12)
        assert (viz.crop_windows_host(f, anywhere, size, fill=colour) == colour).all()


def test_invalid_and_too_large_windows_give_fill_and_empty_masks():
    from fgvc_amd import viz
    f = CC.frames(1, 37, 53)
    ids = np.ones((1, 37, 53), np.uint8)
    win = np.array([[[5, 5, 5, 9], [9, 5, 3, 9], [0, 0, 40, 30], [0, 0, 2 ** 30, 8], [2, 2, 12, 12]]])
    fill = np.array([1, 2, 3], np.uint8)
    crops, masks = viz.crop_windows_host(f, win, (4, 4), fill=fill, ids=ids, objects=[1] * 5, max_taps=8)
    for j in (0, 1, 2, 3):                      # empty, reversed, 40 / 4 = 10 -> 22 taps > 8, a coordinate at the limit
        assert (crops[0, j] == fill).all() and not masks[0, j].any(), j
    assert masks[0, 4].all() and not (crops[0, 4] == fill).all()
    assert viz.crop_axis_taps(40, 4) == 22 and viz.crop_axis_taps(3, 16) == 4 and viz.crop_axis_taps(85, 16) == 14
    unlimited = viz.crop_windows_host(f, win, (4, 4), fill=fill)
    assert not (unlimited[0, 2] == fill).all() and np.array_equal(unlimited[0, 4], crops[0, 4])
    assert viz.crop_window_ok(0, 0, 40, 30, (4, 4)) and not viz.crop_window_ok(0, 0, 40, 30, (4, 4), 8)
    assert viz.crop_default_taps((37, 53), (4, 4)) == 2 * 27 + 2 and viz.crop_default_taps((480, 854), (1, 1)) == viz.CROP_MAX_TAPS


def test_tap_bound_holds_for_every_output():
    from fgvc_amd import viz
    rng = np.random.default_rng(5)
    for _ in range(200):
        a0 = int(rng.integers(-50, 50))
        span, n = int(rng.integers(1, 300)), int(rng.integers(1, 40))
        los, Ks = viz.crop_axis_coefficients(a0, a0 + span, n)
        assert max(len(k) for k in Ks) <= viz.crop_axis_taps(span, n)
        assert (np.diff(los) >= 0).all() and (np.diff([lo + len(k) for lo, k in zip(los, Ks)]) >= 0).all()
        assert all(abs(int(k.sum()) - (1 << 22)) <= len(k) for k in Ks)


def test_masks_sample_the_nearest_pixel_of_the_mask_window():
    from fgvc_amd import viz
    ids = np.zeros((1, 8, 12), np.uint8)
    ids[0, 2:6, 3:9] = 2
    f = np.zeros((1, 16, 24, 3), np.uint8)
    win = np.array([[[2, 1, 10, 7, 4, 2, 20, 14], [-2, -2, 2, 2, -4, -4, 4, 4]]])      # mask-space words first, frame-space last
    crops, masks = viz.crop_windows_host(f, win, (6, 8), ids=ids, objects=[2, 0])
    # window 8 x 6 onto 8 x 6 outputs: mx = 2 + ((2 xx + 1) * 8) // 16 = 2 + xx, my = 1 + yy
    assert np.array_equal(masks[0, 0], np.where(ids[0, 1:7, 2:10] == 2, 255, 0))
    # object 0 (the background) in a window that starts outside the map: outside is 0, never a clamped sample
    # mx = -2 + ((2 xx + 1) * 4) // 16 for xx = 0 .. 7 = -2, -2, -1, -1, 0, 0, 1, 1; my = -2 + ((2 yy + 1) * 4) // 12 = -2, -1, -1, 0, 1, 1
    want = np.zeros((6, 8), np.uint8)
    want[3:, 4:] = 255
    assert np.array_equal(masks[0, 1], want)


def test_object_tracks_chain_on_host_statistics():
    from fgvc_amd import engine, metrics, viz
    ids = CC.blob_ids(3, 37, 53, 1)
    f = CC.frames(3, 37, 53)
    tracks = engine.ObjectTracks(metrics.object_stats_host(ids, 4))
    win = tracks.windows((16, 16), mask_size=(37, 53))
    assert isinstance(win, np.ndarray) and win.shape == (3, 3, 8)
    oc = tracks.crops(f, size=(16, 16), masks=True, ids=ids, fill=(7, 7, 7))
    assert isinstance(oc, engine.ObjectCrops) and oc.size == (16, 16) and oc.objects == [1, 2, 3]
    assert np.array_equal(oc.windows, win)
    want, wm = viz.crop_windows_host(f, win, (16, 16), fill=np.array([7, 7, 7], np.uint8), ids=ids, objects=[1, 2, 3])
    assert np.array_equal(oc.crops, want) and np.array_equal(oc.masks, wm)
    assert oc.valid.tolist() == (metrics.object_stats_host(ids, 4)[:, 1:, 0] > 0).tolist() and not oc.valid[1, 1]
    assert (oc.crops[1, 1] == 7).all() and not oc.masks[1, 1].any()
    # every present object's mask is mostly the object: the window is centred on it
    assert all(oc.masks[t, j].any() for t in range(3) for j in range(3) if oc.valid[t, j])
    chw = tracks.crops(np.ascontiguousarray(f.transpose(0, 3, 1, 2)), size=(16, 16), layout="tchw", fill=(7, 7, 7))
    assert chw.masks is None and np.array_equal(chw.crops, want)
    one = tracks.crops(f, size=(5, 7), objects=[3])
    assert one.crops.shape == (3, 1, 5, 7, 3) and one.objects == [3]


def test_to_crop_and_from_crop_invert_each_other():
    from fgvc_amd import engine
    win = np.array([[[1, 16, 39, 54, 2, 36, 88, 122], [0] * 8]], np.int64)
    oc = engine.ObjectCrops(np.zeros((1, 2, 16, 32, 3), np.uint8), None, win, [1, 2], (16, 32))
    assert np.allclose(oc.to_crop([[2.0, 36.0], [88.0, 122.0]], 0, 0), [[0, 0], [32, 16]])
    assert np.allclose(oc.to_crop([2.0, 36.0], 0, 0, pixel_centers=True), [0.5 * 32 / 86 - 0.5, 0.5 * 16 / 86 - 0.5])
    pts = np.random.default_rng(0).uniform(-50, 300, (7, 2))
    for centers in (False, True):
        assert np.allclose(oc.from_crop(oc.to_crop(pts, 0, 0, centers), 0, 0, centers), pts)
        assert np.allclose(oc.to_crop(oc.from_crop(pts, 0, 0, centers), 0, 0, centers), pts)
    with pytest.raises(ValueError, match="empty"):
        oc.to_crop([0.0, 0.0], 0, 1)
    with pytest.raises(ValueError, match="xy"):
        oc.from_crop([0.0, 0.0, 1.0], 0, 0)
    assert oc.valid.tolist() == [[True, False]]


def test_contact_sheet_shapes():
    from fgvc_amd import viz
    crops = np.arange(3 * 2 * 4 * 5 * 3, dtype=np.uint8).reshape(3, 2, 4, 5, 3)
    sheet = viz.contact_sheet(crops)
    assert sheet.shape == (3 * 4, 2 * 5, 3) and np.array_equal(sheet[4:8, 5:10], crops[1, 1])
    wide = viz.contact_sheet(crops, cols=4)
    assert wide.shape == (2 * 4, 4 * 5, 3) and np.array_equal(wide[4:8, 5:10], crops[2, 1]) and not wide[4:8, 10:].any()
    valid = np.ones((3, 2), bool)
    valid[1, 1] = False
    masked = viz.contact_sheet(crops, valid=valid)
    assert not masked[4:8, 5:10].any() and np.array_equal(masked[8:12, 5:10], crops[2, 1])
    assert viz.contact_sheet(crops[:, :1], cols=1).shape == (12, 5, 3)
    with pytest.raises(ValueError, match="crops"):
        viz.contact_sheet(crops[0])
    with pytest.raises(ValueError, match="cols"):
        viz.contact_sheet(crops, cols=0)
    with pytest.raises(ValueError, match="valid"):
        viz.contact_sheet(crops, valid=np.ones((2, 3), bool))


def test_every_refusal_is_by_name():
    from fgvc_amd import engine, metrics, viz
    stats = CC.window_cases()["one_frame_one_object"][0]
    ok = dict(size=(16, 16), mask_size=(64, 96))
    for bad, name in ((dict(size=(0, 16)), "size"), (dict(size=(16, 1025)), "size"), (dict(size=16), "size"), (dict(pad=-0.1), "pad"),
                      (dict(pad=4.5), "pad"), (dict(pad=float("nan")), "pad"), (dict(min_side=0), "min_side"), (dict(smooth=-1), "smooth"),
                      (dict(mask_size=(32769, 96)), "mask_size h"), (dict(mask_size=(64, 40000)), "mask_size w"),
                      (dict(frame_size=(32769, 96)), "frame_size H"), (dict(frame_size=(64, 0)), "frame_size W"),
                      (dict(objects=[2]), "objects"), (dict(objects=[-1]), "objects"), (dict(mask_size=None), "mask_size")):
        with pytest.raises(ValueError, match=name):
            metrics.object_windows_host(stats, **{**ok, **bad})
    with pytest.raises(ValueError, match="stats"):
        metrics.object_windows_host(stats.astype(np.int32), **ok)
    f = CC.frames(1, 37, 53)
    win = np.array([[[0, 0, 8, 8]]])
    for args, kw, name in (((f[0], win, (4, 4)), {}, "frames"), ((f, win[0], (4, 4)), {}, "windows"), ((f, win.astype(float), (4, 4)), {}, "windows"),
                           ((f, win, (0, 4)), {}, "size"), ((f, win, (4, 2000)), {}, "size"), ((f, win, (4, 4)), dict(fill=[1, 2]), "fill"),
                           ((f, win, (4, 4)), dict(ids=np.zeros((1, 5, 5), np.uint8)), "ids and objects"),
                           ((f, win, (4, 4)), dict(ids=np.zeros((1, 5, 5), np.uint8), objects=[1, 2]), "ids")):
        with pytest.raises(ValueError, match=name):
            viz.crop_windows_host(*args, **kw)
    tracks = engine.ObjectTracks(stats)
    with pytest.raises(ValueError, match="masks=True needs ids"):
        tracks.crops(f, masks=True)
    with pytest.raises(ValueError, match="layout"):
        tracks.crops(f, layout="hwc")
    with pytest.raises(ValueError, match="objects"):
        tracks.crops(f, objects=[5])
