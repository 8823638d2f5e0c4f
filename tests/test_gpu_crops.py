"""GPU tests of the object crops: fgvc_seg_object_windows_i64 against metrics.object_windows_host and
fgvc_frames_object_crops_u8 against viz.crop_windows_host, both with `==` -- the windows are integers and the resampler's float64 half is
held operation for operation, so there is no tolerance anywhere in this file.  The cases are those of tests/crops_cases.py, which
tests/test_crops_host.py holds to hand-computed windows and to Pillow on the CPU."""
import numpy as np
import pytest
import torch

from tests import crops_cases as CC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _report(name, got, want):
    bad = np.argwhere(got != want)
    first = tuple(bad[0]) if len(bad) else ()
    return f"{name}: {len(bad)} elements differ; first {bad[:4].tolist()}: got {got[first] if first else ''}, want {want[first] if first else ''}"


def _same(name, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(got, want), _report(name, got, want)


# ---- the resampler on explicit windows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", CC.SIZES)
@pytest.mark.parametrize("T,H,W", [(1, 37, 53), (3, 64, 96), (5, 37, 53), (1, 64, 96)])
def test_named_windows_equal_the_contract(dev, T, H, W, size):
    """upscaling, downscaling by about 5.3 and by 12 on one axis, every border and corner, windows outside the frame, one-pixel sides,
    invalid windows, on every size: within a band, across bands, with a ragged last band and ragged column chunks"""
    from fgvc_amd import ops, viz
    S_h, S_w = size
    taps = viz.crop_default_taps((H, W), size)
    want = CC.expected_crops(T, H, W, S_h, S_w, (0, 0, 0), taps)
    win = torch.from_numpy(CC.window_array(T, H, W, S_h, S_w)).to(dev)
    got = ops.object_crops(torch.from_numpy(np.array(CC.frames(T, H, W))).to(dev), win, size)
    _same(f"{T}x{H}x{W} -> {size}", got, np.asarray(want))
    names = list(CC.named_windows(H, W, S_h, S_w))
    for name in ("invalid_x", "invalid_reversed", "invalid_zeros", "outside_right", "outside_top_left"):
        assert not bool(got[:, names.index(name)].any()), name


def test_nonzero_fill_and_int32_windows(dev):
    from fgvc_amd import ops, viz
    T, H, W, size, fill = 3, 37, 53, (16, 16), (9, 200, 77)
    want = CC.expected_crops(T, H, W, 16, 16, fill, viz.crop_default_taps((H, W), size))
    win = torch.from_numpy(CC.window_array(T, H, W, 16, 16)).to(dev)
    f = torch.from_numpy(np.array(CC.frames(T, H, W))).to(dev)
    _same("fill", ops.object_crops(f, win, size, fill=fill), np.asarray(want))
    _same("fill as an array, int32 windows", ops.object_crops(f, win.to(torch.int32), size, fill=np.array(fill, np.uint8)), np.asarray(want))
    names = list(CC.named_windows(H, W, 16, 16))
    got = ops.object_crops(f, win, size, fill=fill).cpu().numpy()
    assert (got[:, names.index("invalid_x")] == np.array(fill, np.uint8)).all()
    assert (got[:, names.index("outside_right")] == np.array(fill, np.uint8)).all()


@pytest.mark.parametrize("M", (1, 40))
def test_random_windows_one_and_forty_a_frame(dev, M):
    from fgvc_amd import ops, viz
    T, H, W, size = 3, 64, 96, (16, 16)
    f = CC.frames(T, H, W)
    win = CC.random_windows(T, M, H, W, 100 + M)
    fill = np.array([255, 0, 128], np.uint8)
    want = viz.crop_windows_host(f, win, size, fill=fill, max_taps=viz.crop_default_taps((H, W), size))
    _same(f"M={M}", ops.object_crops(torch.from_numpy(np.array(f)).to(dev), torch.from_numpy(win).to(dev), size, fill=fill), want)


def test_max_taps_turns_large_windows_into_fill(dev):
    from fgvc_amd import ops, viz
    H, W, size = 64, 96, (5, 7)
    f = CC.frames(1, H, W)
    win = CC.window_array(1, H, W, 5, 7)
    fill = np.array([1, 2, 3], np.uint8)
    ok = [viz.crop_window_ok(*w, size, 8) for w in win[0].tolist()]
    valid = [viz.crop_window_ok(*w, size) for w in win[0].tolist()]
    assert sum(ok) >= 5 and sum(valid) - sum(ok) >= 5             # both kinds occur: windows within 8 taps, and valid ones beyond
    want = viz.crop_windows_host(f, win, size, fill=fill, max_taps=8)
    got = ops.object_crops(torch.from_numpy(np.array(f)).to(dev), torch.from_numpy(win).to(dev), size, fill=fill, max_taps=8)
    _same("max_taps=8", got, want)
    assert all((want[0, j] == fill).all() for j in range(len(ok)) if not ok[j])
    # the largest table: 256 taps, a 96-pixel window onto one output (194 taps)
    one = np.array([[[0, 0, 96, 64], [-10, -10, 110, 80]]])
    want = viz.crop_windows_host(f, one, (1, 1), fill=fill, max_taps=256)
    _same("256 taps", ops.object_crops(torch.from_numpy(np.array(f)).to(dev), torch.from_numpy(one).to(dev), (1, 1), fill=fill, max_taps=256), want)
    assert not (want[0, 1] == fill).all()


def test_coefficient_table_equals_the_contract_word_for_word(dev):
    """The plan pass's table in the workspace -- per crop: first taps [S_w], tap counts [S_w], first taps [S_h], tap counts [S_h],
    K [S_w][max_taps], K [S_h][max_taps], int32 -- against viz.crop_axis_coefficients.  The bytes of a crop cannot tell a first tap that
    moved by one when the tap it gains or loses weighs nothing; the table can.  x: [5, 10) onto 3 and y: [10, 21) onto 3 are axes where
    the centre of output 2, formed with one rounding instead of two (a contracted multiply-add), moves the first tap."""
    from fgvc_amd import ops, viz
    H, W, taps = 37, 53, 16
    f = torch.from_numpy(np.array(CC.frames(1, H, W))).to(dev)
    for (S_h, S_w), win in (((3, 3), (5, 10, 10, 21)), ((5, 7), (-4, -4, 9, 9)), ((3, 3), (17, 33, 28, 46)), ((16, 16), (2, 1, 87, 17))):
        need = ops.object_crops_workspace_bytes(1, 1, (S_h, S_w), max_taps=taps)
        ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
        ops.object_crops(f, torch.tensor([[list(win)]], device=dev), (S_h, S_w), workspace=ws, max_taps=taps)
        tab = ws.cpu().numpy().view(np.int32)
        xlo, xcnt, ylo, ycnt = tab[:S_w], tab[S_w:2 * S_w], tab[2 * S_w:2 * S_w + S_h], tab[2 * S_w + S_h:2 * (S_w + S_h)]
        K = tab[2 * (S_w + S_h):].reshape(S_w + S_h, taps)
        for (a0, a1, n, lo, cnt, rows) in ((win[0], win[2], S_w, xlo, xcnt, K[:S_w]), (win[1], win[3], S_h, ylo, ycnt, K[S_w:])):
            want_lo, want_K = viz.crop_axis_coefficients(a0, a1, n)
            assert lo.tolist() == want_lo.tolist(), (win, n, lo.tolist(), want_lo.tolist())
            assert cnt.tolist() == [len(k) for k in want_K], (win, n)
            for j in range(n):
                assert rows[j, :cnt[j]].tolist() == want_K[j].tolist(), (win, n, j)


# ---- the window kernel -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CC.window_cases()))
def test_window_kernel_equals_the_hand_computed_windows(dev, name):
    from fgvc_amd import ops
    stats, kw, want = CC.window_cases()[name]
    got = ops.object_windows(torch.from_numpy(stats).to(dev), **kw)
    _same(name, got, want)


def test_window_kernel_on_the_statistics_of_random_maps(dev):
    from fgvc_amd import metrics, ops
    from tests import objects_cases as OC
    for T, h, w, seed in ((5, 37, 53, 1), (3, 64, 96, 2)):
        for ids in (CC.blob_ids(T, h, w, seed), OC.run_map(T, h, w, seed)):
            d = torch.from_numpy(ids).to(dev)
            stats = ops.object_stats(d, 6)
            host = metrics.object_stats_host(ids, 6)
            for kw in (dict(size=(16, 16)), dict(size=(5, 7), pad=0.0, min_side=1, smooth=1), dict(size=(33, 48), pad=1.7, smooth=2),
                       dict(size=(9, 130), pad=4.0, smooth=50, frame_size=(h * 9 // 4, w * 9 // 4)),
                       dict(size=(1, 1), min_side=3, objects=[5, 0, 3, 3])):
                want = metrics.object_windows_host(host, mask_size=(h, w), **kw)
                _same(str(kw), ops.object_windows(stats, mask_size=(h, w), **kw), want)


# ---- the whole chain ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", (1, 2.25))
def test_object_tracks_crops_on_device_statistics_equal_the_host_chain(dev, scale):
    from fgvc_amd import engine, metrics, ops
    T, h, w = 5, 64, 96
    H, W = int(h * scale), int(w * scale)
    ids, f = CC.blob_ids(T, h, w, 7), CC.frames(T, H, W)
    host = engine.ObjectTracks(metrics.object_stats_host(ids, 4)).crops(f, size=(33, 48), smooth=1, masks=True, ids=ids, fill=(5, 6, 7))
    d_ids = torch.from_numpy(ids).to(dev)
    tracks = engine.ObjectTracks(ops.object_stats(d_ids, 4))
    got = tracks.crops(torch.from_numpy(np.array(f)).to(dev), size=(33, 48), smooth=1, masks=True, ids=d_ids, fill=(5, 6, 7))
    assert got.crops.is_cuda and got.masks.is_cuda and got.windows.is_cuda and got.objects == [1, 2, 3] and got.size == (33, 48)
    _same("windows", got.windows, host.windows)
    _same("crops", got.crops, host.crops)
    _same("masks", got.masks, host.masks)
    assert got.valid.tolist() == host.valid.tolist() and not got.valid.all() and got.valid.any()
    assert bool(got.masks.any()) and (host.windows[..., 4:] != host.windows[..., :4]).any() == (scale != 1)
    plain = tracks.crops(torch.from_numpy(np.array(f)).to(dev), size=(33, 48), smooth=1, fill=(5, 6, 7), mask_size=(h, w))
    assert plain.masks is None
    _same("without masks", plain.crops, host.crops)


# ---- memory handling ---------------------------------------------------------------------------------------------------------------------

def test_views_are_read_in_place(dev):
    from fgvc_amd import ops, viz
    T, H, W, size = 3, 37, 53, (16, 16)
    f = CC.frames(T, H, W)
    win = CC.window_array(T, H, W, 16, 16)
    taps = viz.crop_default_taps((H, W), size)
    want = np.asarray(CC.expected_crops(T, H, W, 16, 16, (0, 0, 0), taps))
    d, dw = torch.from_numpy(np.array(f)).to(dev), torch.from_numpy(win).to(dev)
    chw = d.permute(0, 3, 1, 2).contiguous()
    _same("tchw", ops.object_crops(chw, dw, size, layout="tchw"), want)
    _same("thwc view of a tchw tensor", ops.object_crops(chw.permute(0, 2, 3, 1), dw, size), want)
    # a spatial window of a larger tensor, a sentinel colour all around it: a stray read would show against fill = 0
    big = torch.full((T, H + 7, W + 9, 3), 255, dtype=torch.uint8, device=dev)
    big[:, 3:3 + H, 4:4 + W] = d
    view = big[:, 3:3 + H, 4:4 + W]
    assert not view.is_contiguous()
    _same("spatial window", ops.object_crops(view, dw, size), want)
    bigc = torch.full((T, 3, H + 7, W + 9), 255, dtype=torch.uint8, device=dev)
    bigc[:, :, 3:3 + H, 4:4 + W] = chw
    _same("spatial window, tchw", ops.object_crops(bigc[:, :, 3:3 + H, 4:4 + W], dw, size, layout="tchw"), want)
    two = d.repeat_interleave(2, 0)
    two[1::2] = 255
    _same("time slice", ops.object_crops(two[::2], dw, size), want)
    flat = torch.full((T * H * W * 3 + 2,), 255, dtype=torch.uint8, device=dev)
    flat[1:-1] = d.flatten()
    odd = flat[1:-1].view(T, H, W, 3)
    assert odd.data_ptr() % 2 == 1
    _same("odd addresses", ops.object_crops(odd, dw, size), want)
    # ids through their strides, with id 1 all around the window: a clamped or stray sample would read as object 1
    ids = CC.blob_ids(T, H, W, 3)
    objs = [1, 2, 3] + [1] * (win.shape[1] - 3)
    _, wm = viz.crop_windows_host(f, win, size, ids=ids, objects=objs, max_taps=taps)
    big_ids = torch.full((T, H + 5, W + 3), 1, dtype=torch.uint8, device=dev)
    big_ids[:, 2:2 + H, 1:1 + W] = torch.from_numpy(ids).to(dev)
    _, gm = ops.object_crops(d, dw, size, ids=big_ids[:, 2:2 + H, 1:1 + W], objects=objs)
    _same("masks from a window of a larger map", gm, wm)


def test_out_between_guard_bands_a_dirty_workspace_and_a_second_call(dev):
    from fgvc_amd import ops, viz
    T, H, W, size = 3, 37, 53, (33, 48)
    f, ids = CC.frames(T, H, W), CC.blob_ids(T, H, W, 3)
    win = CC.window_array(T, H, W, 33, 48)
    M = win.shape[1]
    objs = [(j % 3) + 1 for j in range(M)]
    taps = viz.crop_default_taps((H, W), size)
    want, wm = viz.crop_windows_host(f, win, size, ids=ids, objects=objs, max_taps=taps)
    d, dw, di = torch.from_numpy(np.array(f)).to(dev), torch.from_numpy(win).to(dev), torch.from_numpy(ids).to(dev)
    n, nm, g = want.size, wm.size, 256
    buf = torch.full((n + 2 * g,), 0xA5, dtype=torch.uint8, device=dev)
    mbuf = torch.full((nm + 2 * g,), 0x5A, dtype=torch.uint8, device=dev)
    out, mout = buf[g:-g].view(want.shape), mbuf[g:-g].view(wm.shape)
    need = ops.object_crops_workspace_bytes(T, M, size, (H, W))
    assert need == 4 * T * M * (33 + 48) * (2 + taps) and ops.object_crops_workspace_bytes(T, M, size, max_taps=taps) == need
    ws = torch.full((need + 64,), 0xFF, dtype=torch.uint8, device=dev)
    c, m = ops.object_crops(d, dw, size, ids=di, objects=objs, out=out, mask_out=mout, workspace=ws[:need])
    assert c is out and m is mout
    _same("crops", out, want)
    _same("masks", mout, wm)
    hb, hm, hw = buf.cpu(), mbuf.cpu(), ws.cpu()
    assert bool((hb[:g] == 0xA5).all()) and bool((hb[-g:] == 0xA5).all())
    assert bool((hm[:g] == 0x5A).all()) and bool((hm[-g:] == 0x5A).all())
    assert bool((hw[need:] == 0xFF).all())
    # the same buffers again with other windows (valid ones become invalid and the reverse): nothing of the first call is left
    win2 = np.ascontiguousarray(win[:, ::-1]) + np.array([1, 2, 1, 2])
    want2, wm2 = viz.crop_windows_host(f, win2, size, ids=ids, objects=objs, max_taps=taps)
    ops.object_crops(d, torch.from_numpy(win2).to(dev), size, ids=di, objects=objs, out=out, mask_out=mout, workspace=ws[:need])
    _same("second call, crops", out, want2)
    _same("second call, masks", mout, wm2)
    assert not np.array_equal(want, want2)


def test_refusals_are_by_name_before_any_launch(dev):
    from fgvc_amd import _lib, ops
    f = torch.zeros((2, 8, 9, 3), dtype=torch.uint8, device=dev)
    win = torch.zeros((2, 1, 4), dtype=torch.int64, device=dev)
    ids = torch.zeros((2, 8, 9), dtype=torch.uint8, device=dev)
    for kw, exc, name in ((dict(size=(0, 4)), ValueError, "size"), (dict(size=(4, 1025)), ValueError, "size"),
                          (dict(layout="hwc"), ValueError, "layout"), (dict(fill=(1, 2)), ValueError, "fill"),
                          (dict(fill=(1, 2, 256)), ValueError, "fill"), (dict(max_taps=257), ValueError, "max_taps"),
                          (dict(max_taps=3), ValueError, "max_taps"), (dict(ids=ids), ValueError, "ids and objects"),
                          (dict(ids=ids, objects=[1, 2]), ValueError, "objects"), (dict(ids=ids, objects=[256]), ValueError, "objects"),
                          (dict(mask_out=ids), ValueError, "mask_out"), (dict(out=torch.zeros((2, 1, 4, 4, 3), device=dev)), ValueError, "out"),
                          (dict(workspace=torch.zeros(8, dtype=torch.uint8, device=dev)), ValueError, "workspace")):
        args = dict(size=(4, 4))
        args.update(kw)
        with pytest.raises(exc, match=name):
            ops.object_crops(f, win, **args)
    with pytest.raises(ValueError, match="windows"):
        ops.object_crops(f, win[:1], (4, 4))
    with pytest.raises(TypeError, match="windows"):
        ops.object_crops(f, win.float(), (4, 4))
    with pytest.raises(TypeError, match="frames_u8"):
        ops.object_crops(f.float(), win, (4, 4))
    with pytest.raises(_lib.FgvcHipError, match="frames_u8"):
        ops.object_crops(f.cpu(), win, (4, 4))
    stats = torch.zeros((2, 3, 8), dtype=torch.int64, device=dev)
    for kw, name in ((dict(size=(4, 2000)), "size"), (dict(pad=5.0), "pad"), (dict(objects=[3]), "objects"), (dict(mask_size=(40000, 9)), "mask_size h"),
                     (dict(frame_size=(8, 32769)), "frame_size W"), (dict(min_side=0), "min_side"), (dict(smooth=-2), "smooth")):
        args = dict(size=(4, 4), mask_size=(8, 9))
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            ops.object_windows(stats, **args)
    with pytest.raises(_lib.FgvcHipError, match="stats"):
        ops.object_windows(stats.cpu(), (4, 4), mask_size=(8, 9))
    lib = _lib.load()
    assert lib.fgvc_frames_object_crops_u8(None, 1, 8, 9, 0, 0, 0, 0, None, 5, 1, 4, 4, 0, 0, 0, None, 0, 0, 0, 0, None, 16, None, None, None, 0,
                                           None) == 1 and b"window_words" in lib.fgvc_last_error()
    assert lib.fgvc_frames_object_crops_u8(None, 1, 8, 40000, 0, 0, 0, 0, None, 4, 1, 4, 4, 0, 0, 0, None, 0, 0, 0, 0, None, 16, None, None, None,
                                           0, None) == 1 and b"H, W" in lib.fgvc_last_error()
    assert lib.fgvc_seg_object_windows_i64(None, 1, 2, None, 1, 4, 4, 5000, 8, 0, 8, 9, 8, 9, None, None) == 1 and b"pad_q" in lib.fgvc_last_error()
    # empty clips and empty object lists launch nothing
    assert tuple(ops.object_crops(f[:0], win[:0], (4, 4)).shape) == (0, 1, 4, 4, 3)
    assert tuple(ops.object_crops(f, win[:, :0], (4, 4)).shape) == (2, 0, 4, 4, 3)
    assert tuple(ops.object_windows(stats, (4, 4), mask_size=(8, 9), objects=[]).shape) == (2, 0, 8)
