"""CPU tests of objects as boxes: metrics.object_stats_host on hand-built maps whose words are written out here,
engine.ObjectTracks, metrics.box_iou, the MOT text round trip, parse_objects, the host box painter against pixel sets built with numpy
slices, the digit table, the C surface of the two new entries and their code-object notes."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from fgvc_amd import viz
from tests import objects_cases as OC
from tests import render_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"fgvc_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the contract on maps whose answer is written out --------------------------------------------------------------------------------------
def test_contract_on_hand_built_maps():
    from fgvc_amd import metrics
    m = np.zeros((2, 5, 7), np.uint8)
    m[0, 0, 0], m[0, 0, 6], m[0, 4, 0], m[0, 4, 6] = 1, 2, 3, 4            # one pixel in each corner
    # an L: a column of four pixels at x = 2 (y = 0 .. 3) and a foot of three more on y = 3 (x = 3 .. 5)
    m[1, 0:4, 2] = 5
    m[1, 3, 3:6] = 5
    got = metrics.object_stats_host(m, 7)
    assert got.dtype == np.int64 and got.shape == (2, 7, 8)
    #                    area x0 y0 x1 y1 sum_x sum_y border
    assert got[0].tolist() == [[31, 0, 0, 7, 5, 93, 62, 16],               # the background: 35 - 4 pixels, 20 border pixels - 4
                               [1, 0, 0, 1, 1, 0, 0, 1],
                               [1, 6, 0, 7, 1, 6, 0, 1],
                               [1, 0, 4, 1, 5, 0, 4, 1],
                               [1, 6, 4, 7, 5, 6, 4, 1],
                               [0] * 8, [0] * 8]
    assert got[1, 5].tolist() == [7, 2, 0, 6, 4, 2 * 4 + 3 + 4 + 5, 0 + 1 + 2 + 3 + 3 * 3, 1]      # only (2, 0) is on the border
    assert got[1, 0].tolist() == [28, 0, 0, 7, 5, 105 - 20, 70 - 15, 19]
    assert not got[1, 1:5].any() and not got[1, 6].any()
    # ids of n_ids or more are counted nowhere; a one-pixel frame is all border
    assert metrics.object_stats_host(m, 2)[0].tolist() == got[0, :2].tolist()
    assert metrics.object_stats_host(np.full((1, 1, 1), 3, np.uint8), 4)[0, 3].tolist() == [1, 0, 0, 1, 1, 0, 0, 1]
    assert metrics.object_stats_host(np.full((1, 3, 1), 1, np.uint8), 2)[0, 1].tolist() == [3, 0, 0, 1, 3, 0, 3, 3]
    with pytest.raises(ValueError, match="n_ids"):
        metrics.object_stats_host(m, 0)
    with pytest.raises(ValueError, match="ids"):
        metrics.object_stats_host(m[0], 2)


def test_shared_cases_have_what_they_name():
    c = OC.cases()
    assert len(np.unique(c["all_256_ids_2x16x257"][0][0])) == 256 and len(np.unique(c["all_256_ids_2x16x257"][0][1])) == 256
    m, n = c["ids_beyond_n_ids_2x9x63"]
    assert int(m.max()) >= n
    m, _ = c["checkerboard_3x9x65"]
    assert bool((m[:, :, 1:] != m[:, :, :-1]).all()) and bool((m[:, 1:] != m[:, :-1]).all())
    m, _ = c["object_across_every_band_2x64x40"]
    rows = np.flatnonzero((m[0] == 1).any(1))
    per = -(-64 // OC.WAVES)
    assert all(b - 1 in rows and b in rows for b in range(per, 64, per))              # both sides of every boundary between two bands
    assert int(OC.expected("row_sums_beyond_2p32_2x70000")[0, 1, 5]) > 2 ** 32
    assert int(OC.expected("one_row_sum_beyond_2p32_1x100000")[0, 1, 5]) > 2 ** 32


def test_both_clip_lengths_occur_for_every_width_and_height():
    """the size sweep of test_gpu_objects.py runs T = 1 and T = 3 at every width and at every height"""
    for w in OC.WIDTHS:
        assert {OC.sized(w, h).shape[0] for h in OC.HEIGHTS} == {1, 3}
    for h in OC.HEIGHTS:
        assert {OC.sized(w, h).shape[0] for w in OC.WIDTHS} == {1, 3}


# ---- ObjectTracks, box_iou, MOT ----------------------------------------------------------------------------------------------------------------
def _two_frames():
    from fgvc_amd import engine, metrics
    m = np.zeros((2, 6, 8), np.uint8)
    m[0, 1:3, 2:6] = 1                                                      # 2 x 4 pixels: centroid (3.5, 1.5)
    m[1, 2:5, 1:3] = 2
    return engine.ObjectTracks(metrics.object_stats_host(m, 3))


def test_object_tracks_present_and_absent():
    from fgvc_amd import engine
    tr = _two_frames()
    assert tr.area.tolist() == [[40, 8, 0], [42, 0, 6]] and tr.area.dtype == np.int64
    assert tr.present.dtype == np.bool_ and tr.present.tolist() == [[True, True, False], [True, False, True]]
    assert tr.boxes.shape == (2, 3, 4) and tr.boxes.dtype == np.int64
    assert tr.boxes[0, 1].tolist() == [2, 1, 6, 3] and tr.boxes[1, 2].tolist() == [1, 2, 3, 5]
    assert tr.boxes[0, 2].tolist() == [0, 0, 0, 0] and tr.boxes[1, 1].tolist() == [0, 0, 0, 0]       # absent: an empty box
    assert tr.centroids.dtype == np.float64 and tr.centroids[0, 1].tolist() == [3.5, 1.5] and tr.centroids[1, 2].tolist() == [1.5, 3.0]
    assert np.isnan(tr.centroids[0, 2]).all() and np.isnan(tr.centroids[1, 1]).all()
    assert tr.border.tolist() == [[24, 0, 0], [24, 0, 0]]
    tracks, vis = tr.centroid_tracks()
    assert tracks.shape == (3, 2, 2) and tracks.dtype == np.float64 and vis.shape == (3, 2) and vis.dtype == np.bool_
    assert vis.tolist() == [[True, True], [True, False], [False, True]] and np.isfinite(tracks).all()
    assert tracks[1, 0].tolist() == [3.0, 1.0]                             # centroid - 0.5: the painters draw a coordinate c at c + 0.5
    # ... so a one-pixel object gets its dot centred on that pixel
    one = np.zeros((1, 16, 16), np.uint8)
    one[0, 8, 6] = 1
    from fgvc_amd import metrics
    t1, v1 = engine.ObjectTracks(metrics.object_stats_host(one, 2)).centroid_tracks()
    dot = viz.paint_point_track(np.zeros((1, 16, 16, 3), np.uint8), t1[1:], v1[1:], colors=np.array([[255, 255, 255]]), radius=3)[0, :, :, 0]
    ys, xs = np.nonzero(dot == dot.max())
    assert dot[8, 6] == 255 and ys.mean() == 8 and xs.mean() == 6
    assert tr.area.base is tr.boxes.base and not tr.area.flags.writeable            # one host copy behind every property
    # a tensor works as well as an array; a wrong shape is refused
    assert engine.ObjectTracks(torch.from_numpy(tr.stats)).area.tolist() == tr.area.tolist()
    with pytest.raises(ValueError, match="stats"):
        engine.ObjectTracks(np.zeros((2, 3, 7), np.int64)).area


def test_box_iou_corner_cases():
    from fgvc_amd import metrics
    iou = metrics.box_iou
    assert iou([0, 0, 2, 2], [1, 1, 3, 3]) == 1 / 7 and iou([0, 0, 4, 4], [0, 0, 4, 4]) == 1.0 and iou([0, 0, 2, 2], [2, 0, 4, 2]) == 0.0
    assert iou([0, 0, 4, 4], [1, 1, 2, 2]) == 1 / 16
    assert iou([0, 0, 0, 0], [1, 1, 3, 3]) == 0.0 and iou([1, 1, 3, 3], [5, 5, 5, 9]) == 0.0          # an empty box against anything
    assert iou([2, 2, 1, 5], [0, 0, 9, 9]) == 0.0                                                    # x1 < x0 is empty too, not negative
    assert np.isnan(iou([0, 0, 0, 0], [3, 3, 3, 3])) and np.isnan(iou([0, 0, 0, 5], [0, 0, 0, 0]))  # two empty boxes
    a = np.array([[[0, 0, 2, 2], [0, 0, 0, 0]]])
    got = iou(a, np.array([0, 0, 2, 2]))
    assert got.dtype == np.float64 and got.shape == (1, 2) and got.tolist() == [[1.0, 0.0]]
    with pytest.raises(ValueError, match="boxes"):
        iou([0, 0, 1], [0, 0, 1, 1])


def test_mot_round_trip(tmp_path):
    from fgvc_amd import datasets
    tr = _two_frames()
    path = tmp_path / "out.txt"
    assert datasets.write_mot(path, tr) == 2
    lines = open(path).read().splitlines()
    assert lines[0] == "1,1,2,1,4,2,1,-1,-1,-1" and lines[1] == "2,2,1,2,2,3,1,-1,-1,-1"          # the background (row 0) is not written
    back = datasets.read_mot(path)
    assert back == {1: {0: (2, 1, 6, 3)}, 2: {1: (1, 2, 3, 5)}}
    for o, frames in back.items():
        for t, box in frames.items():
            assert tr.present[t, o] and tr.boxes[t, o].tolist() == list(box)
    assert datasets.write_mot(path, tr, ids=[0, 17, 5]) == 2 and set(datasets.read_mot(path)) == {17, 5}
    with pytest.raises(ValueError, match="ids"):
        datasets.write_mot(path, tr, ids=[1, 2])


def test_parse_objects():
    from fgvc_amd import engine
    assert engine.parse_objects(None) is False and engine.parse_objects(dict(stats=True)) is True
    assert engine.parse_objects(dict(stats=False)) is False and engine.parse_objects({}) is True
    with pytest.raises(ValueError, match="boxes"):
        engine.parse_objects(dict(stats=True, boxes=True))
    with pytest.raises(ValueError, match="test_cfg.objects.stats"):
        engine.parse_objects(dict(stats=1))
    with pytest.raises(ValueError, match="test_cfg.objects"):
        engine.parse_objects(True)


# ---- the host box painter ------------------------------------------------------------------------------------------------------------------------
H, W = 24, 40


def _frame(seed=1):
    return np.random.default_rng(seed).integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)


def _blend(img, mask, col, alpha):
    """the overlay's formula on the pixels of mask (H, W) bool"""
    mixed = ((img.astype(np.int64) * (256 - alpha) + np.array(col, np.int64) * alpha + 128) >> 8).astype(np.uint8)
    return np.where(mask[..., None], mixed, img)


def _rect(x0, y0, x1, y1):
    m = np.zeros((H, W), bool)
    m[max(y0, 0):max(y1, 0), max(x0, 0):max(x1, 0)] = True
    return m


def _ring(box, bw):
    x0, y0, x1, y1 = box
    return _rect(x0 - bw, y0 - bw, x1 + bw, y1 + bw) & ~_rect(x0, y0, x1, y1)


def _glyphs(img, text, tx, ty, ink):
    """the digits of `text` written into img (H, W, 3) at scale 1, from the table's bits"""
    out = img.copy()
    for g, ch in enumerate(text):
        bits = np.unpackbits(np.array(viz.DIGITS_5X7[int(ch)])[:, None], axis=1)[:, 3:].astype(bool)      # (7, 5)
        region = out[ty + 1:ty + 8, tx + 1 + 6 * g:tx + 6 + 6 * g]
        region[bits] = ink
    return out


def test_ring_only():
    f = _frame()
    col = (200, 30, 90)
    got = viz.render(f, boxes=[[[10, 8, 20, 14]]], box_colors=[col], box_width=2)
    ring = _ring((10, 8, 20, 14), 2)
    assert ring.sum() == 14 * 10 - 10 * 6
    assert np.array_equal(got[0], _blend(f[0], ring, col, 255))
    assert np.array_equal(got[0][8:14, 10:20], f[0][8:14, 10:20])                                   # the object stays uncovered
    assert np.array_equal(viz.paint_boxes(f, [[[10, 8, 20, 14]]], box_colors=[col]), got)


def test_tag_moves_inside_at_the_top_edge():
    f = _frame(2)
    col, box, bw = (250, 240, 60), (10, 3, 30, 20), 2                                              # a light colour: black digits
    got = viz.render(f, boxes=[[box]], box_colors=[col], box_width=bw, box_labels=[5])
    # 3 - 2 - 9 < 0: the tag's rows are [3, 12), its columns [8, 15); its first two columns lie on the ring and are blended twice
    want = _blend(f[0], _ring(box, bw), col, 255)
    want = _blend(want, _rect(8, 3, 15, 12), col, 255)
    want = _glyphs(want, "5", 8, 3, 0)
    assert np.array_equal(got[0], want)
    assert (got[0][4:11, 9:14] == 0).all(-1).sum() == bin(int.from_bytes(bytes(viz.DIGITS_5X7[5].tolist()), "big")).count("1")
    # one row lower and the tag fits above the ring: rows [0, 9)
    got = viz.render(f, boxes=[[(10, 11, 30, 20)]], box_colors=[col], box_width=bw, box_labels=[5])
    want = _glyphs(_blend(_blend(f[0], _ring((10, 11, 30, 20), bw), col, 255), _rect(8, 0, 15, 9), col, 255), "5", 8, 0, 0)
    assert np.array_equal(got[0], want)


def test_tag_shifts_left_at_the_right_edge():
    f = _frame(3)
    col, box, bw = (10, 20, 120), (30, 14, 38, 20), 1                                              # a dark colour: white digits
    got = viz.render(f, boxes=[[box]], box_colors=[col], box_width=bw, box_labels=[123])
    # three digits: 19 columns; 29 + 19 > 40, so the tag starts at 40 - 19 = 21, rows [14 - 1 - 9, 13) = [4, 13)
    want = _blend(f[0], _ring(box, bw), col, 255)
    want = _glyphs(_blend(want, _rect(21, 4, 40, 13), col, 255), "123", 21, 4, 255)
    assert np.array_equal(got[0], want)
    # a frame narrower than the tag: it starts at column 0 and is clipped
    narrow = np.ascontiguousarray(f[:, :, :12])
    got = viz.render(narrow, boxes=[[(4, 14, 9, 20)]], box_colors=[col], box_width=bw, box_labels=[123])
    wide = np.zeros((1, H, W, 3), np.uint8)
    wide[:, :, :12] = narrow
    want = _glyphs(_blend(wide[0], _rect(0, 4, 19, 13), col, 255), "123", 0, 4, 255)[:, :12]
    ring = _ring((4, 14, 9, 20), bw)[:, :12]
    assert np.array_equal(got[0], np.where(ring[..., None], _blend(narrow[0], ring, col, 255), want))


def test_two_overlapping_boxes_in_index_order_and_alpha_128():
    f = _frame(4)
    cols = [(255, 0, 0), (0, 0, 255)]
    boxes = [(8, 6, 22, 16), (14, 10, 30, 20)]
    got = viz.render(f, boxes=[boxes], box_colors=cols, box_width=2, box_alpha=128)
    want = _blend(_blend(f[0], _ring(boxes[0], 2), cols[0], 128), _ring(boxes[1], 2), cols[1], 128)
    assert np.array_equal(got[0], want)
    both = _ring(boxes[0], 2) & _ring(boxes[1], 2)
    assert both.any()                                                                              # pixels blended twice, first box first
    swapped = viz.render(f, boxes=[boxes[::-1]], box_colors=cols[::-1], box_width=2, box_alpha=128)
    assert not np.array_equal(swapped[0][both], got[0][both])
    # the formula itself, at one ring pixel
    y, x = 4, 8
    assert got[0, y, x].tolist() == [(int(f[0, y, x, c]) * 128 + cols[0][c] * 128 + 128) >> 8 for c in range(3)]
    # invisible and empty boxes draw nothing; box_colors=None takes palette[i]
    assert np.array_equal(viz.render(f, boxes=[boxes], box_visibles=[[False, False]]), f)
    assert np.array_equal(viz.render(f, boxes=[[(5, 5, 5, 9), (9, 9, 12, 9), (7, 3, 2, 8)]]), f)
    pal = viz.davis_palette()
    assert np.array_equal(viz.render(f, boxes=[boxes]), viz.render(f, boxes=[boxes], box_colors=pal[:2]))
    # scale: every bitmap pixel is an s x s block
    one = viz.render(np.zeros((1, 40, 60, 3), np.uint8), boxes=[[(2, 12, 30, 30)]], box_colors=[(0, 0, 0)], box_labels=[8], box_alpha=256)
    three = viz.render(np.zeros((1, 120, 180, 3), np.uint8), boxes=[[(6, 36, 90, 90)]], box_colors=[(0, 0, 0)], box_labels=[8], box_alpha=256,
                       label_scale=3, box_width=6)
    assert one.any() and np.array_equal(three, one.repeat(3, 1).repeat(3, 2))


def test_digit_table():
    d = viz.DIGITS_5X7
    assert d.shape == (10, 7) and d.dtype == np.uint8 and not d.flags.writeable
    assert int(d.max()) < 32 and all(int(g.max()) > 0 and int(np.count_nonzero(g)) == 7 for g in d)      # 5 bits a row, no empty glyph or row
    assert len({bytes(g.tolist()) for g in d}) == 10


@pytest.mark.parametrize("name", list(RC.cases()))
def test_no_boxes_is_todays_render(name):
    c = RC.cases()[name]
    got = viz.render(boxes=None, box_visibles=None, box_colors=None, box_width=2, box_alpha=255, box_labels=None, label_scale=1, **c)
    assert np.array_equal(got, RC.expected(name))


def test_painter_refusals_by_name():
    f = _frame()
    b = [[(1, 1, 5, 5)]]
    tr = np.zeros((1, 1, 2))
    for kw, word in ((dict(tracks=tr, trail=2), "trail"), (dict(tracks=tr, skeleton=[[0, 0]]), "skeleton"),
                     (dict(heat=np.zeros((1, 1, H, W), np.float32)), "heat")):
        with pytest.raises(ValueError, match=f"boxes: not together with {word}="):
            viz.render(f, boxes=b, **kw)
    for kw, word in ((dict(boxes=np.zeros((1, 256, 4), np.int64)), "boxes: N=256"), (dict(boxes=[[(0, 0, 2 ** 20, 4)]]), "boxes: coordinates"),
                     (dict(boxes=[[(0, -2 ** 20, 3, 4)]]), "boxes: coordinates"), (dict(boxes=[[(0.5, 0, 3, 4)]]), "boxes"),
                     (dict(boxes=[(0, 0, 3, 4)]), "boxes"), (dict(boxes=b, box_width=0), "box_width"), (dict(boxes=b, box_width=17), "box_width"),
                     (dict(boxes=b, box_width=2.0), "box_width"), (dict(boxes=b, box_alpha=257), "box_alpha"),
                     (dict(boxes=b, box_labels=[1000]), "box_labels"), (dict(boxes=b, box_labels=[-1]), "box_labels"),
                     (dict(boxes=b, box_labels=[1, 2]), "box_labels"), (dict(boxes=b, box_labels=[1], label_scale=5), "label_scale"),
                     (dict(boxes=b, box_colors=[(1, 2, 300)]), "box_colors"), (dict(boxes=b, box_colors=[(1, 2, 3)] * 2), "box_colors"),
                     (dict(boxes=b, box_visibles=[[1]]), "box_visibles"), (dict(boxes=b, box_visibles=[[True, True]]), "box_visibles")):
        with pytest.raises((ValueError, TypeError), match=word):
            viz.render(f, **kw)
    with pytest.raises(ValueError, match="boxes"):
        viz.paint_boxes(f, None)


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_exported_and_validate():
    import re
    from fgvc_amd import _lib, build
    assert "objects.hip" in build.SOURCES and "boxes.hip" in build.SOURCES
    with open(os.path.join(ROOT, "include", "fgvc_hip.h")) as f:
        text = f.read()
    lib = _lib.load()
    for name in ("fgvc_seg_object_stats_u8", "fgvc_render_boxes_u8"):
        decl = re.search(r"int " + name + r"\(([^;]*)\);", text)
        assert decl and name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name               # one ctypes argument per declared parameter
    ids, out = C.create_string_buffer(64), C.create_string_buffer(4 * 8 * 8)                       # never reached
    pi, po = C.cast(ids, C.c_void_p), C.cast(out, C.c_void_p)

    def stats(ids=pi, st=16, sy=4, T=1, h=4, w=4, n=2, out=po):
        return lib.fgvc_seg_object_stats_u8(ids, st, sy, T, h, w, n, out, None)
    for kw, word in ((dict(ids=None), b"ids"), (dict(out=None), b"stats"), (dict(n=0), b"n_ids"), (dict(n=257), b"n_ids"), (dict(T=0), b"T="),
                     (dict(T=-1), b"T="), (dict(h=0), b"h="), (dict(w=0), b"w="), (dict(w=-3), b"w="), (dict(sy=3), b"ids_stride_y"),
                     (dict(T=2, st=-16), b"ids_stride_y"), (dict(h=1 << 21, w=1 << 21, sy=1 << 21), b"2^62"),
                     (dict(h=1 << 30, w=1 << 2, sy=4), b"2^62")):
        assert stats(**kw) == _lib.ERR_INVALID_ARG and lib.fgvc_last_error().startswith(b"fgvc_seg_object_stats_u8: ") \
            and word in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())

    fr = C.create_string_buffer(4 * 4 * 3)
    pf = C.cast(fr, C.c_void_p)

    def boxes(N=1, bw=2, ba=255, scale=1, bx=po, colors=pi, labels=None, digits=None, b_st=4, T=1):
        head = [pf, 48, 12, pf, 48, 12, T, 4, 4, None, 0, 0, None, 128, 0, None, 0, 0, None, 0, 0, None, 0, 0, None]
        return lib.fgvc_render_boxes_u8(*head, bx, b_st, None, 0, colors, N, bw, ba, labels, scale, digits, None)
    for kw, word in ((dict(N=256), b"N=256"), (dict(N=-1), b"N=-1"), (dict(bw=0), b"box_width"), (dict(bw=17), b"box_width"),
                     (dict(ba=257), b"box_alpha"), (dict(ba=-1), b"box_alpha"), (dict(scale=0), b"label_scale"), (dict(scale=5), b"label_scale"),
                     (dict(bx=None), b"boxes"), (dict(colors=None), b"box_colors"), (dict(labels=po), b"digits"),
                     (dict(T=2, b_st=-4), b"frame stride")):
        assert boxes(**kw) == _lib.ERR_INVALID_ARG and lib.fgvc_last_error().startswith(b"fgvc_render_boxes_u8: ") \
            and word in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())


def test_wrapper_refusals_without_a_gpu():
    from fgvc_amd import _lib, ops
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.object_stats(torch.zeros(1, 4, 4, dtype=torch.uint8), 2)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.render_boxes(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), torch.zeros(1, 1, 4, dtype=torch.int64))


def test_kernels_use_no_scratch():
    """The code-object notes of the built library.  fgvc_seg_object_stats_u8: no scratch memory and no spilled register, vector or scalar; its
    table is 256 ids x 8 words x 8 bytes of LDS; 1024 threads a workgroup leave at most 128 VGPRs.  fgvc_render_boxes_u8: no scratch and no
    spilled register, vector or scalar, either; the LDS of the plain renderer plus the stage's 14 words per box record; no more VGPRs than
    the trail kernel's 80."""
    notes = _tool("kernel_notes").kernel_notes()
    stats = {k: v for k, v in notes.items() if "object_stats_kernel" in k}
    boxes = {k: v for k, v in notes.items() if "render_boxes_kernel" in k}
    plain = {k: v for k, v in notes.items() if "render_frames_kernel" in k}
    assert len(stats) == 1 and len(boxes) == 1 and len(plain) == 1, (sorted(stats), sorted(boxes), sorted(plain))
    for k, v in stats.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == 256 * 8 * 8 and v["vgpr_count"] <= 128, (k, v)
    lds = next(iter(plain.values()))["group_segment_fixed_size"]
    for k, v in boxes.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0, (k, v)
        assert v["group_segment_fixed_size"] == lds + 14 * 256 * 4 and v["vgpr_count"] <= 80, (k, v)     # + the records of up to 255 boxes
