"""Shared by test_objects_host.py, test_gpu_objects.py and test_gpu_boxes.py: the id maps the object statistics kernel
(fgvc_seg_object_stats_u8) is held to, with their expected words from metrics.object_stats_host computed once, and the
box-painting cases of viz.render(boxes=...).  Everything here runs on the CPU."""
import functools

import numpy as np

WIDTHS = (1, 15, 16, 17, 63, 64, 65, 257, 1025)
HEIGHTS = (1, 2, 9, 33)
N_IDS = (1, 2, 4, 256)
WAVES = 16              # waves of the kernel's one workgroup per frame: each takes a contiguous band of ceil(items / 16) row segments
SEGMENT = 1024          # pixels of one item (a row segment: 64 lanes x 16 pixels)


def run_map(T, h, w, seed, ids=(0, 0, 0, 1, 2, 3, 5, 255), max_run=40):
    """(T, h, w) uint8 of runs of random length 1 .. max_run in row-major order (runs wrap over row ends, so rows begin mid-run)."""
    rng = np.random.default_rng(seed)
    n = T * h * w
    lens = rng.integers(1, max_run + 1, size=n)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), n)) + 1]
    vals = rng.choice(np.array(ids, np.uint8), size=lens.size)
    return np.repeat(vals, lens)[:n].reshape(T, h, w)


@functools.lru_cache(maxsize=None)
def sized(w, h):
    """The map of the size sweep: T = 1 for an even position in the sweep, 3 for an odd one (both occur for every width and height)."""
    T = 1 if (WIDTHS.index(w) + HEIGHTS.index(h)) % 2 == 0 else 3
    m = run_map(T, h, w, 1000 * h + w, max_run=max(2, min(40, w)))
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (ids (T, h, w) uint8, n_ids)."""
    c = {}
    c["all_zero_2x33x65"] = (np.zeros((2, 33, 65), np.uint8), 4)
    c["one_object_fills_2x33x65"] = (np.full((2, 33, 65), 1, np.uint8), 2)
    yy, xx = np.mgrid[0:9, 0:65]
    c["checkerboard_3x9x65"] = (np.broadcast_to((1 + (yy + xx) % 2).astype(np.uint8), (3, 9, 65)).copy(), 3)
    every = (np.arange(2 * 16 * 257).reshape(2, 16, 257) * 7 % 256).astype(np.uint8)      # 7 is odd: every id occurs on every frame
    c["all_256_ids_2x16x257"] = (every, 256)
    c["ids_beyond_n_ids_2x9x63"] = (run_map(2, 9, 63, 5, ids=(0, 1, 2, 3, 4, 5, 6, 7, 200)), 4)
    mid = np.zeros((3, 17, 33), np.uint8)
    mid[1, 4:9, 20:31] = 3
    c["middle_frame_only_3x17x33"] = (mid, 4)
    # the waves' bands: 64 rows of one segment -> 4 rows a wave; rows 2 .. 61 of the object cross every boundary between two bands
    stripe = np.zeros((2, 64, 40), np.uint8)
    stripe[:, 2:62, 7:29] = 1
    stripe[1, 30:34, 0:40] = 2
    c["object_across_every_band_2x64x40"] = (stripe, 3)
    # three segments a row, 9 rows: 27 items, 2 a wave (segment-major), and an object across both segment boundaries
    wide = np.zeros((1, 9, 2100), np.uint8)
    wide[0, :, 1000:1100] = 1
    wide[0, 3:6, 2040:2060] = 2
    wide[0, 4, 1020:1030] = 0
    c["object_across_segments_1x9x2100"] = (wide, 3)
    c["row_sums_beyond_2p32_2x70000"] = (np.full((1, 2, 70000), 1, np.uint8), 2)
    c["one_row_sum_beyond_2p32_1x100000"] = (np.full((1, 1, 100000), 1, np.uint8), 2)
    for m, _ in c.values():
        m.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name):
    from fgvc_amd import metrics
    m, n = cases()[name]
    want = metrics.object_stats_host(m, n)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def expected_sized(w, h):
    """metrics.object_stats_host of sized(w, h) at n_ids = 256; the first n rows are the answer for n_ids = n."""
    from fgvc_amd import metrics
    want = metrics.object_stats_host(sized(w, h), 256)
    want.setflags(write=False)
    return want


# ---- viz.render(boxes=...) -------------------------------------------------------------------------------------------------------------------
BOX_T, BOX_H, BOX_W = 3, 37, 300        # fgvc_render_tile() = (8, 256): two column tiles, five row bands, neither a multiple


def box_frames(T=BOX_T, H=BOX_H, W=BOX_W, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(T, H, W, 3), dtype=np.uint8)


def _per_frame(boxes, T=BOX_T):
    """one list of boxes -> (T, N, 4), moved by (3 t, t) on frame t so that the frames differ"""
    b = np.array(boxes, np.int64).reshape(-1, 4)
    return np.stack([b + np.array([3 * t, t, 3 * t, t]) for t in range(T)])


@functools.lru_cache(maxsize=None)
def box_cases():
    """name -> the keyword arguments of viz.render (frames included)."""
    rng = np.random.default_rng(17)
    f = box_frames()
    ids = np.zeros((BOX_T, BOX_H, BOX_W), np.uint8)
    ids[:, 5:20, 240:270] = 1
    ids[:, 18:30, 20:60] = 2
    tracks = np.array([[[255.5, 7.5]] * BOX_T, [[30.0, 20.0]] * BOX_T, [[299.0, 36.0]] * BOX_T])
    c = {}
    c["across_the_tile_edges"] = dict(frames=f, boxes=_per_frame([[250, 4, 262, 12], [256, 8, 270, 20], [200, 7, 256, 8], [254, 15, 258, 17]]),
                                      box_labels=[1, 2, 3, 4])
    c["partly_and_wholly_outside"] = dict(frames=f, boxes=_per_frame([[-10, -5, 20, 10], [290, 30, 320, 50], [-50, -50, -20, -20],
                                                                      [400, 10, 420, 20], [-5, -5, 305, 42], [-3, 20, 4, 30], [100, -9, 120, -2]]),
                                          box_labels=[10, 11, 12, 13, 14, 15, 16], box_width=3)
    vis = np.ones((BOX_T, 4), bool)
    vis[:, 2] = False
    vis[1, 3] = False
    c["empty_and_invisible"] = dict(frames=f, boxes=_per_frame([[10, 10, 10, 20], [40, 10, 60, 5], [80, 10, 100, 20], [120, 10, 140, 20]]),
                                    box_visibles=vis, box_labels=[1, 2, 3, 4])
    for bw in (1, 2, 16):
        c[f"box_width_{bw}"] = dict(frames=f, boxes=_per_frame([[60, 17, 90, 25], [250, 10, 258, 30]]), box_width=bw, box_alpha=200 + bw)
    c["no_box"] = dict(frames=f, boxes=np.zeros((BOX_T, 0, 4), np.int64), box_labels=[])
    c["one_box"] = dict(frames=f, boxes=_per_frame([[100, 12, 180, 30]]), box_colors=np.array([[250, 250, 40]]), box_labels=[0])
    many = np.zeros((BOX_T, 255, 4), np.int64)
    many[..., 0] = rng.integers(-20, BOX_W, size=(BOX_T, 255))
    many[..., 1] = rng.integers(-10, BOX_H, size=(BOX_T, 255))
    many[..., 2] = many[..., 0] + rng.integers(0, 40, size=(BOX_T, 255))
    many[..., 3] = many[..., 1] + rng.integers(0, 20, size=(BOX_T, 255))
    c["255_boxes"] = dict(frames=f, boxes=many, box_labels=rng.integers(0, 1000, size=255), box_alpha=128, box_width=1,
                          box_visibles=rng.random((BOX_T, 255)) < 0.8)
    for s in (1, 4):
        c[f"labels_scale_{s}"] = dict(frames=f, boxes=_per_frame([[20, 4, 50, 30], [100, 20, 130, 34], [200, 30, 290, 35], [270, 12, 296, 30]]),
                                      box_labels=[7, 42, 999, 180], label_scale=s,
                                      box_colors=np.array([[20, 20, 20], [255, 255, 255], [255, 0, 0], [0, 255, 0]]))
    narrow = box_frames(W=50, seed=4)
    c["tag_wider_than_the_frame"] = dict(frames=narrow, boxes=_per_frame([[20, 10, 40, 30], [2, 20, 30, 36]]), box_labels=[888, 123],
                                         label_scale=4)
    c["with_overlay_and_dots"] = dict(frames=f, ids=ids, tracks=tracks, radius=3,
                                      boxes=_per_frame([[240, 5, 270, 20], [20, 18, 60, 30], [250, 2, 262, 12]]), box_labels=[1, 2, 3])
    c["with_overlay"] = dict(frames=f, ids=ids, alpha=100, contour=False, boxes=_per_frame([[240, 5, 270, 20], [20, 18, 60, 30]]))
    c["with_dots"] = dict(frames=f, tracks=tracks, radius=2, visibles=np.array([[True] * BOX_T, [True, False, True], [True] * BOX_T]),
                          boxes=_per_frame([[250, 2, 262, 12]]), box_labels=[5], box_alpha=256)
    for kw in c.values():
        for v in kw.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def box_expected(name):
    from fgvc_amd import viz
    out = viz.render(backend="host", **box_cases()[name])
    out.setflags(write=False)
    return out
