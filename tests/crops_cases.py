"""Shared by test_crops_host.py and test_gpu_crops.py: the cases the object crops are held to -- statistics rows with
their windows worked out by hand for the window rule (metrics.object_windows_host / fgvc_seg_object_windows_i64), and frames with explicit
windows for the resampling rule (viz.crop_windows_host / fgvc_frames_object_crops_u8).  Everything here runs on the CPU."""
import functools

import numpy as np

BAND = 8                 # output rows one workgroup of the resample kernel owns
COLS = 64                # output columns one workgroup owns
FRAME_SIZES = ((37, 53), (64, 96))
FRAME_COUNTS = (1, 3, 5)
# (33, 48): five bands, the last of one row, and a ragged column chunk; (9, 130): three column chunks, the last of two columns
SIZES = ((1, 1), (5, 7), (16, 16), (33, 48), (9, 130))


def _stats(boxes):
    """boxes: per frame a list of (x0, y0, x1, y1) or None per id 1 .. -> (T, N, 8) int64 with row 0 (the background) absent"""
    T, N = len(boxes), 1 + len(boxes[0])
    s = np.zeros((T, N, 8), np.int64)
    for t, row in enumerate(boxes):
        for o, b in enumerate(row, 1):
            if b is not None:
                x0, y0, x1, y1 = b
                s[t, o] = (max((x1 - x0) * (y1 - y0), 1), x0, y0, x1, y1, 0, 0, 0)
    return s


GAP = [[(0, 0, 10, 10)], [(2, 4, 12, 10)], [None], [(6, 4, 20, 12)], [(9, 5, 21, 15)]]


@functools.lru_cache(maxsize=None)
def window_cases():
    """name -> (stats, kwargs of object_windows_host, expected (T, M, 8) worked out by hand; see the arithmetic beside each)."""
    c = {}
    # Wm, Hm = 20, 30; pad_q = 128: Wp = 20 + 2 ceil(2560 / 1024) = 26, Hp = 30 + 2 ceil(3840 / 1024) = 38; 26 * 16 < 38 * 16: Wp = 38;
    # wx0 = (40 - 38) // 2 = 1, wy0 = (70 - 38) // 2 = 16
    c["one_frame_one_object"] = (_stats([[(10, 20, 30, 50)]]), dict(size=(16, 16), pad=0.125, min_side=8, mask_size=(64, 96)),
                                 [[[1, 16, 39, 54, 1, 16, 39, 54]]])
    # 1 + 2 ceil(128 / 1024) = 3 < min_side: Wp = Hp = 8; S = (5, 7): 8 * 5 < 8 * 7: Wp = ceil(56 / 5) = 12; wx0 = (11 - 12) // 2 = -1
    # (an odd negative numerator: truncation gives 0), wy0 = (15 - 8) // 2 = 3
    c["one_pixel_object"] = (_stats([[(5, 7, 6, 8)]]), dict(size=(5, 7), pad=0.125, min_side=8, mask_size=(37, 53)),
                             [[[-1, 3, 11, 11, -1, 3, 11, 11]]])
    # pad_q = 256: Wp = 53 + 2 ceil(13568 / 1024) = 53 + 28 = 81, Hp = 37 + 2 ceil(9472 / 1024) = 57; 81 * 16 >= 57 * 16: Hp = 81;
    # wx0 = (53 - 81) // 2 = -14, wy0 = (37 - 81) // 2 = -22: outside the 37 x 53 frame on all four sides
    c["whole_frame_with_pad"] = (_stats([[(0, 0, 53, 37)]]), dict(size=(16, 16), pad=0.25, min_side=8, mask_size=(37, 53)),
                                 [[[-14, -22, 67, 59, -14, -22, 67, 59]]])
    # boxes of widths 10, 10, -, 14, 12 and heights 10, 6, -, 8, 10; x0 + x1 = 10, 14, -, 26, 30; y0 + y1 = 10, 14, -, 16, 20
    # t = 0: U = {0, 1}: 10 x 10, ((24 - 20) // 4, (24 - 20) // 4) = (1, 1)
    # t = 1: U = {0, 1, 3}: 14 x 10 -> 14 x 14, ((50 - 42) // 6, (40 - 42) // 6) = (1, -1)          (-2 // 6 = -1; truncation gives 0)
    # t = 2: absent at t itself: zeros
    # t = 3: U = {1, 3, 4} (absent at t - 1): 14 x 14, ((70 - 42) // 6, (50 - 42) // 6) = (4, 1)
    # t = 4: U = {3, 4}: 14 x 14, ((56 - 28) // 4, (36 - 28) // 4) = (7, 2)
    c["smooth_2_across_a_gap"] = (_stats(GAP), dict(size=(16, 16), pad=0.0, min_side=1, smooth=2, mask_size=(64, 96)),
                                  [[[1, 1, 11, 11] * 2], [[1, -1, 15, 13] * 2], [[0] * 8], [[4, 1, 18, 15] * 2], [[7, 2, 21, 16] * 2]])
    # U = {0, 1, 3, 4} on every present frame: 14 x 14, ((80 - 56) // 8, (60 - 56) // 8) = (3, 0)
    c["smooth_larger_than_T"] = (_stats(GAP), dict(size=(16, 16), pad=0.0, min_side=1, smooth=100, mask_size=(64, 96)),
                                 [[[3, 0, 17, 14] * 2], [[3, 0, 17, 14] * 2], [[0] * 8], [[3, 0, 17, 14] * 2], [[3, 0, 17, 14] * 2]])
    # Wp = Hp = 8 = min_side; (3 - 8) // 2 = -3 (truncation: -2)
    c["odd_negative_numerator"] = (_stats([[(0, 0, 3, 3)]]), dict(size=(16, 16), pad=0.0, min_side=8, mask_size=(64, 96)),
                                   [[[-3, -3, 5, 5, -3, -3, 5, 5]]])
    # S = (33, 48): 20 * 33 >= 10 * 48: Hp = ceil(660 / 48) = 14; wx0 = (40 - 20) // 2 = 10, wy0 = (30 - 14) // 2 = 8
    c["non_square_size"] = (_stats([[(10, 10, 30, 20)]]), dict(size=(33, 48), pad=0.0, min_side=1, mask_size=(64, 96)),
                            [[[10, 8, 30, 22, 10, 8, 30, 22]]])
    # the first case at 9 / 4 the mask: (1 * 216 // 96, 16 * 144 // 64, ceil(39 * 216 / 96), ceil(54 * 144 / 64)) = (2, 36, 88, 122)
    c["frame_9_4_of_the_mask"] = (_stats([[(10, 20, 30, 50)]]),
                                  dict(size=(16, 16), pad=0.125, min_side=8, mask_size=(64, 96), frame_size=(144, 216)),
                                  [[[1, 16, 39, 54, 2, 36, 88, 122]]])
    # (-3 * 216) // 96 = -7 (-6.75), (-3 * 144) // 64 = -7, ceil(1080 / 96) = 12, ceil(720 / 64) = 12
    c["frame_9_4_negative_origin"] = (_stats([[(0, 0, 3, 3)]]),
                                      dict(size=(16, 16), pad=0.0, min_side=8, mask_size=(64, 96), frame_size=(144, 216)),
                                      [[[-3, -3, 5, 5, -7, -7, 12, 12]]])
    # a box left of and above the map (statistics are only integers to the rule): 20 x 20, wx0 = (-60 - 20) // 2 = -40, wy0 = -30;
    # (-40 * 216 // 96, -30 * 144 // 64, ceil(-4320 / 96), ceil(-1440 / 64)) = (-90, -68, -45, -22): both roundings on negative numerators
    c["negative_ceiling"] = (_stats([[(-40, -30, -20, -10)]]),
                             dict(size=(16, 16), pad=0.0, min_side=1, mask_size=(64, 96), frame_size=(144, 216)),
                             [[[-40, -30, -20, -10, -90, -68, -45, -22]]])
    # two objects, the second chosen alone and then both in reverse order
    two = _stats([[(10, 20, 30, 50), (0, 0, 3, 3)]])
    c["objects_subset"] = (two, dict(size=(16, 16), pad=0.0, min_side=8, mask_size=(64, 96), objects=[2]), [[[-3, -3, 5, 5, -3, -3, 5, 5]]])
    # object 1 without pad: 20 x 30 -> 30 x 30, ((40 - 30) // 2, (70 - 30) // 2) = (5, 20)
    c["objects_reversed"] = (two, dict(size=(16, 16), pad=0.0, min_side=8, mask_size=(64, 96), objects=[2, 1]),
                             [[[-3, -3, 5, 5, -3, -3, 5, 5], [5, 20, 35, 50, 5, 20, 35, 50]]])
    return {k: (s, kw, np.asarray(e, np.int64)) for k, (s, kw, e) in c.items()}


def blob_ids(T, h, w, seed, n_objects=3):
    """(T, h, w) uint8: n_objects drifting rectangles, object 2 absent on the middle frame, object 3 leaving through the right border"""
    rng = np.random.default_rng(seed)
    ids = np.zeros((T, h, w), np.uint8)
    for o in range(1, n_objects + 1):
        bw, bh = int(rng.integers(3, max(4, w // 3))), int(rng.integers(3, max(4, h // 3)))
        x, y = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
        for t in range(T):
            if o == 2 and T > 2 and t == T // 2:
                continue
            dx = (x + t * (o if o != 3 else 7)) if o != 3 else (w - bw + t * 2)
            ids[t, max(0, y + t):y + t + bh, max(0, dx):dx + bw] = o
    return ids


@functools.lru_cache(maxsize=None)
def frames(T, H, W, seed=0):
    """(T, H, W, 3) uint8: noise over a gradient, so that both a wrong tap and a wrong origin show"""
    rng = np.random.default_rng(1000 * H + W + seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), ((xx + yy) * 7) % 256], -1)
    f = np.clip(base[None] + rng.integers(-60, 61, (T, H, W, 3)), 0, 255).astype(np.uint8)
    f.setflags(write=False)
    return f


def named_windows(H, W, S_h, S_w):
    """name -> (x0, y0, x1, y1): the windows every size is resampled from, on an H x W frame"""
    return {
        "up_3x3": (W // 2 - 1, H // 2 - 1, W // 2 + 2, H // 2 + 2),                 # upscaling (for S > 3): three taps
        "identity": (6, 3, 6 + S_w, 3 + S_h),                                      # the output's own size
        "down_5p3_x": (2, 1, 2 + (53 * S_w + 9) // 10, 1 + S_h),                   # about 5.3 on x, 1 on y
        "down_12_y": (3, -4, 3 + S_w, -4 + 12 * S_h),                              # 12 on y only
        "down_both": (1, 2, 1 + (37 * S_w) // 10, 2 + (29 * S_h) // 10),
        "left": (-5, 10, 12, 25), "right": (W - 9, 10, W + 6, 25), "top": (10, -6, 25, 9), "bottom": (10, H - 7, 25, H + 8),
        "top_left": (-4, -4, 9, 9), "top_right": (W - 8, -5, W + 5, 8), "bottom_left": (-6, H - 9, 7, H + 4),
        "bottom_right": (W - 7, H - 7, W + 6, H + 6),
        "outside_right": (W + 20, H + 5, W + 40, H + 30), "outside_top_left": (-50, -50, -30, -35),
        "one_column": (7, 5, 8, 30), "one_row": (7, 5, 30, 6), "one_pixel": (4, 4, 5, 5),
        "whole_frame": (0, 0, W, H), "around_the_frame": (-3, -2, W + 4, H + 5),
        "invalid_x": (5, 5, 5, 9), "invalid_reversed": (9, 5, 3, 9), "invalid_zeros": (0, 0, 0, 0),
    }


def window_array(T, H, W, S_h, S_w):
    """(T, M, 4) int64: named_windows on every frame, shifted by (2 t, -t) so that no two frames share a plan"""
    base = np.asarray(list(named_windows(H, W, S_h, S_w).values()), np.int64)
    return np.stack([base + np.array([2 * t, -t, 2 * t, -t]) * (base[:, 2:3] > base[:, 0:1]) for t in range(T)])


def random_windows(T, M, H, W, seed, inside=False):
    """(T, M, 4) int64 random windows of 1 .. 59 pixels a side; inside=True: within the frame"""
    rng = np.random.default_rng(seed)
    out = np.zeros((T, M, 4), np.int64)
    for t in range(T):
        for j in range(M):
            if inside:
                ww, wh = int(rng.integers(1, min(60, W) + 1)), int(rng.integers(1, min(60, H) + 1))
                x0, y0 = int(rng.integers(0, W - ww + 1)), int(rng.integers(0, H - wh + 1))
            else:
                ww, wh = int(rng.integers(1, 60)), int(rng.integers(1, 60))
                x0, y0 = int(rng.integers(-10, W)), int(rng.integers(-10, H))
            out[t, j] = (x0, y0, x0 + ww, y0 + wh)
    return out


@functools.lru_cache(maxsize=None)
def expected_crops(T, H, W, S_h, S_w, fill=(0, 0, 0), max_taps=None):
    """viz.crop_windows_host of frames(T, H, W) on window_array(...), computed once"""
    from fgvc_amd import viz
    want = viz.crop_windows_host(frames(T, H, W), window_array(T, H, W, S_h, S_w), (S_h, S_w), fill=np.asarray(fill, np.uint8),
                                 max_taps=max_taps)
    want.setflags(write=False)
    return want
