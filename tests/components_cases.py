"""Shared by test_components_host.py and test_gpu_components.py: the id maps the connected-component kernels (fgvc_seg_components_i32,
fgvc_seg_clean_u8) are held to.  The component cases sit on the seams of the labelling tile; the clean cases carry
their expected maps and statistics written out by hand.  Everything here runs on the CPU."""
import functools

import numpy as np

TR, TC = 16, 64         # fgvc_seg_ccl_tile_rows() / _cols(): one workgroup labels a tile of TR x TC pixels in LDS (the GPU test checks them)
WIDTHS = (1, TC - 1, TC, TC + 1, 2 * TC + 1)
HEIGHTS = (1, 2, TR, TR + 1, 2 * TR + 1)
H, W = 2 * TR + 1, 2 * TC + 1
VARIANTS = tuple((c, b) for c in (4, 8) for b in (False, True))        # (connectivity, background)


def run_map(T, h, w, seed, ids=(0, 0, 1, 2, 3, 255), max_run=6):
    """(T, h, w) uint8 of runs of random length 1 .. max_run in row-major order (objects_cases.run_map's style: runs wrap over row ends)."""
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
    m = run_map(T, h, w, 1000 * h + w)
    m.setflags(write=False)
    return m


def _serpentine(h, w, v=1):
    """a one-pixel path: every second row full, joined to the next full row at alternating ends"""
    m = np.zeros((h, w), np.uint8)
    m[0::2] = v
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = v
    return m


def _spiral(h, w, v=1):
    """a one-pixel path that winds inwards with a one-pixel gap between its turns"""
    m = np.zeros((h, w), np.uint8)
    y, x, dy, dx = 0, 0, 0, 1
    m[0, 0] = v

    def free(yy, xx):
        return not (0 <= yy < h and 0 <= xx < w) or m[yy, xx] == 0
    while True:
        for _ in range(2):                               # straight on, else one turn to the right
            ny, nx = y + dy, x + dx
            if 0 <= ny < h and 0 <= nx < w and m[ny, nx] == 0 and free(ny + dy, nx + dx):
                break
            dy, dx = dx, -dy
        else:
            return m
        y, x = ny, nx
        m[y, x] = v


@functools.lru_cache(maxsize=None)
def cases():
    """name -> ids (T, h, w) uint8."""
    c = {}
    s = _serpentine(H, W)
    c["serpentine"] = np.stack([s, _serpentine(W, H, 2).T.copy(), s[::-1, ::-1] * 3])
    sp = _spiral(H, W)
    c["spiral"] = np.stack([sp, sp[::-1].copy() * 2, sp[:, ::-1].copy()])
    comb = np.zeros((H, W), np.uint8)
    comb[:, 0::2] = 1
    comb[H - 1, :] = 1                                   # the teeth join along the bottom row only
    c["comb_u"] = np.stack([comb, comb * 2, comb])
    c["comb_u_mirrored"] = np.stack([comb[::-1].copy(), comb[::-1, ::-1].copy() * 2, comb[::-1].copy()])
    yy, xx = np.mgrid[0:H, 0:W]
    c["checkerboard"] = np.broadcast_to((1 + (yy + xx) % 2).astype(np.uint8), (3, H, W)).copy()
    d = np.zeros((3, H, W), np.uint8)
    d[0][yy - TR == xx - TC] = 1                         # through the corner where four tiles meet: (TR - 1, TC - 1) -> (TR, TC)
    d[1][yy - TR == -(xx - TC) - 1] = 2                  # the other diagonal: (TR - 1, TC) -> (TR, TC - 1)
    d[2] = 1
    d[2][yy - TR == xx - TC] = 0                         # zeros on a diagonal: id 0 is 4-connected whatever the connectivity
    c["diagonal_through_tile_corners"] = d
    b = np.zeros((3, H, W), np.uint8)
    b[0, TR - 4:TR, TC - 5:TC] = 1
    b[0, TR:TR + 3, TC:TC + 6] = 1
    b[1, TR - 4:TR, TC:TC + 5] = 2
    b[1, TR:TR + 3, TC - 6:TC] = 2
    b[2, 2 * TR - 2:2 * TR, TC - 3:TC] = 3
    b[2, 2 * TR:2 * TR + 1, TC:TC + 2] = 3
    c["blocks_touching_at_a_tile_corner"] = b
    c["all_256_ids"] = (np.arange(3 * H * W).reshape(3, H, W) * 7 % 256).astype(np.uint8)
    c["one_id_fills_the_frame"] = np.full((3, H, W), 5, np.uint8)
    e = np.zeros((3, H, W), np.uint8)
    e[0, H - 1, :] = 1
    e[1, 0, :] = 1                                       # the last row of frame 0 and the first row of frame 1: equal, and not joined
    e[1, H - 1, 3:9] = 2
    e[2, 0, 3:9] = 2
    c["last_row_equals_next_first_row"] = e
    c["one_pixel_frames"] = np.array([[[1]], [[0]], [[7]]], np.uint8)
    c["all_background"] = np.zeros((2, TR + 1, TC + 1), np.uint8)
    for m in c.values():
        m.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def expected(name, connectivity, background):
    from fgvc_amd import metrics
    want = metrics.components_host(cases()[name], connectivity, background)
    want.setflags(write=False)
    return want


@functools.lru_cache(maxsize=None)
def expected_sized(w, h, connectivity, background):
    from fgvc_amd import metrics
    want = metrics.components_host(sized(w, h), connectivity, background)
    want.setflags(write=False)
    return want


# ---- the cleaning rule: maps with their answers written out ------------------------------------------------------------------------------------
def art(*rows):
    """rows of characters -> (h, w) uint8: '.' is 0, a digit its value"""
    return np.array([[0 if ch == "." else int(ch) for ch in row] for row in rows], np.uint8)


def _case(ids, want, n_ids, stats, **kw):
    ids, want = (np.asarray(a, np.uint8) for a in (ids, want))
    if ids.ndim == 2:
        ids, want = ids[None], want[None]
    st = np.zeros((ids.shape[0], n_ids, 4), np.int64)
    for (t, o), words in stats.items():
        st[t, o] = words
    for a in (ids, want, st):
        a.setflags(write=False)
    return dict(ids=ids, want=want, n_ids=n_ids, stats=st, kw=kw)


@functools.lru_cache(maxsize=None)
def clean_cases():
    """name -> dict(ids (T, h, w), want (T, h, w), n_ids, stats (T, n_ids, 4), kw): clean_masks_host(ids, n_ids, **kw) == (want, stats).
    stats words: components before the drop, components kept, pixels dropped, pixels filled."""
    c = {}
    # id 1: parts of 3 and 2 pixels; id 2: parts of 3 and 1 -- an area of exactly min_area stays, min_area - 1 goes
    c["area_exactly_min_area_is_kept"] = _case(
        art("11.1.",
            "1..1.",
            ".....",
            "222.2"),
        art("11...",
            "1....",
            ".....",
            "222.."), 3, {(0, 1): (2, 1, 2, 0), (0, 2): (2, 1, 1, 0)}, min_area=3)
    # id 1: two parts of 2 pixels, roots 1 and 10 -- the smaller root stays; id 2: parts of 1 and 3 pixels
    c["equal_areas_the_smaller_root_stays"] = _case(
        art(".11.2",
            ".....",
            "11...",
            "..222"),
        art(".11..",
            ".....",
            ".....",
            "..222"), 3, {(0, 1): (2, 1, 2, 0), (0, 2): (2, 1, 1, 0)}, keep="largest")
    speck = art(".......",
                ".11111.",
                ".11111.",
                ".11211.",
                ".11111.",
                ".......")
    speck_clean = np.where(speck == 2, 1, speck)
    c["speck_inside_is_dropped_then_filled"] = _case(speck, speck_clean, 3, {(0, 1): (1, 1, 0, 1), (0, 2): (1, 0, 1, 0)}, min_area=2,
                                                     fill_holes=True)
    border = art("111",
                 "1.1",
                 "1.1")
    c["hole_touching_the_border_is_not_filled"] = _case(border, border, 2, {(0, 1): (1, 1, 0, 0)}, fill_holes=True)
    two = art(".....",
              ".112.",
              ".1.2.",
              ".122.",
              ".....")
    c["hole_bounded_by_two_ids_is_not_filled"] = _case(two, two, 3, {(0, 1): (1, 1, 0, 0), (0, 2): (1, 1, 0, 0)}, fill_holes=True)
    c["hole_meeting_the_outside_diagonally_is_filled"] = _case(
        art(".....",
            ".11..",
            ".1.1.",
            "..11.",
            "....."),
        art(".....",
            ".11..",
            ".111.",
            "..11.",
            "....."), 2, {(0, 1): (1, 1, 0, 1)}, fill_holes=True)
    c["max_hole_area_at_its_boundary"] = _case(
        art("..........",
            ".11111111.",
            ".1..1...1.",
            ".11111111.",
            ".........."),
        art("..........",
            ".11111111.",
            ".1111...1.",
            ".11111111.",
            ".........."), 2, {(0, 1): (1, 1, 0, 2)}, fill_holes=True, max_hole_area=2)
    # id 9 >= n_ids = 2: its pixels stay, the hole it helps to bound and the hole it bounds alone stay; the lone pixel of id 1 goes
    c["ids_beyond_n_ids_are_untouched_and_block_a_fill"] = _case(
        art("........",
            ".111.999",
            ".1.9.9.9",
            ".111.999",
            ".......1"),
        art("........",
            ".111.999",
            ".1.9.9.9",
            ".111.999",
            "........"), 2, {(0, 1): (2, 1, 1, 0)}, min_area=2, fill_holes=True)
    c["frames_switched_off_are_unchanged"] = _case(np.stack([speck, speck, speck]), np.stack([speck, speck_clean, speck]), 3,
                                                   {(1, 1): (1, 1, 0, 1), (1, 2): (1, 0, 1, 0)}, min_area=2, fill_holes=True,
                                                   frames=(False, True, False))
    noisy = run_map(2, 9, 21, 3, ids=(0, 1, 2), max_run=3)
    from fgvc_amd import metrics
    lab = metrics.components_host(noisy)
    counts = {(t, o): (n, n, 0, 0) for t in range(2) for o in (1, 2) for n in [len(np.unique(lab[t][noisy[t] == o]))]}
    c["a_spec_that_does_nothing_returns_its_input"] = _case(noisy, noisy, 3, counts, min_area=1)
    return c


def clean_kwargs(kw):
    """the case's keywords with `frames` as the array the host contract takes"""
    kw = dict(kw)
    if "frames" in kw:
        kw["frames"] = np.array(kw["frames"], bool)
    return kw


CLEAN_SWEEP = (dict(min_area=4), dict(keep="largest"), dict(fill_holes=True), dict(min_area=3, keep="largest", fill_holes=True, max_hole_area=5),
               dict(min_area=6, fill_holes=True, connectivity=4))
