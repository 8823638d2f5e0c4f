"""Show a result: point tracks and mask overlays painted onto uint8 RGB video.

    paint_point_track(frames, point_tracks, visibles, colors)    the reference's dot painter (flyingthingsplus/utils/visualize.py:85-155)
    overlay_masks(frames, ids, palette, alpha, contour)          object ids blended in, integer arithmetic, optional contour
    render(frames, ids=..., tracks=..., visibles=...)            overlay, then points; with trail=L: overlay, trails, points
    paint_trails(frames, point_tracks, visibles, trail=8)        every point's last L steps as a fading poly-line
    paint_pose(frames, joints, visibles, skeleton=, heat=)       joint heat maps, limbs and dots
    paint_boxes(frames, boxes, box_visibles, box_labels=)        object boxes as rings with id tags
    pose_tracks(coords), pose_visibles(coords, peak, min_conf)   the pose call's (2, K, T) coordinates as what the painters take
    frames_to_yuv420(frames, fmt, matrix, range, siting)         the painted frames as packed 8-bit 4:2:0 video

backend='host' is plain numpy: it is the contract, the default, and works without a GPU.  backend='hip' is ONE launch of
fgvc_render_frames_u8 (ops.render_frames) and is held to the host backend with `==`.  The per-pixel arithmetic, both backends:

  overlay   k = ids[t, y, x] > 0:  out_c = (frame_c (256 - alpha) + palette[k][c] alpha + 128) >> 8;  with contour=True a pixel whose left,
            right, upper or lower in-image neighbour has another id takes palette[k] itself;  k == 0: the frame's pixel.
  points    for every visible point i in index order: x = track_x + 0.5 clamped to [0, W], x1 = floor(x), x2 = x1 + 1 (y alike); at the
            pixels a = py + r + 1 - y1, b = px + r + 1 - x1 in [0, 2 r + 1], with I the (2 r + 1)^2 icon (zero outside),
              patch = I(a, b) (x2 - x) (y2 - y) + I(a - 1, b) (x2 - x) (y - y1) + I(a, b - 1) (x - x1) (y2 - y) + I(a - 1, b - 1) (x - x1) (y - y1)
              v_c   = (1 - patch) v_c + patch colour[i][c], truncated to uint8 -- after EVERY point, as the reference's assignment into its
            uint8 image does; float64 throughout, each product left to right.  A point with a non-finite coordinate is skipped.
  trails    (trail=L; between the overlay and the points; backend='hip': ONE launch of fgvc_render_trails_u8, ops.render_trails)  on frame t,
            for every point i in index order and every step s = max(0, t - L) .. t - 1, oldest first: the segment from A = track[i, s] + 0.5
            to B = track[i, s + 1] + 0.5 (pixel (px, py) is the point (px, py); the + 0.5 is the dots' own shift), drawn only if both ends
            are visible and all four coordinates are below 2**20 in magnitude (NaN and the infinities are not); ends are not clamped.
            With d = B - A, L2 = dx dx + dy dy, ro = linewidth / 2 + 0.5, ri = max(linewidth / 2 - 0.5, 0), ro2 = ro ro, g = 1 / (ro2 - ri ri):
              u   = 0 if L2 == 0 else min(max(((px - ax) dx + (py - ay) dy) / L2, 0), 1)
              ex  = px - (ax + u dx), ey = py - (ay + u dy), d2 = ex ex + ey ey
              cov = min(max((ro2 - d2) g, 0), 1), op = cov fade[t - 1 - s]
              v_c = (1 - op) v_c + op colour_c, truncated to uint8 after EVERY segment; cov <= 0: the pixel keeps its value
            float64, every product and sum left to right, no square root, one (correctly rounded) division.  Not OpenCV's LINE_AA rasteriser
            (the reference's draw_traj_on_image_py), whose bytes nothing here can pin; the joint of two consecutive segments is blended twice.
  heat      (heat=(T, K, H, W) float32 | float64; after the overlay; backend='hip': ONE launch of fgvc_render_pose_u8, ops.render_pose)  per
            pixel, for k = 0 .. K - 1 in order, with v = heat[t, k, y, x] widened to float64:
              a   = min(max(v heat_gain, 0), 1) heat_alpha;  not a > 0 (zero, negative, NaN): the pixel keeps its value
              v_c = (1 - a) v_c + a heat_colors[k][c], truncated to uint8 after EVERY map.
  limbs     (skeleton=(E, 2) joint indices; after the heat, before the points; the same launch)  on frame t, for every edge e = (a, b) in
            order: the trails' segment from A = track[a, t] + 0.5 to B = track[b, t] + 0.5 with linewidth = limb_width, drawn only if both
            ends are visible on t and all four coordinates are below 2**20 in magnitude; op = cov limb_alpha, colour limb_colors[e] (None:
            the colour of joint b), truncated to uint8 after EVERY limb.  a == b and a zero-length limb are discs (L2 == 0).
  boxes     (boxes=(T, N, 4) integers (x0, y0, x1, y1), half-open; after the overlay, before the points; backend='hip': ONE launch of
            fgvc_render_boxes_u8, ops.render_boxes)  on frame t, box i = 0 .. N - 1 in order; a box with x1 <= x0 or y1 <= y0 or with
            box_visibles[t, i] false draws nothing (engine.ObjectTracks' boxes and present are exactly that).  With bw = box_width,
            a = box_alpha, C = box_colors[i] (None: palette[i]), every step on the pixels inside the frame, integers only:
              ring    the pixels of [x0 - bw, x1 + bw) x [y0 - bw, y1 + bw) that are NOT in the box (the object stays uncovered):
                      v_c = (v_c (256 - a) + C_c a + 128) >> 8, the overlay's formula
              tag     (box_labels given)  d = the decimal digits of box_labels[i], s = label_scale, tw = (6 d + 1) s, th = 9 s;
                      ty = y0 - bw - th (on top of the ring), or y0 when that is above row 0; tx = x0 - bw, or max(W - tw, 0) when the tag
                      would end beyond column W.  [tx, tx + tw) x [ty, ty + th) blends as the ring does
              digits  glyph g = 0 .. d - 1 from the left (most significant digit first) of DIGITS_5X7: its row r, column c (bit 4 - c of the
                      row) is the s x s block at (tx + (1 + 6 g + c) s, ty + (1 + r) s), set -- opaque -- to white when
                      299 C_r + 587 C_g + 114 C_b < 128000, else to black
            boxes= goes with neither trail= nor skeleton= / heat= (one stage per launch).
Tracks are (x, y) in the pixel frame of `frames` (scale_tracks for tracks predicted at another size) and are converted to float64 first.
"""
from __future__ import annotations

import colorsys
import functools
from typing import Optional, Tuple

import numpy as np

BACKENDS = ("host", "hip")
MAX_RADIUS = 31
MAX_TRAIL = 64
LINEWIDTHS = (1.0, 16.0)
TRAIL_LIMIT = float(2 ** 20)    # a segment with a coordinate at or beyond it (or NaN) is not drawn
TRAIL_COLOR_BY = ("track", "time")
MAX_HEAT_MAPS = 256
# The 14 limbs of a JHMDB puppet over the dataset's joint order -- 0 neck, 1 belly, 2 face, 3 right shoulder, 4 left shoulder, 5 right hip,
# 6 left hip, 7 right elbow, 8 left elbow, 9 right knee, 10 left knee, 11 right wrist, 12 left wrist, 13 right ankle, 14 left ankle.
_JHMDB_EDGES = ((0, 1), (0, 2), (0, 3), (0, 4), (1, 5), (1, 6), (3, 7), (7, 11), (4, 8), (8, 12), (5, 9), (9, 13), (6, 10), (10, 14))
DOT_FRACTION = 0.015          # the reference's dot_size_as_fraction_of_min_edge
MAX_BOXES = 255
BOX_WIDTHS = (1, 16)
BOX_LIMIT = 2 ** 20           # a box coordinate at or beyond it in magnitude is refused
MAX_LABEL = 999
LABEL_SCALES = (1, 4)
SHARPNESS = 0.15


# ---- tables ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _davis_palette() -> np.ndarray:
    pal = np.zeros((256, 3), np.uint8)
    for k in range(256):
        c, v = k, [0, 0, 0]
        for j in range(8):                                   # bit 3 j + ch of the id -> bit 7 - j of channel ch
            for ch in range(3):
                v[ch] |= ((c >> ch) & 1) << (7 - j)
            c >>= 3
        pal[k] = v
    pal.setflags(write=False)
    return pal


def davis_palette() -> np.ndarray:
    """(256, 3) uint8: the VOC / DAVIS bit-pattern palette -- (0, 0, 0), (128, 0, 0), (0, 128, 0), (128, 128, 0), ..."""
    return _davis_palette().copy()


def track_colors(num_points: int) -> np.ndarray:
    """(P, 3) uint8, deterministic: P hues evenly round the circle at lightness 0.55, saturation 0.95, neighbours in index far apart in hue
    (the reference draws lightness and saturation at random and shuffles: its colours enter only as an explicit `colors`)."""
    P = int(num_points)
    out = np.zeros((P, 3), np.uint8)
    step = next(s for s in range(max(1, int(round(P * 0.381966))), P + 2) if np.gcd(s, max(P, 1)) == 1)     # a golden-angle stride, coprime to P
    for i in range(P):
        r, g, b = colorsys.hls_to_rgb(((i * step) % P) / P, 0.55, 0.95)
        out[i] = (int(r * 255), int(g * 255), int(b * 255))
    return out


def _jhmdb_skeleton() -> np.ndarray:
    sk = np.array(_JHMDB_EDGES, np.int32)
    sk.setflags(write=False)
    return sk


JHMDB_SKELETON = _jhmdb_skeleton()
"""JHMDB_SKELETON: (14, 2) int32, read-only, zero-based: the limbs of the JHMDB puppet as a tree over its 15 joints (neck, belly, face, right
and left shoulder, hip, elbow, knee, wrist, ankle).  Restated from the dataset's public description of its joint order; it is UNPINNED:
no JHMDB data is available offline to check it against.  BADJA has no agreed skeleton: pass the edges."""


def _digits_5x7() -> np.ndarray:
    rows = ("01110 10001 10011 10101 11001 10001 01110", "00100 01100 00100 00100 00100 00100 01110",
            "01110 10001 00001 00010 00100 01000 11111", "11110 00001 00001 01110 00001 00001 11110",
            "00010 00110 01010 10010 11111 00010 00010", "11111 10000 11110 00001 00001 10001 01110",
            "00110 01000 10000 11110 10001 10001 01110", "11111 00001 00010 00100 01000 01000 01000",
            "01110 10001 10001 01110 10001 10001 01110", "01110 10001 10001 01111 00001 00010 01100")
    t = np.array([[int(r, 2) for r in g.split()] for g in rows], np.uint8)
    t.setflags(write=False)
    return t


DIGITS_5X7 = _digits_5x7()
"""DIGITS_5X7: (10, 7) uint8, read-only: the ten decimal digits as 5 x 7 bitmaps drawn for this project, one byte a row, bit 4 the
leftmost column."""


def default_radius(h: int, w: int) -> int:
    """The reference's dot radius, int(round(min(H, W) * 0.015)): 0 below 34 px (refused by the painters: the icon divides by it)."""
    return int(round(min(int(h), int(w)) * DOT_FRACTION))


def check_radius(radius: Optional[int], h: int, w: int) -> int:
    r = default_radius(h, w) if radius is None else int(radius)
    if r < 1:
        raise ValueError(f"radius={r}: at least 1 (the icon divides by the radius; the default is 0 for frames under 34 px: pass radius=)")
    if r > MAX_RADIUS:
        raise ValueError(f"radius={r}: at most {MAX_RADIUS}")
    return r


@functools.lru_cache(maxsize=None)
def _icon_table(radius: int) -> np.ndarray:
    r = int(radius)
    d = 2 * r + 1
    qy = np.square(np.arange(d)[:, np.newaxis] - r - 1)      # off centre by one: the reference's, part of the contract
    qx = np.square(np.arange(d)[np.newaxis, :] - r - 1)
    icon = (qy + qx) - (r ** 2) / 2.0
    icon = 1 - np.clip(icon / (r * 2 * SHARPNESS), 0, 1)
    icon = np.ascontiguousarray(icon, dtype=np.float64)
    icon.setflags(write=False)
    return icon


def icon_table(radius: int) -> np.ndarray:
    """(2 r + 1, 2 r + 1) float64, read-only: the dot's opacity."""
    return _icon_table(int(radius))

@functools.lru_cache(maxsize=None)
def _trail_fade(length: int) -> np.ndarray:
    L = int(length)
    fade = (L - np.arange(L, dtype=np.float64)) / L
    fade.setflags(write=False)
    return fade


def trail_fade(length: int) -> np.ndarray:
    """(L,) float64, read-only: the default opacity of a trail segment by its age in frames, (L - age) / L -- 1 for the newest step."""
    L = int(length)
    if not 1 <= L <= MAX_TRAIL:
        raise ValueError(f"trail={length!r}: an integer in 1 .. {MAX_TRAIL}")
    return _trail_fade(L)


def spring_colors(num_frames: int) -> np.ndarray:
    """(T - 1, 3) uint8: the colour of step s by time, matplotlib's 'spring' map through its 256-entry table as the reference's trajectory
    drawing samples it (improc.py draw_traj_on_image_py): (255, k, 255 - k) with k = min(int(s / max(1, T - 2) * 256), 255)."""
    T = int(num_frames)
    out = np.zeros((max(T - 1, 0), 3), np.uint8)
    for s in range(T - 1):
        k = min(int(s / max(1, T - 2) * 256), 255)
        out[s] = (255, k, 255 - k)
    return out


def trail_consts(linewidth: float):
    """(ro2, g, reach) of a line width: the two doubles of the coverage ramp, made ONCE here for both backends, and ceil(ro), what a
    segment's box is grown by."""
    lw = float(linewidth)
    ro = lw / 2 + 0.5
    ri = max(lw / 2 - 0.5, 0.0)
    ro2 = ro * ro
    return ro2, 1.0 / (ro2 - ri * ri), int(np.ceil(ro))


def scale_tracks(tracks, from_size: Tuple[int, int], to_size: Tuple[int, int]) -> np.ndarray:
    """Tracks (..., 2) as (x, y) predicted on frames of from_size = (h, w) -> float64 in the pixel frame of to_size = (h, w)."""
    t = np.array(_numpy(tracks), dtype=np.float64)
    if t.ndim < 1 or t.shape[-1] != 2:
        raise ValueError(f"tracks: (..., 2) as (x, y), got {t.shape}")
    (fh, fw), (th, tw) = from_size, to_size
    if min(fh, fw, th, tw) <= 0:
        raise ValueError(f"sizes must be positive, got {from_size} -> {to_size}")
    t[..., 0] *= float(tw) / float(fw)
    t[..., 1] *= float(th) / float(fh)
    return t


# ---- argument checks (one set for both backends) --------------------------------------------------------------------------------------------
def _numpy(x):
    if x is None or isinstance(x, np.ndarray):
        return x
    if hasattr(x, "detach"):
        return x.detach().cpu().numpy()
    return np.asarray(x)


def _is_cuda(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def _check_frames(frames):
    if frames.dtype != np.uint8:
        raise TypeError(f"frames: expected uint8, got {frames.dtype}")
    if frames.ndim != 4 or frames.shape[3] != 3:
        raise ValueError(f"frames: (T, H, W, 3), got {frames.shape}")


def _check_overlay(frames, ids, palette, alpha):
    if ids.dtype != np.uint8:
        raise TypeError(f"ids: expected uint8 object ids, got {ids.dtype}")
    if ids.shape != frames.shape[:3]:
        raise ValueError(f"ids: {frames.shape[:3]} to go with the frames, got {ids.shape}")
    palette = _davis_palette() if palette is None else palette
    if palette.dtype != np.uint8:
        raise TypeError(f"palette: expected uint8, got {palette.dtype}")
    if palette.shape != (256, 3):
        raise ValueError(f"palette: (256, 3), got {palette.shape}")
    if int(alpha) != alpha or not 0 <= int(alpha) <= 256:
        raise ValueError(f"alpha={alpha!r}: an integer in 0 .. 256")
    return palette, int(alpha)


def _check_points(frames, tracks, visibles, colors, radius):
    T, H, W = frames.shape[:3]
    if tracks.ndim != 3 or tracks.shape[1] != T or tracks.shape[2] != 2:
        raise ValueError(f"point_tracks: (P, {T}, 2) to go with the frames, got {tracks.shape}")
    if tracks.dtype.kind not in "fiu":
        raise TypeError(f"point_tracks: a real number type, got {tracks.dtype}")
    tracks = tracks.astype(np.float64)
    P = tracks.shape[0]
    if visibles is None:
        visibles = np.ones((P, T), bool)
    if visibles.dtype != np.bool_:
        raise TypeError(f"visibles: expected bool, got {visibles.dtype}")
    if visibles.shape != (P, T):
        raise ValueError(f"visibles: {(P, T)} to go with the tracks, got {visibles.shape}")
    if colors is None:
        colors = track_colors(P)
    if colors.dtype.kind not in "iu":
        raise TypeError(f"colors: integers in 0 .. 255, got {colors.dtype}")
    if colors.shape != (P, 3):
        raise ValueError(f"colors: {(P, 3)} to go with the tracks, got {colors.shape}")
    if colors.size and (int(colors.min()) < 0 or int(colors.max()) > 255):
        raise ValueError("colors: integers in 0 .. 255")
    return tracks, visibles, colors.astype(np.uint8), check_radius(radius, H, W)

def _check_trails(trail, linewidth, fade, color_by):
    """-> (L, linewidth, fade (L,) float64)"""
    if isinstance(trail, (bool, np.bool_)) or not isinstance(trail, (int, np.integer)) or not 1 <= int(trail) <= MAX_TRAIL:
        raise ValueError(f"trail={trail!r}: an integer in 1 .. {MAX_TRAIL}")
    L = int(trail)
    try:
        lw = float(linewidth)
    except (TypeError, ValueError):
        raise ValueError(f"linewidth={linewidth!r}: a number in {list(LINEWIDTHS)}") from None
    if not LINEWIDTHS[0] <= lw <= LINEWIDTHS[1]:
        raise ValueError(f"linewidth={linewidth!r}: a number in {list(LINEWIDTHS)}")
    if color_by not in TRAIL_COLOR_BY:
        raise ValueError(f"trail_color_by={color_by!r}: one of {TRAIL_COLOR_BY}")
    if fade is None:
        fade = _trail_fade(L)
    else:
        fade = np.asarray(_numpy(fade))
        if fade.dtype.kind not in "fiu":
            raise ValueError(f"trail_fade: ({L},) real numbers in [0, 1], got {fade.dtype}")
        fade = np.ascontiguousarray(fade, dtype=np.float64)
        if fade.shape != (L,):
            raise ValueError(f"trail_fade: ({L},) to go with trail={L}, got {fade.shape}")
        if not bool(((fade >= 0.0) & (fade <= 1.0)).all()):
            raise ValueError("trail_fade: values in [0, 1]")
    return L, lw, fade


def _check_limb_consts(limb_width, limb_alpha):
    """-> (limb_width, limb_alpha) as floats"""
    try:
        lw = float(limb_width)
    except (TypeError, ValueError):
        raise ValueError(f"limb_width={limb_width!r}: a number in {list(LINEWIDTHS)}") from None
    if not LINEWIDTHS[0] <= lw <= LINEWIDTHS[1]:
        raise ValueError(f"limb_width={limb_width!r}: a number in {list(LINEWIDTHS)}")
    try:
        la = float(limb_alpha)
    except (TypeError, ValueError):
        raise ValueError(f"limb_alpha={limb_alpha!r}: a number in [0, 1]") from None
    if not 0.0 <= la <= 1.0:
        raise ValueError(f"limb_alpha={limb_alpha!r}: a number in [0, 1]")
    return lw, la


def _check_skeleton(skeleton, num_joints: int) -> np.ndarray:
    """-> (E, 2) int32, every index in 0 .. P - 1"""
    sk = np.asarray(skeleton)
    if sk.size == 0 and sk.ndim <= 2:
        return np.zeros((0, 2), np.int32)
    if sk.dtype.kind not in "iu":
        raise TypeError(f"skeleton: (E, 2) integer joint indices, got {sk.dtype}")
    if sk.ndim != 2 or sk.shape[1] != 2:
        raise ValueError(f"skeleton: (E, 2) integer joint indices, got {sk.shape}")
    P = int(num_joints)
    for e, (a, b) in enumerate(sk.tolist()):
        if not (0 <= a < P and 0 <= b < P):
            raise ValueError(f"skeleton: edge {e} = ({a}, {b}) names a joint outside 0 .. {P - 1}")
    return np.ascontiguousarray(sk, dtype=np.int32)


def _check_limb_colors(limb_colors, skeleton, colors) -> np.ndarray:
    """-> (E, 3) uint8; None: the colour of every edge's second joint"""
    E = skeleton.shape[0]
    if limb_colors is None:
        return np.ascontiguousarray(colors[skeleton[:, 1]], dtype=np.uint8).reshape(E, 3)
    if limb_colors.dtype.kind not in "iu":
        raise TypeError(f"limb_colors: integers in 0 .. 255, got {limb_colors.dtype}")
    if limb_colors.shape != (E, 3):
        raise ValueError(f"limb_colors: {(E, 3)} to go with the skeleton, got {limb_colors.shape}")
    if limb_colors.size and (int(limb_colors.min()) < 0 or int(limb_colors.max()) > 255):
        raise ValueError("limb_colors: integers in 0 .. 255")
    return limb_colors.astype(np.uint8)


def _check_heat_consts(heat_gain, heat_alpha):
    """-> (heat_gain, heat_alpha) as floats"""
    try:
        gain = float(heat_gain)
    except (TypeError, ValueError):
        raise ValueError(f"heat_gain={heat_gain!r}: a finite number > 0") from None
    if not (np.isfinite(gain) and gain > 0.0):
        raise ValueError(f"heat_gain={heat_gain!r}: a finite number > 0")
    try:
        ha = float(heat_alpha)
    except (TypeError, ValueError):
        raise ValueError(f"heat_alpha={heat_alpha!r}: a number in [0, 1]") from None
    if not 0.0 <= ha <= 1.0:
        raise ValueError(f"heat_alpha={heat_alpha!r}: a number in [0, 1]")
    return gain, ha


def _check_heat_shape(shape, dtype_name: str, frames_shape):
    """heat's shape and type against the frames' (T, H, W, 3); -> K"""
    T, H, W = (int(v) for v in frames_shape[:3])
    if dtype_name not in ("float32", "float64"):
        raise TypeError(f"heat: expected float32 or float64, got {dtype_name}")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 4 or (shape[0], shape[2], shape[3]) != (T, H, W):
        raise ValueError(f"heat: ({T}, K, {H}, {W}) to go with the frames, got {shape}")
    if not 1 <= shape[1] <= MAX_HEAT_MAPS:
        raise ValueError(f"heat: K={shape[1]} maps (1 .. {MAX_HEAT_MAPS})")
    return shape[1]


def _check_heat_colors(heat_colors, K: int) -> np.ndarray:
    if heat_colors is None:
        return track_colors(K)
    if heat_colors.dtype.kind not in "iu":
        raise TypeError(f"heat_colors: integers in 0 .. 255, got {heat_colors.dtype}")
    if heat_colors.shape != (K, 3):
        raise ValueError(f"heat_colors: {(K, 3)} to go with the maps, got {heat_colors.shape}")
    if heat_colors.size and (int(heat_colors.min()) < 0 or int(heat_colors.max()) > 255):
        raise ValueError("heat_colors: integers in 0 .. 255")
    return heat_colors.astype(np.uint8)


def _int_in(value, lo: int, hi: int, name: str) -> int:
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, np.integer)) or not lo <= int(value) <= hi:
        raise ValueError(f"{name}={value!r}: an integer in {lo} .. {hi}")
    return int(value)


def _check_boxes(frames_shape, boxes, box_visibles, box_colors, box_width, box_alpha, box_labels, label_scale, palette):
    """-> (boxes (T, N, 4) int32, visibles (T, N) bool | None, colors (N, 3) uint8, box_width, box_alpha, labels (N,) int32 | None,
    label_scale); every refusal names its argument"""
    T = int(frames_shape[0])
    b = np.asarray(boxes)
    if b.dtype.kind not in "iu":
        raise TypeError(f"boxes: ({T}, N, 4) integers (x0, y0, x1, y1), got {b.dtype}")
    if b.ndim != 3 or b.shape[0] != T or b.shape[2] != 4:
        raise ValueError(f"boxes: ({T}, N, 4) to go with the frames, got {b.shape}")
    N = b.shape[1]
    if N > MAX_BOXES:
        raise ValueError(f"boxes: N={N} boxes a frame (0 .. {MAX_BOXES})")
    if b.size and int(np.abs(b.astype(np.int64)).max()) >= BOX_LIMIT:
        raise ValueError(f"boxes: coordinates below 2**20 in magnitude, got {int(np.abs(b.astype(np.int64)).max())}")
    vis = None
    if box_visibles is not None:
        vis = np.asarray(box_visibles)
        if vis.dtype != np.bool_:
            raise TypeError(f"box_visibles: expected bool, got {vis.dtype}")
        if vis.shape != (T, N):
            raise ValueError(f"box_visibles: {(T, N)} to go with the boxes, got {vis.shape}")
    if box_colors is None:
        pal = _davis_palette() if palette is None else np.asarray(palette)
        if pal.dtype != np.uint8 or pal.shape != (256, 3):
            raise ValueError(f"palette: (256, 3) uint8 (box_colors=None takes palette[i]), got {pal.dtype} {pal.shape}")
        col = pal[:N]
    else:
        col = np.asarray(box_colors)
        if col.dtype.kind not in "iu":
            raise TypeError(f"box_colors: integers in 0 .. 255, got {col.dtype}")
        if col.shape != (N, 3):
            raise ValueError(f"box_colors: {(N, 3)} to go with the boxes, got {col.shape}")
        if col.size and (int(col.min()) < 0 or int(col.max()) > 255):
            raise ValueError("box_colors: integers in 0 .. 255")
    bw = _int_in(box_width, BOX_WIDTHS[0], BOX_WIDTHS[1], "box_width")
    alpha = _int_in(box_alpha, 0, 256, "box_alpha")
    scale = _int_in(label_scale, LABEL_SCALES[0], LABEL_SCALES[1], "label_scale")
    labels = None
    if box_labels is not None:
        labels = np.asarray(box_labels)
        if labels.size == 0:
            labels = labels.astype(np.int32)                                            # (an empty list has no integer type of its own)
        if labels.dtype.kind not in "iu" or labels.shape != (N,):
            raise ValueError(f"box_labels: {N} integers in 0 .. {MAX_LABEL}, got {labels.dtype} {labels.shape}")
        if labels.size and (int(labels.min()) < 0 or int(labels.max()) > MAX_LABEL):
            raise ValueError(f"box_labels: integers in 0 .. {MAX_LABEL}")
        labels = np.ascontiguousarray(labels, dtype=np.int32)
    return np.ascontiguousarray(b, dtype=np.int32), vis, np.ascontiguousarray(col, dtype=np.uint8), bw, alpha, labels, scale


def _backend(backend: str) -> bool:
    """True for 'hip' (after its refusal), False for 'host'."""
    if backend not in BACKENDS:
        raise ValueError(f"backend={backend!r}: one of {BACKENDS}")
    if backend == "host":
        return False
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("backend='hip' needs a GPU (fgvc_render_frames_u8 has no CPU path); use backend='host'")
    return True


# ---- the host backend: the contract -------------------------------------------------------------------------------------------------------
def _overlay_host(frames, ids, palette, alpha, contour):
    inside = ids > 0
    colour = palette[ids]                                                            # (T, H, W, 3)
    blend = ((frames.astype(np.int64) * (256 - alpha) + colour.astype(np.int64) * alpha + 128) >> 8).astype(np.uint8)
    out = np.where(inside[..., None], blend, frames)
    if contour:
        edge = np.zeros(ids.shape, bool)
        dx, dy = ids[:, :, 1:] != ids[:, :, :-1], ids[:, 1:, :] != ids[:, :-1, :]
        edge[:, :, 1:] |= dx
        edge[:, :, :-1] |= dx
        edge[:, 1:, :] |= dy
        edge[:, :-1, :] |= dy
        out = np.where((edge & inside)[..., None], colour, out)
    return out


def _paint_host(video, tracks, visibles, colors, radius):
    """Paints into `video` (T, H, W, 3) uint8.  Per point the reference's own patch expression, on the part of the patch inside the image
    (the reference pads the image by r + 1, scatters, and cuts the pad off: the same pixels get the same values)."""
    T, H, W = video.shape[:3]
    r, d = radius, 2 * radius + 1
    z = np.zeros((d + 2, d + 2, 1), np.float64)
    z[1:d + 1, 1:d + 1, 0] = icon_table(r)
    icon1, icon2, icon3, icon4 = z[1:, 1:], z[:-1, 1:], z[1:, :-1], z[:-1, :-1]      # I(a, b), I(a - 1, b), I(a, b - 1), I(a - 1, b - 1)
    cols = colors.astype(np.int64)
    for t in range(T):
        image = video[t]
        for i in range(tracks.shape[0]):
            if not visibles[i, t] or not np.isfinite(tracks[i, t]).all():
                continue
            x, y = tracks[i, t, :] + 0.5
            x = min(max(x, 0.0), W)
            y = min(max(y, 0.0), H)
            x1, y1 = np.floor(x).astype(np.int32), np.floor(y).astype(np.int32)
            x2, y2 = x1 + 1, y1 + 1
            patch = (icon1 * (x2 - x) * (y2 - y) + icon2 * (x2 - x) * (y - y1) + icon3 * (x - x1) * (y2 - y) + icon4 * (x - x1) * (y - y1))
            a0, a1 = max(0, r + 1 - int(y1)), min(d + 1, H + r + 1 - int(y1))        # rows a of the patch inside the image
            b0, b1 = max(0, r + 1 - int(x1)), min(d + 1, W + r + 1 - int(x1))
            if a0 >= a1 or b0 >= b1:
                continue
            ys, xs = slice(a0 + int(y1) - r - 1, a1 + int(y1) - r - 1), slice(b0 + int(x1) - r - 1, b1 + int(x1) - r - 1)
            p = patch[a0:a1, b0:b1]
            image[ys, xs] = ((1 - p) * image[ys, xs] + p * cols[i][np.newaxis, np.newaxis, :]).astype(np.uint8)
    return video


def _segment_host(image, ax, ay, bx, by, ro2, g, reach, factor, colour):
    """One anti-aliased segment from (ax, ay) to (bx, by) (the + 0.5 already in) into image (H, W, 3) uint8, of opacity cov * factor: the
    module text's rule on the part of the segment's box (grown by ceil(ro): outside it cov is exactly 0) inside the image.  What the trails
    and the limbs share."""
    H, W = image.shape[:2]
    x_lo, x_hi = max(int(np.floor(min(ax, bx))) - reach, 0), min(int(np.ceil(max(ax, bx))) + reach, W - 1)
    y_lo, y_hi = max(int(np.floor(min(ay, by))) - reach, 0), min(int(np.ceil(max(ay, by))) + reach, H - 1)
    if x_lo > x_hi or y_lo > y_hi:
        return
    px = np.arange(x_lo, x_hi + 1, dtype=np.float64)[np.newaxis, :]
    py = np.arange(y_lo, y_hi + 1, dtype=np.float64)[:, np.newaxis]
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    u = 0.0 if L2 == 0 else np.minimum(np.maximum(((px - ax) * dx + (py - ay) * dy) / L2, 0.0), 1.0)
    ex, ey = px - (ax + u * dx), py - (ay + u * dy)
    d2 = ex * ex + ey * ey
    cov = np.minimum(np.maximum((ro2 - d2) * g, 0.0), 1.0)
    op = (cov * factor)[:, :, np.newaxis]
    col = colour.astype(np.float64)[np.newaxis, np.newaxis, :]
    ys, xs = slice(y_lo, y_hi + 1), slice(x_lo, x_hi + 1)
    image[ys, xs] = ((1 - op) * image[ys, xs] + op * col).astype(np.uint8)


def _trails_host(video, t, tracks, visibles, colors, L, ro2, g, reach, fade, time_colors):
    """Frame t's trails into video[t] (H, W, 3) uint8: a segment at a time, in point order, oldest step first."""
    image = video[t]
    s0 = max(0, t - L)
    if s0 >= t or tracks.shape[0] == 0:
        return
    with np.errstate(invalid="ignore"):
        ok = visibles[:, s0:t + 1] & (np.abs(tracks[:, s0:t + 1]) < TRAIL_LIMIT).all(-1)
    for i, k in np.argwhere(ok[:, :-1] & ok[:, 1:]):                                   # in point order, oldest step first
        s = s0 + int(k)
        ax, ay = tracks[i, s] + 0.5
        bx, by = tracks[i, s + 1] + 0.5
        _segment_host(image, ax, ay, bx, by, ro2, g, reach, fade[t - 1 - s], time_colors[s] if time_colors is not None else colors[i])


def _limbs_host(video, t, tracks, visibles, skeleton, limb_colors, ro2, g, reach, limb_alpha):
    """Frame t's limbs into video[t] (H, W, 3) uint8: an edge at a time, in edge order."""
    if skeleton.shape[0] == 0:
        return
    with np.errstate(invalid="ignore"):
        ok = visibles[:, t] & (np.abs(tracks[:, t]) < TRAIL_LIMIT).all(-1)
    for e, (a, b) in enumerate(skeleton.tolist()):
        if ok[a] and ok[b]:
            ax, ay = tracks[a, t] + 0.5
            bx, by = tracks[b, t] + 0.5
            _segment_host(video[t], ax, ay, bx, by, ro2, g, reach, limb_alpha, limb_colors[e])


def _blend_rect(image, xa, ya, xb, yb, colour, alpha):
    """The overlay's blend of `colour` into the part of [xa, xb) x [ya, yb) inside image (H, W, 3) uint8."""
    H, W = image.shape[:2]
    xa, ya, xb, yb = max(xa, 0), max(ya, 0), min(xb, W), min(yb, H)
    if xa >= xb or ya >= yb:
        return
    region = image[ya:yb, xa:xb].astype(np.int64)
    image[ya:yb, xa:xb] = ((region * (256 - alpha) + colour.astype(np.int64) * alpha + 128) >> 8).astype(np.uint8)


def _boxes_host(video, boxes, visibles, colors, bw, alpha, labels, scale):
    """The boxes into video (T, H, W, 3) uint8, frame by frame, box by box in index order: ring, tag, digits (the module text's rule)."""
    T, H, W = video.shape[:3]
    for t in range(T):
        image = video[t]
        for i in range(boxes.shape[1]):
            x0, y0, x1, y1 = (int(v) for v in boxes[t, i])
            if x1 <= x0 or y1 <= y0 or (visibles is not None and not visibles[t, i]):
                continue
            col = colors[i]
            # the ring as four bars: above, below, left and right of the box
            _blend_rect(image, x0 - bw, y0 - bw, x1 + bw, y0, col, alpha)
            _blend_rect(image, x0 - bw, y1, x1 + bw, y1 + bw, col, alpha)
            _blend_rect(image, x0 - bw, y0, x0, y1, col, alpha)
            _blend_rect(image, x1, y0, x1 + bw, y1, col, alpha)
            if labels is None:
                continue
            text = str(int(labels[i]))
            tw, th = (6 * len(text) + 1) * scale, 9 * scale
            ty = y0 - bw - th
            if ty < 0:
                ty = y0
            tx = x0 - bw
            if tx + tw > W:
                tx = max(W - tw, 0)
            _blend_rect(image, tx, ty, tx + tw, ty + th, col, alpha)
            ink = 255 if 299 * int(col[0]) + 587 * int(col[1]) + 114 * int(col[2]) < 128000 else 0
            for g, ch in enumerate(text):
                for r in range(7):
                    bits = int(DIGITS_5X7[int(ch), r])
                    for c in range(5):
                        if (bits >> (4 - c)) & 1:
                            xa, ya = tx + (1 + 6 * g + c) * scale, ty + (1 + r) * scale
                            image[max(ya, 0):max(min(ya + scale, H), 0), max(xa, 0):max(min(xa + scale, W), 0)] = ink


def _heat_host(video, heat, heat_colors, gain, heat_alpha):
    """The maps heat (T, K, H, W) into video (T, H, W, 3) uint8, map after map (the module text's rule)."""
    cols = heat_colors.astype(np.float64)
    for t in range(video.shape[0]):
        image = video[t]
        for k in range(heat.shape[1]):
            with np.errstate(invalid="ignore", over="ignore"):
                a = np.minimum(np.maximum(heat[t, k].astype(np.float64) * gain, 0.0), 1.0) * heat_alpha
                m = a > 0                                                                # False for NaN
            if not m.any():
                continue
            am = a[m][:, np.newaxis]
            image[m] = ((1 - am) * image[m] + am * cols[k][np.newaxis, :]).astype(np.uint8)


# ---- the public functions -----------------------------------------------------------------------------------------------------------------
def render(frames, ids=None, tracks=None, visibles=None, colors=None, palette=None, alpha: int = 128, contour: bool = True,
           radius: Optional[int] = None, backend: str = "host", *, trail: Optional[int] = None, linewidth: float = 2.0, trail_fade=None,
           trail_color_by: str = "track", skeleton=None, limb_colors=None, limb_width: float = 2.0, limb_alpha: float = 1.0, heat=None,
           heat_colors=None, heat_gain: float = 1.0, heat_alpha: float = 0.5, boxes=None, box_visibles=None, box_colors=None,
           box_width: int = 2, box_alpha: int = 255, box_labels=None, label_scale: int = 1):
    """Overlay (when `ids` is given), then points (when `tracks` is given) onto frames (T, H, W, 3) uint8; neither: a copy.  ids (T, H, W)
    uint8, palette (256, 3) uint8 (None: davis_palette()), alpha 0 .. 256; tracks (P, T, 2) as (x, y), visibles (P, T) bool (None: all),
    colors (P, 3) integers 0 .. 255 (None: track_colors(P)), radius 1 .. 31 (None: the reference's round(min(H, W) * 0.015)).
    trail=L (1 .. 64, needs tracks; None: no trails): between the overlay and the points, every point's last L steps as line segments
    `linewidth` (1 .. 16) pixels wide, of opacity trail_fade[age] ((L,) in [0, 1]; None: trail_fade(L)), in the point's colour
    (trail_color_by='track') or the step's (='time': spring_colors(T)) -- the module text has the rule.
    heat (T, K, H, W) float32 | float64 (None: no maps): after the overlay, map k blended in with heat_colors[k] ((K, 3) integers 0 .. 255;
    None: track_colors(K)) at opacity clamp(v heat_gain, 0, 1) heat_alpha.  skeleton (E, 2) joint indices (needs tracks; None: no limbs):
    after the heat, edge e as a line `limb_width` (1 .. 16) pixels wide of opacity limb_alpha in limb_colors[e] ((E, 3); None: the colour
    of the edge's second joint).  The stages run overlay, heat, limbs, points; trail= goes with neither (one stage per launch: paint the
    trails first and the pose onto that output).
    boxes (T, N, 4) integers (x0, y0, x1, y1), half-open, N <= 255, coordinates below 2**20 in magnitude (None: no boxes): after the
    overlay and before the points, box i as a ring `box_width` (1 .. 16) pixels wide OUTSIDE the box in box_colors[i] ((N, 3) integers
    0 .. 255; None: palette[i], so pass row o for object o) at opacity box_alpha (0 .. 256, the overlay's formula), skipped where it is
    empty or box_visibles[t, i] ((T, N) bool; None: all) is false; box_labels (N integers 0 .. 999; None: no tags) puts the number on a
    tag above the box, label_scale (1 .. 4) pixels per bitmap pixel -- the module text has the rule.  boxes= goes with neither trail=
    nor skeleton= / heat=: render the boxes in place, then paint_trails.  boxes=None: the renderer as it was.
    backend='hip': numpy arrays or CUDA tensors, one launch; returns a CUDA uint8 tensor when `frames` is one, numpy otherwise."""
    pose = _pose_args(skeleton, limb_colors, limb_width, limb_alpha, heat, heat_colors, heat_gain, heat_alpha, trail, tracks, True)
    bx = _box_args(boxes, box_visibles, box_colors, box_width, box_alpha, box_labels, label_scale, trail, skeleton, heat)
    return _render(frames, ids, tracks, visibles, colors, palette, alpha, contour, radius, backend, trail, linewidth, trail_fade,
                   trail_color_by, True, pose, bx)


def _box_args(boxes, box_visibles, box_colors, box_width, box_alpha, box_labels, label_scale, trail, skeleton, heat):
    """The box stage's arguments as a dict, None without boxes; its refusals by name, before any work."""
    if boxes is None:
        return None
    for name, other in (("trail", trail), ("skeleton", skeleton), ("heat", heat)):
        if other is not None:
            raise ValueError(f"boxes: not together with {name}= (one stage runs per launch: render the boxes first, in place, and paint "
                             f"the {'trails' if name == 'trail' else 'pose'} onto that output)")
    return dict(boxes=boxes, box_visibles=box_visibles, box_colors=box_colors, box_width=box_width, box_alpha=box_alpha,
                box_labels=box_labels, label_scale=label_scale)


def _pose_args(skeleton, limb_colors, limb_width, limb_alpha, heat, heat_colors, heat_gain, heat_alpha, trail, tracks, dots):
    """The pose stage's arguments as a dict, None without skeleton and heat; its refusals by name, before any work."""
    if skeleton is None and heat is None:
        return None
    if trail is not None:
        raise ValueError("trail: not together with skeleton= or heat= (one stage runs per launch: paint the trails first and the pose onto "
                         "that output)")
    if skeleton is not None and tracks is None:
        raise ValueError("skeleton: needs tracks (P, T, 2), got None")
    pose = dict(dots=bool(dots), skeleton=skeleton, limb_colors=limb_colors, heat=heat, heat_colors=heat_colors)
    if skeleton is not None:
        pose["limb_width"], pose["limb_alpha"] = _check_limb_consts(limb_width, limb_alpha)
    if heat is not None:
        pose["heat_gain"], pose["heat_alpha"] = _check_heat_consts(heat_gain, heat_alpha)
    return pose


def _render(frames, ids, tracks, visibles, colors, palette, alpha, contour, radius, backend, trail, linewidth, fade, color_by, dots,
            pose=None, boxes=None):
    hip = _backend(backend)
    on_device = hip and _is_cuda(frames)
    trails = None
    if trail is not None:
        if tracks is None:
            raise ValueError("trail: needs tracks (P, T, 2), got None")
        L, lw, fd = _check_trails(trail, linewidth, fade, color_by)
        trails = dict(L=L, linewidth=lw, fade=fd, by_time=color_by == "time", dots=bool(dots))
    if hip:
        return _render_hip(frames, ids, tracks, visibles, colors, palette, alpha, contour, radius, on_device, trails, pose, boxes)
    f = _numpy(frames)
    _check_frames(f)
    if boxes is not None:
        bx = _check_boxes(f.shape, _numpy(boxes["boxes"]), _numpy(boxes["box_visibles"]), _numpy(boxes["box_colors"]), boxes["box_width"],
                          boxes["box_alpha"], _numpy(boxes["box_labels"]), boxes["label_scale"], _numpy(palette))
    hm = hcol = sk = lcol = pts = None
    with_dots = (trails is None or trails["dots"]) and (pose is None or pose["dots"])
    if ids is not None:
        m = _numpy(ids)
        pal, a = _check_overlay(f, m, _numpy(palette), alpha)
    if tracks is not None:
        pts = tr, vis, col, r = _check_points(f, _numpy(tracks), _numpy(visibles), _numpy(colors), radius if with_dots else 1)
    if pose is not None and pose["heat"] is not None:
        hm = _numpy(pose["heat"])
        hcol = _check_heat_colors(_numpy(pose["heat_colors"]), _check_heat_shape(hm.shape, hm.dtype.name, f.shape))
    if pose is not None and pose["skeleton"] is not None:
        sk = _check_skeleton(_numpy(pose["skeleton"]), tr.shape[0])
        lcol = _check_limb_colors(_numpy(pose["limb_colors"]), sk, col)
    out = f.copy()
    if ids is not None:
        out = _overlay_host(out, m, pal, a, bool(contour))
    out = np.ascontiguousarray(out)
    if boxes is not None:
        _boxes_host(out, *bx)
    if hm is not None:
        _heat_host(out, hm, hcol, pose["heat_gain"], pose["heat_alpha"])
    if sk is not None:
        ro2, g, reach = trail_consts(pose["limb_width"])
        for t in range(f.shape[0]):
            _limbs_host(out, t, tr, vis, sk, lcol, ro2, g, reach, pose["limb_alpha"])
    if pts is not None:
        if trails is not None:
            ro2, g, reach = trail_consts(trails["linewidth"])
            tcol = spring_colors(f.shape[0]) if trails["by_time"] else None
            for t in range(f.shape[0]):
                _trails_host(out, t, tr, vis, col, trails["L"], ro2, g, reach, trails["fade"], tcol)
        if with_dots:
            out = _paint_host(out, tr, vis, col, r)
    return out


def _render_hip(frames, ids, tracks, visibles, colors, palette, alpha, contour, radius, on_device, trails=None, pose=None, boxes=None):
    import torch
    from . import ops
    dev = frames.device if on_device else torch.device("cuda", torch.cuda.current_device())

    def up(x, dtype=None):
        if x is None:
            return None
        if not isinstance(x, torch.Tensor):
            x = torch.from_numpy(np.ascontiguousarray(x))
        x = x.to(dev)
        return x if dtype is None or x.dtype == dtype else x.to(dtype)
    f = up(frames)
    kw = {}
    if ids is not None:
        kw.update(ids=up(ids), palette=up(palette), alpha=alpha, contour=contour)
    if tracks is not None:
        tr = tracks if isinstance(tracks, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(tracks))
        if not (tr.dtype.is_floating_point or tr.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8)):
            raise TypeError(f"point_tracks: a real number type, got {tr.dtype}")
        col = None
        if colors is not None:
            c = _numpy(colors)
            if c.dtype.kind not in "iu":
                raise TypeError(f"colors: integers in 0 .. 255, got {c.dtype}")
            if c.size and (int(c.min()) < 0 or int(c.max()) > 255):
                raise ValueError("colors: integers in 0 .. 255")
            col = up(c.astype(np.uint8))
        kw.update(tracks=up(tr, torch.float64), visibles=up(visibles), colors=col, radius=radius)
    if pose is not None:
        def table(x, name):
            if x is None:
                return None
            c = _numpy(x)
            if c.dtype.kind not in "iu":
                raise TypeError(f"{name}: integers in 0 .. 255, got {c.dtype}")
            if c.size and (int(c.min()) < 0 or int(c.max()) > 255):
                raise ValueError(f"{name}: integers in 0 .. 255")
            return up(c.astype(np.uint8))
        pk = dict(dots=pose["dots"])
        if pose["heat"] is not None:
            h = pose["heat"]
            _check_heat_shape(h.shape, str(h.dtype).replace("torch.", ""), f.shape if f.dim() == 4 else (0, 0, 0))
            pk.update(heat=up(h), heat_colors=table(pose["heat_colors"], "heat_colors"), heat_gain=pose["heat_gain"],
                      heat_alpha=pose["heat_alpha"])
        if pose["skeleton"] is not None:
            pk.update(skeleton=_numpy(pose["skeleton"]), limb_colors=table(pose["limb_colors"], "limb_colors"),
                      limb_width=pose["limb_width"], limb_alpha=pose["limb_alpha"])
        out = ops.render_pose(f, **pk, **kw)
    elif trails is not None:
        tcol = up(spring_colors(f.shape[0])) if trails["by_time"] and f.dim() == 4 else None
        out = ops.render_trails(f, trail=trails["L"], linewidth=trails["linewidth"], fade=up(trails["fade"]), time_colors=tcol,
                                dots=trails["dots"], **kw)
    elif boxes is not None:
        # the boxes are a few integers a frame: checked on the host (a device tensor is read back), then uploaded as the entry takes them
        b, vis, col, bw, a, labels, scale = _check_boxes(f.shape if f.dim() == 4 else (0,), _numpy(boxes["boxes"]), _numpy(boxes["box_visibles"]),
                                                         _numpy(boxes["box_colors"]), boxes["box_width"], boxes["box_alpha"],
                                                         _numpy(boxes["box_labels"]), boxes["label_scale"], _numpy(palette))
        out = ops.render_boxes(f, up(b), None if vis is None else up(vis), up(col), bw, a, None if labels is None else up(labels), scale, **kw)
    else:
        out = ops.render_frames(f, **kw)
    return out if on_device else out.cpu().numpy()


def paint_boxes(frames, boxes, box_visibles=None, box_colors=None, box_width: int = 2, box_alpha: int = 255, box_labels=None,
                label_scale: int = 1, palette=None, backend: str = "host"):
    """frames (T, H, W, 3) uint8 with the boxes (T, N, 4) drawn on as rings with optional id tags (see render and the module text).  With
    tr = engine.ObjectTracks: paint_boxes(frames, tr.boxes, tr.present, box_labels=range(N)) draws every present object's box in its
    palette colour with its number; row 0 is the background's (pass box_visibles with column 0 false to leave it out)."""
    if boxes is None:
        raise ValueError("boxes: (T, N, 4), got None")
    return render(frames, palette=palette, backend=backend, boxes=boxes, box_visibles=box_visibles, box_colors=box_colors,
                  box_width=box_width, box_alpha=box_alpha, box_labels=box_labels, label_scale=label_scale)


def paint_trails(frames, point_tracks, visibles=None, colors=None, trail: int = 8, linewidth: float = 2.0, fade=None, color_by: str = "track",
                 dots: bool = True, radius: Optional[int] = None, backend: str = "host"):
    """frames (T, H, W, 3) uint8 with every point's last `trail` steps drawn as a fading poly-line (see render and the module text) and,
    with dots=True, the dots of paint_point_track on top.  What the reference's second demo video shows (Summ_writer.summ_traj2ds_on_rgbs);
    color_by='time' is its colouring."""
    if point_tracks is None:
        raise ValueError("point_tracks: (P, T, 2), got None")
    if trail is None:
        raise ValueError("trail=None: an integer in 1 .. 64 (paint_point_track draws the dots alone)")
    return _render(frames, None, point_tracks, visibles, colors, None, 128, True, radius, backend, trail, linewidth, fade, color_by, dots)


def paint_pose(frames, joints=None, visibles=None, colors=None, skeleton=None, limb_colors=None, limb_width: float = 2.0,
               limb_alpha: float = 1.0, heat=None, heat_colors=None, heat_gain: float = 1.0, heat_alpha: float = 0.5, dots: bool = True,
               radius: Optional[int] = None, backend: str = "host"):
    """frames (T, H, W, 3) uint8 with a pose drawn on: the joints' heat maps `heat` (T, K, H, W), the limbs of `skeleton` (E, 2) between the
    joints (K, T, 2) (pose_tracks of the pose call's coordinates; pose_visibles for `visibles`) and, with dots=True, the joints' dots on
    top -- see render and the module text.  JHMDB_SKELETON is the JHMDB puppet's; BADJA has no agreed skeleton."""
    if joints is None and heat is None:
        raise ValueError("paint_pose: joints (K, T, 2) or heat (T, K, H, W), got neither")
    if skeleton is None and heat is None:
        skeleton = np.zeros((0, 2), np.int32)                                           # the dots alone, through the same stage
    pose = _pose_args(skeleton, limb_colors, limb_width, limb_alpha, heat, heat_colors, heat_gain, heat_alpha, None, joints, dots)
    return _render(frames, None, joints, visibles, colors, None, 128, True, radius, backend, None, 2.0, None, "track", dots, pose)


def pose_tracks(coords) -> np.ndarray:
    """The pose call's coordinates (2, K, T) (x row, then y row) -> (K, T, 2) float64 as (x, y): what the painters take as tracks."""
    c = np.asarray(_numpy(coords), dtype=np.float64)
    if c.ndim != 3 or c.shape[0] != 2:
        raise ValueError(f"coords: (2, K, T), got {c.shape}")
    return np.ascontiguousarray(np.moveaxis(c, 0, -1))


def pose_visibles(coords, peak=None, min_conf: Optional[float] = None) -> np.ndarray:
    """(K, T) bool from the pose call's coordinates (2, K, T): a joint is visible when its coordinate is finite, is not the reference's
    (-1, -1) of an empty map and, when both `peak` (K, T) (last_pose['peak']) and `min_conf` are given, peak >= min_conf."""
    c = np.asarray(_numpy(coords), dtype=np.float64)
    if c.ndim != 3 or c.shape[0] != 2:
        raise ValueError(f"coords: (2, K, T), got {c.shape}")
    vis = np.isfinite(c).all(0) & ~((c[0] == -1.0) & (c[1] == -1.0))
    if peak is not None and min_conf is not None:
        p = np.asarray(_numpy(peak), dtype=np.float64)
        if p.shape != vis.shape:
            raise ValueError(f"peak: {vis.shape} to go with the coordinates, got {p.shape}")
        with np.errstate(invalid="ignore"):
            vis &= p >= float(min_conf)
    return vis


def paint_point_track(frames, point_tracks, visibles, colors=None, radius: Optional[int] = None, backend: str = "host"):
    """The reference's paint_point_track with its argument order and shapes: frames (T, H, W, 3) uint8, point_tracks (P, T, 2), visibles
    (P, T) bool -> the painted video.  Equal to the reference function called with float64 tracks and `colors` as its colour table."""
    if point_tracks is None:
        raise ValueError("point_tracks: (P, T, 2), got None")
    return render(frames, tracks=point_tracks, visibles=visibles, colors=colors, radius=radius, backend=backend)


def overlay_masks(frames, ids, palette=None, alpha: int = 128, contour: bool = True, backend: str = "host"):
    """frames (T, H, W, 3) uint8 with the objects of ids (T, H, W) uint8 blended in (see the module text)."""
    if ids is None:
        raise ValueError("ids: (T, H, W) uint8, got None")
    return render(frames, ids=ids, palette=palette, alpha=alpha, contour=contour, backend=backend)


# ---- dense flow -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flow_wheel() -> np.ndarray:
    """The 55-colour wheel of the Middlebury flow code (Baker et al., "A Database and Evaluation Methodology for Optical Flow"): (55, 3)
    float64 in [0, 1], the six ramps red-yellow 15, yellow-green 6, green-cyan 4, cyan-blue 11, blue-magenta 13, magenta-red 6."""
    ramps = ((15, 0, 1, +1), (6, 1, 0, -1), (4, 1, 2, +1), (11, 2, 1, -1), (13, 2, 0, +1), (6, 0, 2, -1))     # (length, full, ramping, direction)
    wheel, at = np.zeros((55, 3)), 0
    for n, full, ramp, sign in ramps:
        t = np.floor(255.0 * np.arange(n) / n) / 255.0
        wheel[at:at + n, full] = 1.0
        wheel[at:at + n, ramp] = t if sign > 0 else 1.0 - t
        at += n
    return wheel


def flow_to_rgb(flow, max_mag: Optional[float] = None) -> np.ndarray:
    """A flow (2, h, w) or (n, 2, h, w) (channel 0 = x; numpy or a tensor on either device) as colours (h, w, 3) / (n, h, w, 3) uint8:
    hue from the direction on flow_wheel(), saturation from the magnitude over `max_mag` (None: the largest finite magnitude of the call),
    white at zero flow, a darkened colour beyond max_mag, black where the flow is not finite.  Host numpy in float64; there is no device
    backend (the colours are a picture for people, made once per saved frame)."""
    f = np.asarray(flow.detach().cpu() if hasattr(flow, "detach") else flow, np.float64)
    if f.ndim not in (3, 4) or f.shape[-3] != 2:
        raise ValueError(f"flow_to_rgb: a flow of shape (2, h, w) or (n, 2, h, w), got {f.shape}")
    u, v = f[..., 0, :, :], f[..., 1, :, :]
    fin = np.isfinite(u) & np.isfinite(v)
    u, v = np.where(fin, u, 0.0), np.where(fin, v, 0.0)
    mag = np.hypot(u, v)
    if max_mag is None:
        max_mag = float(mag.max()) if mag.size else 0.0
    if not max_mag > 0:
        max_mag = 1.0
    r = mag / max_mag
    wheel = flow_wheel()
    a = (np.arctan2(-v, -u) / np.pi + 1.0) / 2.0 * (len(wheel) - 1)
    k0 = np.floor(a).astype(np.int64)
    k1 = (k0 + 1) % len(wheel)
    t = (a - k0)[..., None]
    col = (1.0 - t) * wheel[k0] + t * wheel[k1]
    rr = r[..., None]
    col = np.where(rr <= 1.0, 1.0 - rr * (1.0 - col), col * 0.75)
    out = np.floor(255.0 * col).astype(np.uint8)
    out[~fin] = 0
    return out


# ---- results as video: RGB bytes -> packed 8-bit YUV 4:2:0 frames ----------------------------------------------------------
def frames_to_yuv420(frames, fmt: str = "i420", matrix: str = "bt601", range: str = "limited", siting: str = "left", backend: str = "host"):
    """frames (T, H, W, 3) uint8 with H and W even -> packed (T, 3 H / 2, W) uint8 frames of `fmt` ('i420', what datasets.write_y4m takes, or
    'nv12'): Y'CbCr by `matrix` ('bt601' | 'bt709') and `range` ('limited' | 'full'), chroma filtered to `siting` ('left' | 'center').
    backend='host': datasets.rgb8_to_yuv420 on the CPU, the contract; numpy in, numpy out (a tensor in, a CPU tensor out).
    backend='hip': one launch of fgvc_frames_rgb8_to_yuv420 (ops.rgb_frames_to_yuv420), the same bytes; returns a CUDA tensor when
    `frames` is one, numpy otherwise."""
    import torch
    from . import datasets
    hip = _backend(backend)
    if fmt not in ("i420", "nv12"):
        raise ValueError(f"fmt={fmt!r}: one of ('i420', 'nv12')")
    is_tensor = isinstance(frames, torch.Tensor)
    f = frames if is_tensor else torch.from_numpy(np.ascontiguousarray(frames))
    if f.dtype != torch.uint8:
        raise TypeError(f"frames: expected uint8, got {f.dtype}")
    if f.dim() != 4 or f.shape[3] != 3:
        raise ValueError(f"frames: (T, H, W, 3), got {tuple(f.shape)}")
    if f.shape[1] % 2 or f.shape[2] % 2 or f.shape[1] == 0 or f.shape[2] == 0:
        raise ValueError(f"frames: {f.shape[1]} x {f.shape[2]} frames have no packed 4:2:0 form (an odd or empty side)")
    if hip:
        from . import ops
        on_device = f.is_cuda
        dev = f.device if on_device else torch.device("cuda", torch.cuda.current_device())
        out = ops.rgb_frames_to_yuv420(f.to(dev), fmt, "thwc", matrix, range, siting)
        return out if on_device else out.cpu().numpy()
    packed = datasets.pack_yuv420(*datasets.rgb8_to_yuv420(f.cpu(), matrix, range, siting), fmt)
    return packed if is_tensor else packed.numpy()


# ---- object crops: the resampling rule --------------------------------------------------------------------------

CROP_BITS = 22                 # the coefficients' fixed point: K = int(0.5 + k 2^22), sums rounded with 2^21 and shifted by 22
CROP_MAX_SIZE = 1024           # output sides: 1 .. 1024
CROP_MAX_TAPS = 256            # the most taps per axis the device entry keeps for one output
CROP_LIMIT = 2 ** 30           # a window coordinate at or beyond it in magnitude: the window is not resampled


def crop_axis_taps(span: int, n: int) -> int:
    """The bound on the taps of one output of an axis with window length `span` and n outputs that the device entry sizes its table by:
    2 ceil(max(span, n) / n) + 2 >= floor(c + fs + 0.5) - floor(c - fs + 0.5) for every centre c, with fs = max(span / n, 1)."""
    return 2 * (-(-max(int(span), int(n)) // int(n))) + 2


def crop_default_taps(frame_size, size) -> int:
    """The default max_taps of ops.object_crops: enough for every window up to twice the frame's side on each axis, at most CROP_MAX_TAPS."""
    (H, W), (S_h, S_w) = frame_size, size
    return min(CROP_MAX_TAPS, max(crop_axis_taps(2 * int(H), S_h), crop_axis_taps(2 * int(W), S_w)))


def crop_window_ok(x0: int, y0: int, x1: int, y1: int, size, max_taps: Optional[int] = None) -> bool:
    """Whether a window is resampled: not empty (x1 > x0 and y1 > y0), every coordinate below CROP_LIMIT in magnitude and, with max_taps,
    crop_axis_taps of both axes within it.  Any other window gives a crop of `fill` and a mask of zeros."""
    if x1 <= x0 or y1 <= y0 or max(abs(x0), abs(y0), abs(x1), abs(y1)) >= CROP_LIMIT:
        return False
    return max_taps is None or (crop_axis_taps(x1 - x0, size[1]) <= max_taps and crop_axis_taps(y1 - y0, size[0]) <= max_taps)


def crop_axis_coefficients(a0: int, a1: int, n: int):
    """One axis of the resampling rule: the integer window [a0, a1) onto n outputs -> (lo (n,) int64, K: a list of n int64 arrays).  Output
    j sums K[j][i] * src[lo[j] + i].  The triangle filter widened by the scale, as Pillow's BILINEAR resize with box= applies it, in
    float64 with every operation rounded, left to right; the taps' sum runs in increasing order and the coefficients are fixed point:
    K = int(0.5 + k 2^22).  lo is a floor, not a truncation (it can be negative), and neither end is clipped to the frame."""
    scale = np.float64(a1 - a0) / np.float64(n)
    fs = max(scale, np.float64(1.0))
    inv = np.float64(1.0) / fs
    center = np.float64(a0) + (np.arange(n, dtype=np.float64) + np.float64(0.5)) * scale
    lo = np.floor(center - fs + np.float64(0.5)).astype(np.int64)
    hi = np.floor(center + fs + np.float64(0.5)).astype(np.int64)
    cnt = hi - lo
    q = np.arange(int(cnt.max()), dtype=np.int64)[None, :]                  # all outputs at once; the loop over the taps stays sequential
    a = np.abs(((lo[:, None] + q).astype(np.float64) - center[:, None] + np.float64(0.5)) * inv)
    v = np.where((a < 1.0) & (q < cnt[:, None]), np.float64(1.0) - a, np.float64(0.0))
    ww = np.zeros(n, np.float64)
    for i in range(v.shape[1]):
        ww = ww + v[:, i]                                                  # (past an output's last tap this adds 0.0: exact)
    with np.errstate(invalid="ignore", divide="ignore"):
        k = np.where(ww[:, None] != 0.0, v / ww[:, None], v)
    K = (np.float64(0.5) + k * np.float64(1 << CROP_BITS)).astype(np.int64)
    return lo, [K[j, :cnt[j]] for j in range(n)]


def _crop_axis_matrix(a0: int, a1: int, n: int):
    """crop_axis_coefficients as a dense (n, span) int64 matrix over the source indices [base, base + span)"""
    los, Ks = crop_axis_coefficients(a0, a1, n)
    base = int(los.min())
    span = max(int(lo) + len(k) for lo, k in zip(los, Ks)) - base
    M = np.zeros((n, max(span, 1)), np.int64)
    for j, (lo, k) in enumerate(zip(los, Ks)):
        M[j, int(lo) - base:int(lo) - base + len(k)] = k
    return base, M


def _clip8_round(x: np.ndarray) -> np.ndarray:
    return np.clip((x + (1 << (CROP_BITS - 1))) >> CROP_BITS, 0, 255)


def crop_windows_host(frames, windows, size, fill=None, ids=None, objects=None, max_taps: Optional[int] = None):
    """The contract of ops.object_crops (fgvc_frames_object_crops_u8), in numpy: frames (T, H, W, 3) uint8 RGB, windows (T, M, 8) int64 as
    metrics.object_windows_host gives them (the frame-space words 4 .. 7 are resampled, the mask-space words 0 .. 3 sample the ids) or
    (T, M, 4) integer windows (x0, y0, x1, y1) of the caller's own (both spaces equal), size = (S_h, S_w) -> crops (T, M, S_h, S_w, 3)
    uint8; with ids (T, h, w) and objects (M ids) also masks (T, M, S_h, S_w) uint8, as a pair.
    Per axis the coefficients are crop_axis_coefficients'; horizontal pass first, then vertical, with a uint8 intermediate:
        tmp = clip8((2^21 + sum_i Kx_i src_i) >> 22),  out = clip8((2^21 + sum_i Ky_i tmp_i) >> 22)
    where src outside the frame is fill[c] ((3,) uint8, default zeros): Pillow's Image.resize((S_w, S_h), BILINEAR, box=window) on a frame
    padded with `fill`.  Masks are sampled at the nearest pixel of the mask-space window in integers: mx = wx0 + ((2 xx + 1) Wp) // (2 S_w),
    my likewise; 255 where (my, mx) is inside the map and ids[t, my, mx] == objects[j], else 0.  A window that is not crop_window_ok(...,
    max_taps) -- empty, beyond CROP_LIMIT or, where max_taps is given, with more taps on an axis -- gives a crop of `fill` and a mask of zeros."""
    f = np.asarray(frames)
    if f.ndim != 4 or f.shape[3] != 3 or f.dtype != np.uint8:
        raise ValueError(f"frames: (T, H, W, 3) uint8, got {f.dtype} {f.shape}")
    win = np.asarray(windows)
    if win.ndim != 3 or win.shape[0] != f.shape[0] or win.shape[2] not in (4, 8) or win.dtype.kind not in "iu":
        raise ValueError(f"windows: ({f.shape[0]}, M, 8) or ({f.shape[0]}, M, 4) integers, got {win.dtype} {win.shape}")
    win = win.astype(np.int64)
    S_h, S_w = (int(s) for s in size)
    if not (1 <= S_h <= CROP_MAX_SIZE and 1 <= S_w <= CROP_MAX_SIZE):
        raise ValueError(f"size={tuple(size)}: S_h and S_w in 1 .. {CROP_MAX_SIZE}")
    fill = np.zeros(3, np.uint8) if fill is None else np.asarray(fill)
    if fill.shape != (3,) or fill.dtype != np.uint8:
        raise ValueError(f"fill: (3,) uint8, got {fill.dtype} {fill.shape}")
    T, H, W, _ = f.shape
    M = win.shape[1]
    if (ids is None) != (objects is None):
        raise ValueError("ids and objects: both or neither")
    if ids is not None:
        ids = np.asarray(ids)
        objects = [int(o) for o in objects]
        if ids.ndim != 3 or ids.shape[0] != T or len(objects) != M:
            raise ValueError(f"ids: ({T}, h, w) with {M} objects, got {ids.shape} and {len(objects)} objects")
    crops = np.empty((T, M, S_h, S_w, 3), np.uint8)
    crops[...] = fill
    masks = None if ids is None else np.zeros((T, M, S_h, S_w), np.uint8)
    fw, mw = win[..., -4:], win[..., :4]
    for t in range(T):
        for j in range(M):
            x0, y0, x1, y1 = fw[t, j].tolist()
            if not crop_window_ok(x0, y0, x1, y1, (S_h, S_w), max_taps):
                continue
            bx, Kx = _crop_axis_matrix(x0, x1, S_w)
            by, Ky = _crop_axis_matrix(y0, y1, S_h)
            src = np.empty((Ky.shape[1], Kx.shape[1], 3), np.int64)
            src[...] = fill
            ya, yb, xa, xb = max(by, 0), min(by + Ky.shape[1], H), max(bx, 0), min(bx + Kx.shape[1], W)
            if ya < yb and xa < xb:
                src[ya - by:yb - by, xa - bx:xb - bx] = f[t, ya:yb, xa:xb]
            tmp = _clip8_round(np.einsum("yxc,ox->yoc", src, Kx))
            crops[t, j] = _clip8_round(np.einsum("py,yoc->poc", Ky, tmp)).astype(np.uint8)
            if masks is not None:
                wx0, wy0, wx1, wy1 = mw[t, j].tolist()
                if wx1 <= wx0 or wy1 <= wy0 or max(abs(wx0), abs(wy0), abs(wx1), abs(wy1)) >= CROP_LIMIT:
                    continue
                mx = wx0 + ((2 * np.arange(S_w, dtype=np.int64) + 1) * (wx1 - wx0)) // (2 * S_w)
                my = wy0 + ((2 * np.arange(S_h, dtype=np.int64) + 1) * (wy1 - wy0)) // (2 * S_h)
                okx, oky = (mx >= 0) & (mx < ids.shape[2]), (my >= 0) & (my < ids.shape[1])
                got = ids[t][np.clip(my, 0, ids.shape[1] - 1)[:, None], np.clip(mx, 0, ids.shape[2] - 1)[None, :]] == objects[j]
                masks[t, j] = np.where(got & oky[:, None] & okx[None, :], 255, 0)
    return crops if masks is None else (crops, masks)


def contact_sheet(crops, valid=None, cols: Optional[int] = None) -> np.ndarray:
    """Tiles crops (T, M, S_h, S_w, 3) uint8 into one (rows S_h, cols S_w, 3) image on the host: the T M crops in (t, j) order, row-major,
    `cols` a row (None: M, so a row is a frame and a column an object).  valid (T, M) bools: a crop whose entry is false is left black."""
    c = _numpy(crops)
    if c.ndim != 5 or c.shape[4] != 3 or c.dtype != np.uint8:
        raise ValueError(f"crops: (T, M, S_h, S_w, 3) uint8, got {c.dtype} {c.shape}")
    T, M, S_h, S_w, _ = c.shape
    n = T * M
    cols = max(M, 1) if cols is None else int(cols)
    if cols < 1:
        raise ValueError(f"cols={cols}: at least 1")
    if valid is not None:
        valid = np.asarray(_numpy(valid)).astype(bool)
        if valid.shape != (T, M):
            raise ValueError(f"valid: {(T, M)} bools, got {valid.shape}")
    rows = -(-n // cols)
    sheet = np.zeros((rows * S_h, cols * S_w, 3), np.uint8)
    flat = c.reshape(n, S_h, S_w, 3)
    for i in range(n):
        if valid is not None and not valid.reshape(-1)[i]:
            continue
        r, q = divmod(i, cols)
        sheet[r * S_h:(r + 1) * S_h, q * S_w:(q + 1) * S_w] = flat[i]
    return sheet
