"""Show a result: point tracks and mask overlays painted onto uint8 RGB video.

    paint_point_track(frames, point_tracks, visibles, colors)    the reference's dot painter (flyingthingsplus/utils/visualize.py:85-155)
    overlay_masks(frames, ids, palette, alpha, contour)          object ids blended in, integer arithmetic, optional contour
    render(frames, ids=..., tracks=..., visibles=...)            overlay, then points
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
Tracks are (x, y) in the pixel frame of `frames` (scale_tracks for tracks predicted at another size) and are converted to float64 first.
"""
from __future__ import annotations

import colorsys
import functools
from typing import Optional, Tuple

import numpy as np

BACKENDS = ("host", "hip")
MAX_RADIUS = 31
DOT_FRACTION = 0.015          # the reference's dot_size_as_fraction_of_min_edge
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


# ---- the public functions -----------------------------------------------------------------------------------------------------------------
def render(frames, ids=None, tracks=None, visibles=None, colors=None, palette=None, alpha: int = 128, contour: bool = True,
           radius: Optional[int] = None, backend: str = "host"):
    """Overlay (when `ids` is given), then points (when `tracks` is given) onto frames (T, H, W, 3) uint8; neither: a copy.  ids (T, H, W)
    uint8, palette (256, 3) uint8 (None: davis_palette()), alpha 0 .. 256; tracks (P, T, 2) as (x, y), visibles (P, T) bool (None: all),
    colors (P, 3) integers 0 .. 255 (None: track_colors(P)), radius 1 .. 31 (None: the reference's round(min(H, W) * 0.015)).
    backend='hip': numpy arrays or CUDA tensors, one launch; returns a CUDA uint8 tensor when `frames` is one, numpy otherwise."""
    hip = _backend(backend)
    on_device = hip and _is_cuda(frames)
    if hip:
        return _render_hip(frames, ids, tracks, visibles, colors, palette, alpha, contour, radius, on_device)
    f = _numpy(frames)
    _check_frames(f)
    out = f.copy()
    if ids is not None:
        m = _numpy(ids)
        pal, a = _check_overlay(f, m, _numpy(palette), alpha)
        out = _overlay_host(out, m, pal, a, bool(contour))
    if tracks is not None:
        tr, vis, col, r = _check_points(f, _numpy(tracks), _numpy(visibles), _numpy(colors), radius)
        out = _paint_host(np.ascontiguousarray(out), tr, vis, col, r)
    return out


def _render_hip(frames, ids, tracks, visibles, colors, palette, alpha, contour, radius, on_device):
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
    out = ops.render_frames(f, **kw)
    return out if on_device else out.cpu().numpy()


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
