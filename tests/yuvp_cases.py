"""Shared by tests/test_yuvp_host.py and tests/test_gpu_yuvp.py: two restatements of the input contract for Y'CbCr at 8 to 16 bits, 4:2:0 /
4:2:2 / 4:4:4, written without fgvc_amd.datasets, and the kernels' cases.

  * rgb_f64 / preprocess_f64: float64 coefficients, chroma interpolation, decode, resize and tests/input_cases.py's float64 Lab -- what the
    Lab kernel's error is measured against;
  * rgb8_f32: numpy float32, one rounded operation after another in the contract's order -- what the bytes kernel must equal bit for bit.

Planes are WORDS as a decoder leaves them: the sample sits at `shift`; a high-aligned format carries random low bits, a low-aligned 16-bit one
random bits above its depth -- both restatements mask them off first."""
import numpy as np
import torch

from tests import input_cases as IC

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = ("limited", "full")
SITINGS = ("left", "center")
ERROR_FLOOR = IC.ERROR_FLOOR
# name -> (layout, sub_x, sub_y, depth, shift, numpy dtype): stated here on their own (the host test compares ops.YUV_PIXEL_FORMATS with it)
FORMATS = {
    "p010": ("semi", 2, 2, 10, 6, np.uint16), "p012": ("semi", 2, 2, 12, 4, np.uint16), "p016": ("semi", 2, 2, 16, 0, np.uint16),
    "yuv420p10": ("planar", 2, 2, 10, 0, np.uint16), "yuv420p12": ("planar", 2, 2, 12, 0, np.uint16),
    "yuv422p10": ("planar", 2, 1, 10, 0, np.uint16), "yuv422p12": ("planar", 2, 1, 12, 0, np.uint16),
    "yuv444p10": ("planar", 1, 1, 10, 0, np.uint16), "yuv444p12": ("planar", 1, 1, 12, 0, np.uint16),
    "yuv422p": ("planar", 2, 1, 8, 0, np.uint8), "yuv444p": ("planar", 1, 1, 8, 0, np.uint8),
    "nv16": ("semi", 2, 1, 8, 0, np.uint8),
}
# one per (layout, subsampling, depth) class
KERNEL_FORMATS = ("p010", "yuv420p12", "yuv422p", "yuv422p10", "nv16", "yuv444p", "yuv444p10", "p016")


def fmt_args(fmt):
    """-> dict(depth=, shift=, subsampling=) of a format, as the ops and datasets calls take them."""
    _, sx, sy, depth, shift, _ = FORMATS[fmt]
    return dict(depth=depth, shift=shift, subsampling=(sx, sy))


def coefficients_f64(matrix, rng, depth):
    """(y_off, cy, c_off, crv, cgu, cgv, cbu) in float64 from Kr, Kb, the range and the depth."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    s = 2.0 ** (depth - 8)
    if rng == "limited":
        y_off, cy, c_off, sc = 16 * s, 255.0 / (219 * s), 128 * s, 255.0 / (224 * s)
    else:
        y_off, cy, c_off, sc = 0.0, 255.0 / (2 ** depth - 1), 2.0 ** (depth - 1), 255.0 / (2 ** depth - 1)
    return y_off, cy, c_off, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc


def samples(p, depth, shift):
    """Words -> integer samples (int64)."""
    return (np.asarray(p).astype(np.int64) >> shift) & ((1 << depth) - 1)


def _taps(n_luma, n, sub, back):
    """Per luma index of one axis: chroma samples i0, i1 and i1's weight (float64 quarters); a full-resolution axis: the index itself."""
    if sub == 1:
        i = np.arange(n_luma)
        return i, i, np.zeros(n_luma)
    s = np.clip(np.arange(n_luma, dtype=np.float64) / 2 - (0.25 if back else 0.0), 0, n - 1)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), s - i0


def chroma_at_luma(c, h0, w0, sub, siting, dtype):
    """(T, ch, cw) integer samples -> (T, h0, w0) `dtype`: bilinear and edge clamped on a subsampled axis, the sample itself on a full one."""
    c = np.asarray(c).astype(dtype)
    if sub[0] == 2:
        x0, x1, lx = _taps(w0, c.shape[2], 2, siting == "center")
        lx = lx.astype(dtype)
        c = (dtype(1) - lx) * c[:, :, x0] + lx * c[:, :, x1]
    if sub[1] == 2:
        y0, y1, ly = _taps(h0, c.shape[1], 2, True)
        ly = ly.astype(dtype)[:, None]
        c = (dtype(1) - ly) * c[:, y0] + ly * c[:, y1]
    return c


def _rgb(y, u, v, fmt, matrix, rng, siting, dtype):
    _, sx, sy, depth, shift, _ = FORMATS[fmt]
    y_off, cy, c_off, crv, cgu, cgv, cbu = (dtype(c) for c in coefficients_f64(matrix, rng, depth))
    h0, w0 = y.shape[1:]
    yy = cy * (samples(y, depth, shift).astype(dtype) - y_off)
    cb = chroma_at_luma(samples(u, depth, shift), h0, w0, (sx, sy), siting, dtype) - c_off
    cr = chroma_at_luma(samples(v, depth, shift), h0, w0, (sx, sy), siting, dtype) - c_off
    out = [yy + crv * cr, (yy + cgu * cb) + cgv * cr, yy + cbu * cb]
    assert all(o.dtype == dtype for o in out)
    return out


def rgb_f64(y, u, v, fmt, matrix="bt601", rng="limited", siting="left"):
    """-> (T, 3, h0, w0) float64 R'G'B', 0..255 scale, unclamped."""
    return np.stack(_rgb(y, u, v, fmt, matrix, rng, siting, np.float64), 1)


def rgb_f32(y, u, v, fmt, matrix="bt601", rng="limited", siting="left"):
    """-> (T, h0, w0, 3) float32, unclamped: the coefficients rounded to float32 once, then float32 operation by operation."""
    return np.stack(_rgb(y, u, v, fmt, matrix, rng, siting, np.float32), -1)


def rgb8_f32(y, u, v, fmt, matrix="bt601", rng="limited", siting="left"):
    """-> (T, h0, w0, 3) uint8: rint (half to even) of rgb_f32 clamped to [0, 255]."""
    f = np.float32
    return np.rint(np.clip(rgb_f32(y, u, v, fmt, matrix, rng, siting), f(0), f(255))).astype(np.uint8)


def preprocess_f64(y, u, v, fmt, size=None, matrix="bt601", rng="limited", siting="left"):
    """The whole contract in float64 on the CPU -> (T, 3, h, w) float64 tensor."""
    x = torch.from_numpy(rgb_f64(y, u, v, fmt, matrix, rng, siting))
    if size is not None and tuple(x.shape[-2:]) != tuple(size):
        x = torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    lab = IC.rgb_to_lab_f64((x / 255.0).clamp(0, 1))
    mean = torch.tensor([50.0, 0.0, 0.0], dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor([50.0, 127.0, 127.0], dtype=torch.float64).view(1, 3, 1, 1)
    return (lab - mean) / std


# ---- planes -----------------------------------------------------------------------------------------------------------------------------------
def chroma_shape(fmt, T, h0, w0):
    _, sx, sy = FORMATS[fmt][:3]
    return T, (h0 + sy - 1) // sy, (w0 + sx - 1) // sx


def words(s, fmt, rs):
    """Integer samples -> the format's words: the sample at `shift`, random bits below it (high-aligned) and above the depth (low-aligned)."""
    _, _, _, depth, shift, dt = FORMATS[fmt]
    bits = 8 * np.dtype(dt).itemsize
    w = np.asarray(s).astype(np.int64) << shift
    if shift:
        w |= rs.randint(0, 1 << shift, size=w.shape)
    if depth + shift < bits:
        w |= rs.randint(0, 1 << (bits - depth - shift), size=w.shape) << (depth + shift)
    return w.astype(dt)


def clean_words(s, fmt):
    """Integer samples -> the format's words with every other bit zero."""
    return (np.asarray(s).astype(np.int64) << FORMATS[fmt][4]).astype(FORMATS[fmt][5])


def texture_samples(T, h0, w0, seed, fmt):
    """Integer samples y (T, h0, w0), u, v (chroma_shape): the whole code range -- a smooth ramp over the frame plus noise, so that
    interpolation sees gradients, with 0, 2^depth - 1, the limited-range ends (16 s, 235 s, 240 s) and their outside neighbours planted."""
    depth = FORMATS[fmt][3]
    top = (1 << depth) - 1
    s = 1 << (depth - 8)
    rs = np.random.RandomState(seed)
    special = np.array([0, 1, top, top - 1, 16 * s, 16 * s - 1, 235 * s, 235 * s + 1, 240 * s, 240 * s + 1, 128 * s, 15 * s, 241 * s])

    def plane(shape, phase):
        t, h, w = shape
        ramp = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5 + phase) % 64 / 63.0
        p = np.clip((ramp[None] * top + rs.randint(-top // 8, top // 8 + 1, size=shape) + np.arange(t)[:, None, None] * s), 0, top)
        p = p.astype(np.int64)
        plant = rs.rand(*shape) < 0.15
        p[plant] = special[rs.randint(0, len(special), size=int(plant.sum()))]
        return p
    return plane((T, h0, w0), 0), plane(chroma_shape(fmt, T, h0, w0), 21), plane(chroma_shape(fmt, T, h0, w0), 42)


def texture_planes(T, h0, w0, seed, fmt):
    """-> numpy word planes (y, u, v) of `fmt` with garbage in the unused bits."""
    rs = np.random.RandomState(seed + 1000)
    return tuple(words(p, fmt, rs) for p in texture_samples(T, h0, w0, seed, fmt))


def tie_planes(fmt, matrix="bt601", rng="full"):
    """2 x 16 x 16 luma over constant chroma, V = c_off: the two U codes (searched over a grid of the code range with the float32
    restatement's own arithmetic) under which the most luma codes put B = yy + cbu cb exactly on k + 1/2 inside (0, 255) -- where half-to-even
    differs from half-up and a fused multiply-add leaves the tie; each frame holds those luma codes first, then a ramp.  -> (planes, ties):
    `ties` counts the tie pixels (0 where the format's constants allow none on the grid)."""
    f = np.float32
    depth = FORMATS[fmt][3]
    top = (1 << depth) - 1
    y_off, cy, c_off, _, _, _, cbu = (f(c) for c in coefficients_f64(matrix, rng, depth))
    step = max(1, (top + 1) // 1024)
    codes = np.arange(0, top + 1, step)
    yy = cy * (codes.astype(f) - y_off)
    B = yy[None, :] + (cbu * (codes.astype(f) - c_off))[:, None]               # [U][Y]
    tie = (B > 0) & (B < 255) & (B - np.floor(B) == f(0.5))
    best = np.argsort(-tie.sum(1), kind="stable")[:2]
    ys, us, n = [], [], 0
    for ui in best:
        hit = codes[tie[ui]][:256]
        n += len(hit)
        fill = (np.arange(256 - len(hit)) * (top // 255)) % (top + 1)
        ys.append(np.concatenate([hit, fill]).reshape(16, 16))
        us.append(codes[ui])
    _, ch, cw = chroma_shape(fmt, 2, 16, 16)
    y = np.stack(ys)
    u = np.stack([np.full((ch, cw), c) for c in us])
    v = np.full((2, ch, cw), int(c_off))
    rs = np.random.RandomState(5)
    return tuple(words(p, fmt, rs) for p in (y, u, v)), n


def in_layout(u, v, fmt, dev=None):
    """numpy chroma planes -> torch tensors laid out as the format has them: 'semi' -- views of one interleaved (T, ch, cw, 2) tensor, pixel
    stride 2; 'planar' -- two planes of one buffer, pixel stride 1."""
    semi = FORMATS[fmt][0] == "semi"
    both = torch.from_numpy(np.ascontiguousarray(np.stack([u, v], -1 if semi else 1)))       # (laid out on the host: then one copy)
    if dev is not None:
        both = both.to(dev)
    return (both[..., 0], both[..., 1]) if semi else (both[:, 0], both[:, 1])


def to_torch(planes, fmt, dev=None):
    """numpy (y, u, v) -> torch (y, u, v) in the format's layout, on `dev`."""
    y = torch.from_numpy(np.ascontiguousarray(planes[0]))
    return (y if dev is None else y.to(dev),) + tuple(in_layout(planes[1], planes[2], fmt, dev))


def pack(y, u, v, fmt):
    """Word planes (numpy) of a clip with even sides on the subsampled axes -> packed frames (T, rows, w0) as a torch tensor: the luma rows,
    then a planar format's u plane and v plane or a semi-planar one's rows of interleaved pairs."""
    layout, sx, sy = FORMATS[fmt][:3]
    T, h0, w0 = y.shape
    assert h0 % sy == 0 and w0 % sx == 0
    rows = 2 * h0 // (sx * sy)
    c = np.stack([u, v], -1 if layout == "semi" else 1).reshape(T, rows, w0)
    return torch.from_numpy(np.ascontiguousarray(np.concatenate([y, c], 1)))


# geometry name -> (T, h0, w0, size | None, pad (left, right, top, bottom)): widths 1, 2, 3, 5 and 1023, 1025, 1029 around the 1024 columns a
# workgroup owns, heights 1, 3, 5, 9 around its IN_ROWS = 4 rows, odd on every subsampled axis, the same size and both ways resized, and all
# four pads non-zero
GEOMETRIES = {
    "1x1": (2, 1, 1, None, (0, 0, 0, 0)),
    "3x2_pad": (1, 3, 2, None, (1, 2, 3, 1)),
    "5x3_up_7x9": (1, 5, 3, (7, 9), (0, 0, 0, 0)),
    "9x5_pad": (2, 9, 5, None, (3, 1, 2, 1)),
    "3x1023": (1, 3, 1023, None, (0, 0, 0, 0)),
    "5x1025_pad": (1, 5, 1025, None, (1, 1, 1, 1)),
    "9x1029_down_5x517": (1, 9, 1029, (5, 517), (0, 0, 0, 0)),
    "1x5_up_3x1029": (1, 1, 5, (3, 1029), (2, 1, 1, 2)),
    "19x23_up_41x47_pad": (2, 19, 23, (41, 47), (2, 3, 1, 2)),
    "37x53_down_24x40": (2, 37, 53, (24, 40), (0, 0, 0, 0)),
    "16x20_down_9x13_pad": (2, 16, 20, (9, 13), (1, 3, 1, 2)),
}
SETTINGS = [(m, r, s) for m in MATRICES for r in RANGES for s in SITINGS]


def kernel_cases():
    """id -> (fmt, (T, h0, w0), seed, size, pad, matrix, range, siting): every geometry in every KERNEL_FORMATS format (the settings taken in
    turn, so that each geometry meets both values of matrix, range and siting), 18 x 22 at the same size in every setting and format, and
    'ties' (tie_planes) per format in BT.601 full range."""
    out, k = {}, 0
    for g, (T, h0, w0, size, pad) in GEOMETRIES.items():
        for fmt in KERNEL_FORMATS:
            m, r, s = SETTINGS[k % len(SETTINGS)]
            k += 3                                                           # (3 and 8 are coprime: the formats of one geometry differ in setting)
            out[f"{g}-{fmt}-{m}-{r}-{s}"] = (fmt, (T, h0, w0), k, size, pad, m, r, s)
    for fmt in KERNEL_FORMATS:
        for m, r, s in SETTINGS:
            out[f"17x22-{fmt}-{m}-{r}-{s}"] = (fmt, (2, 17, 22), 7, None, (0, 0, 0, 0), m, r, s)
        for s in SITINGS:
            out[f"ties-{fmt}-bt601-full-{s}"] = (fmt, "ties", 0, None, (0, 0, 0, 0), "bt601", "full", s)
    return out


_PLANES = {}


def case_planes(case):
    """The numpy word planes of a kernel case, made once per (format, shape, seed)."""
    fmt, shape, seed = case[:3]
    key = (fmt, shape, seed)
    if key not in _PLANES:
        _PLANES[key] = tie_planes(fmt)[0] if shape == "ties" else texture_planes(*shape, seed, fmt)
    return _PLANES[key]
