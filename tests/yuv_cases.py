"""Shared by tests/test_yuv_host.py and tests/test_gpu_yuv.py: two restatements of the YUV 4:2:0 input contract, the
kernels' cases and the planes they run on.

  * preprocess_f64 / rgb_f64: the whole contract with float64 coefficients, float64 chroma interpolation, float64 decode, float64 resize and
    tests/input_cases.py's float64 Lab -- what the Lab kernel's error is measured against;
  * rgb8_f32: numpy float32, decode -> bytes in the stated operation order (one rounded operation after another, nothing fused) -- what the
    bytes kernel must equal, bit for bit.

Planes come straight from input_cases.texture_u8 bytes (Y from one channel, subsampled U and V from the others): no encoder."""
import numpy as np
import torch

from tests import input_cases as IC

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = {"limited": (16.0, 255.0 / 219.0, 255.0 / 224.0), "full": (0.0, 1.0, 1.0)}
SITINGS = ("left", "center")
FORMATS = ("nv12", "i420")
ERROR_FLOOR = IC.ERROR_FLOOR


def coefficients_f64(matrix, rng):
    """(y_off, cy, crv, cgu, cgv, cbu) in float64 from Kr, Kb and the range's scales."""
    kr, kb = MATRICES[matrix]
    kg = 1.0 - kr - kb
    y_off, cy, sc = RANGES[rng]
    return y_off, cy, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) / kg * sc, -2 * kr * (1 - kr) / kg * sc, 2 * (1 - kb) * sc


def _taps(n_luma, n, back):
    """Per luma index of one axis: chroma samples i0, i1 and i1's weight (numpy float64; the values are quarters, exact in any format)."""
    s = np.clip(np.arange(n_luma, dtype=np.float64) / 2 - (0.25 if back else 0.0), 0, n - 1)
    i0 = np.floor(s).astype(np.int64)
    return i0, np.minimum(i0 + 1, n - 1), s - i0


def chroma_at_luma(c, h0, w0, siting, dtype):
    """(T, ch, cw) uint8 array -> (T, h0, w0) `dtype`: bilinear, edge clamped."""
    c = np.asarray(c).astype(dtype)
    y0, y1, ly = _taps(h0, c.shape[1], True)
    x0, x1, lx = _taps(w0, c.shape[2], siting == "center")
    ly, lx = ly.astype(dtype)[:, None], lx.astype(dtype)
    one = dtype(1)
    r0, r1 = c[:, y0], c[:, y1]
    top = (one - lx) * r0[:, :, x0] + lx * r0[:, :, x1]
    bot = (one - lx) * r1[:, :, x0] + lx * r1[:, :, x1]
    return (one - ly) * top + ly * bot


def rgb_f64(y, u, v, matrix="bt601", rng="limited", siting="left"):
    """-> (T, 3, h0, w0) float64 R'G'B', 0..255 scale, unclamped."""
    y_off, cy, crv, cgu, cgv, cbu = coefficients_f64(matrix, rng)
    h0, w0 = y.shape[1:]
    yy = cy * (np.asarray(y).astype(np.float64) - y_off)
    cb = chroma_at_luma(u, h0, w0, siting, np.float64) - 128.0
    cr = chroma_at_luma(v, h0, w0, siting, np.float64) - 128.0
    return np.stack([yy + crv * cr, yy + cgu * cb + cgv * cr, yy + cbu * cb], 1)


def rgb8_f64(y, u, v, matrix="bt601", rng="limited", siting="left"):
    """-> (T, h0, w0, 3) uint8 through float64 (the guard's other side)."""
    return np.rint(np.clip(rgb_f64(y, u, v, matrix, rng, siting), 0, 255)).astype(np.uint8).transpose(0, 2, 3, 1)


def rgb_f32(y, u, v, matrix="bt601", rng="limited", siting="left"):
    """-> (T, h0, w0, 3) float32, unclamped: the coefficients rounded to float32 once, then float32 operation by operation in the
    contract's order: yy = cy (Y - y_off); R = yy + crv cr; G = (yy + cgu cb) + cgv cr; B = yy + cbu cb."""
    f = np.float32
    y_off, cy, crv, cgu, cgv, cbu = (f(c) for c in coefficients_f64(matrix, rng))
    h0, w0 = y.shape[1:]
    yy = cy * (np.asarray(y).astype(f) - y_off)
    cb = chroma_at_luma(u, h0, w0, siting, f) - f(128)
    cr = chroma_at_luma(v, h0, w0, siting, f) - f(128)
    rgb = np.stack([yy + crv * cr, (yy + cgu * cb) + cgv * cr, yy + cbu * cb], -1)
    assert rgb.dtype == f
    return rgb


def rgb8_f32(y, u, v, matrix="bt601", rng="limited", siting="left"):
    """-> (T, h0, w0, 3) uint8: rint (half to even) of rgb_f32 clamped to [0, 255]."""
    f = np.float32
    return np.rint(np.clip(rgb_f32(y, u, v, matrix, rng, siting), f(0), f(255))).astype(np.uint8)


def preprocess_f64(y, u, v, size=None, matrix="bt601", rng="limited", siting="left"):
    """The whole contract in float64 on the CPU -> (T, 3, h, w) float64 tensor."""
    x = torch.from_numpy(rgb_f64(y, u, v, matrix, rng, siting))
    if size is not None and tuple(x.shape[-2:]) != tuple(size):
        x = torch.nn.functional.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)
    lab = IC.rgb_to_lab_f64((x / 255.0).clamp(0, 1))
    mean = torch.tensor([50.0, 0.0, 0.0], dtype=torch.float64).view(1, 3, 1, 1)
    std = torch.tensor([50.0, 127.0, 127.0], dtype=torch.float64).view(1, 3, 1, 1)
    return (lab - mean) / std


# ---- planes ---------------------------------------------------------------------------------------------------------------------------------
def texture_planes(T, h0, w0, seed):
    """y (T, h0, w0), u, v (T, (h0 + 1) // 2, (w0 + 1) // 2) uint8 tensors from one texture: Y its first channel, U and V the other two at
    every second row and column."""
    t = IC.texture_u8(T, h0, w0, seed)
    return t[..., 0].contiguous(), t[:, ::2, ::2, 1].contiguous(), t[:, ::2, ::2, 2].contiguous()


def lattice_planes():
    """1 x 128 x 128: the 16-level lattice 0, 17, .., 255 of the whole (Y, Cb, Cr) cube, most of it outside the RGB gamut.  A (Cb, Cr) pair
    holds over a patch of 4 x 4 chroma samples = 8 x 8 luma pixels, inside which the 16 luma levels stand in 2 x 2 blocks: at most the
    patch's first or last row and column blend with the neighbouring patch, so every triple has pixels of pure lattice chroma."""
    lv = torch.arange(16, dtype=torch.uint8) * 17
    u = lv.view(16, 1, 1, 1).expand(16, 4, 16, 4).reshape(1, 64, 64).contiguous()                 # Cb by patch row
    v = lv.view(1, 1, 16, 1).expand(16, 4, 16, 4).reshape(1, 64, 64).contiguous()                 # Cr by patch column
    iy, ix = torch.meshgrid(torch.arange(128), torch.arange(128), indexing="ij")
    y = lv[((iy % 8) // 2) * 4 + (ix % 8) // 2].view(1, 128, 128).contiguous()
    return y, u, v


def tie_planes():
    """2 x 16 x 16, for BT.601 full range: all 256 luma values over constant chroma U = 3 (frame 0) and U = 253 (frame 1), V = 128.  There
    cbu cb = 1.772 * -+125 rounds to exactly -+221.5 in float32, so B = Y -+ 221.5 is an exact tie wherever it is inside [0, 255]: the place
    where half-to-even differs from half-up, and where a fused multiply-add (which keeps the product's rounding error) leaves the tie and
    rounds the other way."""
    y = torch.arange(256, dtype=torch.uint8).view(1, 16, 16).repeat(2, 1, 1)
    u = torch.tensor([3, 253], dtype=torch.uint8).view(2, 1, 1).expand(2, 8, 8).contiguous()
    return y, u, torch.full((2, 8, 8), 128, dtype=torch.uint8)


def in_format(u, v, fmt):
    """The same chroma samples laid out as a decoder would: 'nv12' -- views of one interleaved (T, ch, cw, 2) tensor, pixel stride 2;
    'i420' -- two planes of one buffer, pixel stride 1."""
    if fmt == "nv12":
        uv = torch.stack([u, v], -1).contiguous()
        return uv[..., 0], uv[..., 1]
    both = torch.stack([u, v], 1).contiguous()
    return both[:, 0], both[:, 1]


def pack(y, u, v, fmt):
    """Planes of an even-sized clip -> packed frames (T, 3 h0 / 2, w0): the luma rows, then NV12's interleaved chroma rows or I420's planes."""
    T, h0, w0 = y.shape
    assert h0 % 2 == 0 and w0 % 2 == 0
    if fmt == "nv12":
        c = torch.stack([u, v], -1).reshape(T, h0 // 2, w0)
    else:
        c = torch.stack([u, v], 1).reshape(T, h0 // 2, w0)
    return torch.cat([y, c], 1).contiguous()


def packed_texture(T, h0, w0, seed, fmt):
    return pack(*texture_planes(T, h0, w0, seed), fmt)


# name -> (planes (y, u, v), size (h, w) | None, pad (left, right, top, bottom)): the smallest shapes at which the kernels can go wrong -- odd
# both ways with a width that is no multiple of a lane's 4 columns, one chroma sample, a down- and an up-scale (the edge clamp of luma and
# chroma on all four sides), pads that shift the lane's columns off the frame's
def geometry_cases():
    return {
        "same_2x19x23": (texture_planes(2, 19, 23, 1), None, (0, 0, 0, 0)),
        "one_chroma_2x2": (texture_planes(1, 2, 2, 6), None, (0, 0, 0, 0)),
        "one_pixel_to_3x5": (texture_planes(1, 1, 1, 7), (3, 5), (0, 0, 0, 0)),
        "down_3x37x53_to_24x40": (texture_planes(3, 37, 53, 2), (24, 40), (0, 0, 0, 0)),
        "up_2x18x22_to_41x47": (texture_planes(2, 18, 22, 3), (41, 47), (0, 0, 0, 0)),
        "same_2x16x20_pad": (texture_planes(2, 16, 20, 4), None, (1, 2, 0, 1)),
        "down_2x16x20_to_9x13_pad": (texture_planes(2, 16, 20, 5), (9, 13), (0, 3, 1, 0)),
    }


def kernel_cases():
    """id -> (planes, size, pad, matrix, range, siting, fmt): every geometry in both sitings and both formats (BT.601 limited), the lattice in
    each matrix, range, siting and format, and the rounding ties (tie_planes) in theirs."""
    out = {}
    for name, (planes, size, pad) in geometry_cases().items():
        for siting in SITINGS:
            for fmt in FORMATS:
                out[f"{name}-{siting}-{fmt}"] = (planes, size, pad, "bt601", "limited", siting, fmt)
    for siting in SITINGS:
        for fmt in FORMATS:
            out[f"ties-bt601-full-{siting}-{fmt}"] = (tie_planes(), None, (0, 0, 0, 0), "bt601", "full", siting, fmt)
    lat = lattice_planes()
    for matrix in MATRICES:
        for rng in RANGES:
            for siting in SITINGS:
                for fmt in FORMATS:
                    out[f"lattice-{matrix}-{rng}-{siting}-{fmt}"] = (lat, None, (0, 0, 0, 0), matrix, rng, siting, fmt)
    return out


def np_planes(planes):
    return tuple(p.numpy() for p in planes)
