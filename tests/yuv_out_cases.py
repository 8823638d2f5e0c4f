"""Shared by tests/test_yuv_out_host.py and tests/test_gpu_yuv_out.py: restatements of the YUV 4:2:0 output contract,
their deliberate mutations, and the frames the encoder runs on.

  * encode(frames, ..., np.float64): float64 coefficients, the same filters, the direct formulas -- the guard's other side;
  * encode(frames, ..., np.float32): numpy float32 in the stated order, one rounded operation after another -- what
    datasets.rgb8_to_yuv420 and the kernel must equal byte for byte;
  * MUTATIONS: the float32 chain with one thing wrong each, and the case that must catch it.

Frames come from input_cases.texture_u8, from random bytes and from constant colours."""
import numpy as np
import torch

from tests import input_cases as IC

MATRICES = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
RANGES = {"limited": (16.0, 255.0 / 219.0, 255.0 / 224.0), "full": (0.0, 1.0, 1.0)}
SITINGS = ("left", "center")
FORMATS = ("i420", "nv12")
COMBOS = [(m, r, s) for m in MATRICES for r in RANGES for s in SITINGS]
NEAR = 1e-3          # the float32 chain does about 8 rounded operations below 256: 8 x 2^-24 x 256 = 1.2e-4 from the float64 value at the most


def coefficients_f64(matrix, rng):
    """(kr, kg, kb, y_off, sy, cu, cv) in float64 from Kr, Kb and the range's scales."""
    kr, kb = MATRICES[matrix]
    y_off, cy, sc = RANGES[rng]
    return kr, 1.0 - kr - kb, kb, y_off, 1.0 / cy, 1.0 / (2.0 * (1.0 - kb) * sc), 1.0 / (2.0 * (1.0 - kr) * sc)


def chroma_filter(p, siting, dt, mutation=None):
    """(T, h, w) uint8 -> (T, (h + 1) // 2, (w + 1) // 2) `dt`: the two rows 2 j, 2 j + 1 and the columns of `siting`, edges repeated."""
    T, h, w = p.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    p = p.astype(dt)
    if mutation == "clamp_dropped":                                  # what lies past the right / bottom edge is read as 0
        p = np.concatenate([p, np.zeros((T, h, 2), dt)], 2)
        p = np.concatenate([p, np.zeros((T, 2, w + 2), dt)], 1)
        h, w = h + 2, w + 2
    r0 = np.arange(ch) * 2
    r1 = np.minimum(r0 + 1, h - 1)
    c0 = np.arange(cw) * 2
    cp, cm = np.minimum(c0 + 1, w - 1), np.maximum(c0 - 1, 0)
    if mutation == "left_taps_shifted" and siting == "left":
        cm, c0, cp = c0, cp, np.minimum(c0 + 2, w - 1)
    if mutation == "center_for_left":
        siting = "center"
    a, b = p[:, r0], p[:, r1]
    if siting == "center":
        return ((a[:, :, c0] + a[:, :, cp]) + (b[:, :, c0] + b[:, :, cp])) * dt(0.25)
    top = (a[:, :, cm] + dt(2) * a[:, :, c0]) + a[:, :, cp]
    bot = (b[:, :, cm] + dt(2) * b[:, :, c0]) + b[:, :, cp]
    return (top + bot) * dt(0.125)


def _fma32(a, b, c):
    """float32 a * b + c with one rounding (the product of two float32 values is exact in float64)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def encode_values(frames, matrix, rng, siting, dt, mutation=None):
    """frames (T, h, w, 3) uint8 array -> (Y, U, V) arrays of `dt`, neither clamped nor rounded."""
    kr, kg, kb, y_off, sy, cu, cv = (dt(c) for c in coefficients_f64(matrix, rng))

    def lum(r, g, b):
        if mutation == "fused_multiply_add":                         # what a contracting compiler makes of (kr R + kg G) + kb B
            return _fma32(b, kb, _fma32(g, kg, kr * r))
        return (kr * r + kg * g) + kb * b
    R, G, B = (frames[..., c] for c in range(3))
    Y = y_off + sy * lum(R.astype(dt), G.astype(dt), B.astype(dt))
    Rm, Gm, Bm = (chroma_filter(c, siting, dt, mutation) for c in (R, G, B))
    L = lum(Rm, Gm, Bm)
    U, V = dt(128) + cu * (Bm - L), dt(128) + cv * (Rm - L)
    assert Y.dtype == dt and U.dtype == dt and V.dtype == dt
    return (Y, V, U) if mutation == "u_v_swapped" else (Y, U, V)


def to_bytes(x, mutation=None):
    x = np.clip(x, 0, 255)
    return (np.floor(x) if mutation == "truncation" else np.rint(x)).astype(np.uint8)


def encode(frames, matrix="bt601", rng="limited", siting="left", dt=np.float32, mutation=None):
    """-> (y, u, v) uint8 arrays: rint (half to even) of the clamped values."""
    return tuple(to_bytes(x, mutation) for x in encode_values(np.asarray(frames), matrix, rng, siting, dt, mutation))


# ---- frames ---------------------------------------------------------------------------------------------------------------------------------
def texture(T, h, w, seed=0):
    return IC.texture_u8(T, h, w, seed)


def random_bytes(T, h, w, seed=0):
    return torch.from_numpy(np.random.RandomState(1000 + seed).randint(0, 256, (T, h, w, 3)).astype(np.uint8))


def constant_frames(colours, h=4, w=6):
    """One frame of h x w per colour: (n, h, w, 3) uint8."""
    c = torch.as_tensor(np.asarray(colours, np.uint8).reshape(-1, 3))
    return c[:, None, None, :].expand(-1, h, w, 3).contiguous()


CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


def saturated_frames():
    """The cube's corners as constant frames, and one 4 x 16 frame that holds them side by side in 2-column stripes: in full range their chroma
    lands on 128 +- 127.5: clamped at the high end, an exact tie at the low end (0.5), where the float32 chain's own rounding decides the byte
    and the kernel must decide the same.  (A fused lum gives the same floats on these eight colours: luma_ties is the set that catches it.)"""
    stripes = torch.as_tensor(np.asarray(CORNERS, np.uint8))[None, None, :, None, :].expand(1, 4, 8, 2, 3).reshape(1, 4, 16, 3)
    return torch.cat([constant_frames(CORNERS, 4, 16), stripes.contiguous()])


def luma_ties():
    """1 x 64 x 64: colours whose full-range luma is an exact tie in real arithmetic, each a 2 x 2 block (so its chroma sample is its own in
    'center' siting).  BT.601's weights are thousandths: Y = (299 R + 587 G + 114 B) / 1000 ends in .5 where that sum is 500 mod 1000; BT.709's
    are ten-thousandths (2126, 7152, 722; 5000 mod 10000).  The first 512 of each on the lattice 0, 2, .., 254.  There the float32 chain's own
    rounding decides the byte, and a fused multiply-add in lum, which skips one rounding, decides some of them the other way."""
    lv = np.arange(0, 256, 2)
    r, g, b = (x.ravel() for x in np.meshgrid(lv, lv, lv, indexing="ij"))
    rows = []
    for (wr, wg, wb), mod in (((299, 587, 114), 1000), ((2126, 7152, 722), 10000)):
        hit = (wr * r + wg * g + wb * b) % mod == mod // 2
        rows.append(np.stack([r[hit], g[hit], b[hit]], -1)[:512])
    col = np.concatenate(rows).astype(np.uint8)
    assert col.shape == (1024, 3)
    return torch.from_numpy(np.ascontiguousarray(np.kron(col.reshape(32, 32, 3), np.ones((2, 2, 1), np.uint8))[None]))


SIZES = [(1, 1, 1), (3, 2, 2), (3, 3, 5), (1, 6, 10), (3, 34, 66), (1, 65, 131)]          # (T, h, w): the issue's sizes


def frame_sets():
    """name -> frames (T, h, w, 3) uint8 tensor."""
    out = {}
    for i, (T, h, w) in enumerate(SIZES):
        out[f"texture_{T}x{h}x{w}"] = texture(T, h, w, 20 + i)
        out[f"random_{T}x{h}x{w}"] = random_bytes(T, h, w, i)
    out["saturated"] = saturated_frames()
    out["luma_ties"] = luma_ties()
    return out


def is_natural(name):
    """The sets the float64 guard runs on: textures and random bytes (constant colours sit ON the ties by construction)."""
    return name.startswith(("texture_", "random_"))


def cases():
    """id -> (frame set, matrix, range, siting)."""
    return {f"{name}-{m}-{r}-{s}": (name, m, r, s) for name in frame_sets() for (m, r, s) in COMBOS}


# mutation -> the case that must catch it (its bytes differ from the restatement's there)
MUTATIONS = {
    "clamp_dropped": "texture_3x3x5-bt601-limited-center",
    "left_taps_shifted": "texture_1x6x10-bt601-limited-left",
    "center_for_left": "texture_1x6x10-bt601-limited-left",
    "truncation": "texture_3x34x66-bt709-limited-left",
    "u_v_swapped": "texture_3x2x2-bt601-limited-left",
    "fused_multiply_add": "luma_ties-bt601-full-left",
}

# limited range, (R, G, B) -> (Y, U, V): the textbook colour bars
BARS = {
    "bt601": {(255, 0, 0): (81, 90, 240), (0, 0, 255): (41, 240, 110), (255, 255, 0): (210, 16, 146)},
    "bt709": {(255, 0, 0): (63, 102, 240), (0, 255, 0): (173, 42, 26), (0, 0, 255): (32, 240, 118)},
}
for _m in BARS:
    BARS[_m][(255, 255, 255)] = (235, 128, 128)
    BARS[_m][(0, 0, 0)] = (16, 128, 128)
