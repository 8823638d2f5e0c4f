"""Decoders, float64 models, f32 emulations, mutant models and case tables shared by tests/test_gpu_conv_ops.py (the encoder's
convolutions: csrc/conv_split.hip, conv64.hip, conv_s2.hip, stem7.hip) and tests/test_conv_reference_share.py (the same statements on
the CPU, from the models alone).  No GPU code here: numpy on bit patterns and float64 torch convolutions.

Operands.  A convolution reads 128-byte rows, one per (pixel | output channel, 32-channel chunk), in one of four formats
(conv_split.hip's header, common.hpp, the ops.prepare_* docstrings); `act_parts` / `w_parts` decode a row to the values the matrix
instructions are fed, `act_rows` / `w_rows` encode such values back (byte for byte the inverse on every row the packers make):
    bf16x3  [hi 32 bf16 | lo 32 bf16]                               adds  hi.hi + lo.hi + hi.lo
    f16f8   x: [h 32 f16 | l8 32 e4m3 | h8 32 e4m3]                 adds  h.h + 2^(AW-BX) l8_x.h8_w + 2^(AX-BW) h8_x.l8_w   (the instruction's
            w: [h 32 f16 | h8 32 e4m3 | l8 32 e4m3]                       two fixed E8M0 scales per lane half: F8_AX, F8_BX, F8_AW, F8_BW)
    f16x3   [h 32 f16 | l 32 f16]                                   adds  h.h + l.h + h.l
    f16f6   x: [h | l6 main | h6 main | l6 tail, scale | h6 tail, scale]   adds  h.h + l6_x.h6_w + h6_x.l6_w, every FP6 block under the
            w: [h | h6 main | l6 main | h6 tail, scale | l6 tail, scale]         scale byte that travels in its own row
The operand-ordered weight tensors of prepare_conv64 / prepare_conv64_f16 / prepare_conv_s2 / prepare_stem7 are re-ordered copies of
those rows; `unpack_*` bring them back to [tap][chunk][Cout][row] by index arithmetic written from the docstrings, `pack_*` is the
scatter the other way.

model64(case) is the float64 sum of exactly those products, then acc_scale, bias, residual, ReLU; A is the float64 sum of the
absolute values of the same terms (|bias| and |residual| included).  Two kinds of cases:

EXACT cases (tolerance zero, derived).  Operands are planted as bit patterns: small integers for hi / h, independent small integers
times a fixed power of two for lo / l / l8 / l6, h8 / h6 independent of h, integer bias and residual, so every product is a multiple
of one power of two q and A < 2^24 q at every entry.  Every partial sum of any subset of the terms is then a multiple of q below
2^24 q, i.e. an exact f32: whatever the order of additions, the kernel's f32 output equals model64 bit for bit.  Because h8 != e4m3(h)
and lo is independent of hi, a wrong operand, a tap meeting the wrong pixel offset or a channel meeting the wrong channel changes
the sum at some entry.

REALISTIC cases (a bar measured against the model).  emu32 is the same sum accumulated in float32 on the CPU, one addition per matrix
instruction, chunk by chunk, tap by tap, the main k-steps and then the cross terms.  rho(v) = max |v - model64| / (2^-24 A);
the bar is rho(kernel) <= 4 rho(emu32): the factor covers the unknown order inside an instruction and the maximum over the entries.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fgvc_oracle as O
from tests import volume_cases as VC

ARITHS = ["bf16x3", "f16f8", "f16x3", "f16f6"]
FMT = {"bf16x3": 0, "f16f8": 1, "f16x3": 2, "f16f6": 3}
F8_AX, F8_BX, F8_AW, F8_BW = 7, 3, 2, 9                  # common.hpp / ops.py
U24 = 2.0 ** -24
GUARD = 4096                                              # elements of NaN / of the band pattern around every output
BAR_FACTOR = 4.0
OLD_BARS = {"bf16x3": 2e-5, "f16f8": 3e-5, "f16x3": 5e-6, "f16f6": 3e-5}   # tests/test_gpu_parity.py: of the tensor's largest |y|
E4M3 = VC.E4M3
E2M3 = VC.E2M3                                           # code (sign << 5 | e << 3 | m) -> value, 64 entries


def cdiv(a, b):
    return (a + b - 1) // b


def pad_dims(H, W):
    return 8 * cdiv(H, 8) + 2, 32 * cdiv(W, 32) + 8


# ----------------------------------------------------------------------------------------------------------------------
# element codecs
# ----------------------------------------------------------------------------------------------------------------------
def _bf16_dec(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _bf16_enc(v):
    f = np.ascontiguousarray(v, np.float32)
    assert (f.astype(np.float64) == v).all() and (f.view(np.uint32) & 0xFFFF == 0).all(), "not a bf16 value"
    return (f.view(np.uint32) >> 16).astype(np.uint16)


def _f16_dec(u16):
    return np.ascontiguousarray(u16).view(np.float16).astype(np.float64)


def _f16_enc(v):
    h = np.asarray(v).astype(np.float16)
    assert (h.astype(np.float64) == v).all(), "not an f16 value"
    return h.view(np.uint16)


def _e4m3_enc_fast(v):
    """values that ARE e4m3 values (signed zeros kept) -> codes"""
    mags = E4M3[:127]                                      # ascending: code i = magnitude i
    v = np.asarray(v, np.float64)
    i = np.searchsorted(mags, np.abs(v))
    assert (i < 127).all() and (mags[np.minimum(i, 126)] == np.abs(v)).all(), "not an e4m3 value"
    return (i | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def _fp6_unpack(main16, tail8):
    """(n, 16), (n, 8) uint8 -> (n, 32) codes: element e in bits [6 e, 6 e + 6) of the 24-byte little-endian string"""
    by = np.concatenate([main16, tail8], 1).astype(np.uint32).reshape(-1, 8, 3)
    w = by[:, :, 0] | (by[:, :, 1] << 8) | (by[:, :, 2] << 16)
    return np.stack([(w >> (6 * i)) & 63 for i in range(4)], -1).reshape(-1, 32)


def _fp6_pack(codes):
    c = codes.astype(np.uint32).reshape(-1, 8, 4)
    w = c[:, :, 0] | (c[:, :, 1] << 6) | (c[:, :, 2] << 12) | (c[:, :, 3] << 18)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255], -1).reshape(-1, 24).astype(np.uint8)


_E2M3_MAG = E2M3[:32]                                      # ascending magnitudes: code i


def _e2m3_enc(y):
    """values on the e2m3 grid (signed zeros kept) -> codes"""
    y = np.asarray(y, np.float64)
    i = np.searchsorted(_E2M3_MAG, np.abs(y))
    assert (i < 32).all() and (_E2M3_MAG[np.minimum(i, 31)] == np.abs(y)).all(), "not an e2m3 value"
    return (i | np.where(np.signbit(y), 32, 0)).astype(np.uint8)


# ----------------------------------------------------------------------------------------------------------------------
# rows <-> parts.  rows: (..., 128) uint8;  parts: dict of (..., 32) float64 (+ for f16f6 the two scale exponents "sh", "sl": (...,) int,
# the exponent of the block's E8M0 byte, byte = 127 + s)
# ----------------------------------------------------------------------------------------------------------------------
def _rows_u8(t):
    """int16 (..., 64) tensor / array -> (..., 128) uint8 numpy"""
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    a = np.ascontiguousarray(a)
    if a.dtype != np.uint8:
        a = a.view(np.uint8)
    return a.reshape(*a.shape[:-1], 128) if a.shape[-1] != 128 else a


def _parts(rows, fmt, weight):
    rows = _rows_u8(rows)
    lead = rows.shape[:-1]
    r = rows.reshape(-1, 128)
    u16 = r.view(np.uint16)
    if fmt == 0:
        p = {"hi": _bf16_dec(u16[:, :32]), "lo": _bf16_dec(u16[:, 32:])}
    elif fmt == 2:
        p = {"h": _f16_dec(u16[:, :32]), "l": _f16_dec(u16[:, 32:])}
    elif fmt == 1:
        a, b = E4M3[r[:, 64:96]], E4M3[r[:, 96:128]]
        p = {"h": _f16_dec(u16[:, :32]), "h8": a if weight else b, "l8": b if weight else a}
    else:
        blocks = []
        for main, tail in ((64, 96), (80, 112)):           # slots 4 + 6, slots 5 + 7
            codes = _fp6_unpack(r[:, main:main + 16], r[:, tail:tail + 8])
            s = r[:, tail + 8].astype(np.int64) - 127
            blocks.append((E2M3[codes] * np.exp2(s.astype(np.float64))[:, None], s))
        first, second = blocks                            # activations: l6 first;  weights: h6 first
        (h6, sh), (l6, sl) = (first, second) if weight else (second, first)
        p = {"h": _f16_dec(u16[:, :32]), "h6": h6, "l6": l6, "sh": sh.reshape(lead), "sl": sl.reshape(lead)}
    return {k: (v if k in ("sh", "sl") else v.reshape(*lead, 32)) for k, v in p.items()}


def act_parts(rows, fmt):
    return _parts(rows, fmt, False)


def w_parts(rows, fmt):
    return _parts(rows, fmt, True)


def _rows(p, fmt, weight):
    lead = next(v for k, v in p.items() if k not in ("sh", "sl")).shape[:-1]
    n = int(np.prod(lead)) if lead else 1
    r = np.zeros((n, 128), np.uint8)
    u16 = r.view(np.uint16)
    f = lambda k: np.asarray(p[k], np.float64).reshape(n, 32)
    if fmt == 0:
        u16[:, :32], u16[:, 32:] = _bf16_enc(f("hi")), _bf16_enc(f("lo"))
    elif fmt == 2:
        u16[:, :32], u16[:, 32:] = _f16_enc(f("h")), _f16_enc(f("l"))
    elif fmt == 1:
        u16[:, :32] = _f16_enc(f("h"))
        a, b = _e4m3_enc_fast(f("h8")), _e4m3_enc_fast(f("l8"))
        r[:, 64:96], r[:, 96:128] = (a, b) if weight else (b, a)
    else:
        u16[:, :32] = _f16_enc(f("h"))
        sh, sl = np.asarray(p["sh"]).reshape(n), np.asarray(p["sl"]).reshape(n)
        first, second = (("h6", sh), ("l6", sl)) if weight else (("l6", sl), ("h6", sh))
        for (key, s), main, tail in ((first, 64, 96), (second, 80, 112)):
            by = _fp6_pack(_e2m3_enc(f(key) * np.exp2(-s.astype(np.float64))[:, None]))
            r[:, main:main + 16], r[:, tail:tail + 8], r[:, tail + 8] = by[:, :16], by[:, 16:], (s + 127).astype(np.uint8)
    return r.reshape(*lead, 128)


def act_rows(parts, fmt):
    return _rows(parts, fmt, False)


def w_rows(parts, fmt):
    return _rows(parts, fmt, True)


def terms_of(fmt):
    """[(activation part, weight part, weight of the product in accumulator units)] in the kernel's order: main, then the cross terms"""
    if fmt == 0:
        return [("hi", "hi", 1.0), ("lo", "hi", 1.0), ("hi", "lo", 1.0)]
    if fmt == 2:
        return [("h", "h", 1.0), ("l", "h", 1.0), ("h", "l", 1.0)]
    if fmt == 1:
        return [("h", "h", 1.0), ("l8", "h8", 2.0 ** (F8_AW - F8_BX)), ("h8", "l8", 2.0 ** (F8_AX - F8_BW))]
    return [("h", "h", 1.0), ("l6", "h6", 1.0), ("h6", "l6", 1.0)]


# ----------------------------------------------------------------------------------------------------------------------
# host packers (the formats as the kernels' epilogues and ops.prepare_* write them), on f32 values
# ----------------------------------------------------------------------------------------------------------------------
def _e4m3_round(v):
    """f32 array -> e4m3 values (float64), round to nearest even, saturating at 448, the sign of a zero kept"""
    t = torch.from_numpy(np.ascontiguousarray(v, np.float32)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return E4M3[t.view(torch.uint8).numpy()]


def pack_values(y, fmt, scale_log2=0):
    """(..., 32) f32 values of one chunk -> (..., 128) uint8 rows of the ACTIVATION format `fmt` at scale 2^scale_log2: what
    split_bf16_4 / split_f16_4 / split_f16f6_chunk (common.hpp) make of the f32 values of an epilogue"""
    y = np.ascontiguousarray(y, np.float32)
    lead = y.shape[:-1]
    v = y.reshape(-1, 32)
    if fmt == 0:
        return np.ascontiguousarray(VC.split_bf16_model(v).reshape(-1, 64)).view(np.uint8).reshape(*lead, 128)
    if fmt == 3:
        return O.act_f16f6_rows(v, scale_log2).reshape(*lead, 128)
    c = np.clip(v * np.float32(2.0 ** scale_log2), -65504, 65504).astype(np.float32)
    h = c.astype(np.float16)
    l = c - h.astype(np.float32)
    r = np.zeros((v.shape[0], 128), np.uint8)
    r[:, :64] = h.view(np.uint8).reshape(-1, 64)
    if fmt == 2:
        r[:, 64:] = l.astype(np.float16).view(np.uint8).reshape(-1, 64)
    else:
        r[:, 64:96] = _e4m3_enc_fast(_e4m3_round(l * np.float32(2.0 ** F8_BX)))
        r[:, 96:128] = _e4m3_enc_fast(_e4m3_round(h.astype(np.float32) * np.float32(2.0 ** -F8_AX)))
    return r.reshape(*lead, 128)


def padded(rows_nhw, H, W):
    """(N, H, W, nch, 128) uint8 -> the padded split NHWC tensor (N, Hp, Wp, nch, 64) int16 with its zero border"""
    N, _, _, nch, _ = rows_nhw.shape
    Hp, Wp = pad_dims(H, W)
    out = np.zeros((N, Hp, Wp, nch, 128), np.uint8)
    out[:, 1:H + 1, 1:W + 1] = rows_nhw
    return torch.from_numpy(out.view(np.int16).reshape(N, Hp, Wp, nch, 64))


def pack_act(x_nchw, fmt, scale_log2=0):
    """f32 (N, C, H, W) -> padded split NHWC int16 in format `fmt`"""
    N, C, H, W = x_nchw.shape
    v = x_nchw.permute(0, 2, 3, 1).contiguous().float().numpy().reshape(N, H, W, C // 32, 32)
    return padded(pack_values(v, fmt, scale_log2), H, W)


def expected_split(y_nhwc, fmt, scale_log2=0):
    """dense NHWC f32 (N, H, W, C) torch / numpy -> the padded split output a kernel must write for it, border zero"""
    y = y_nhwc.cpu().numpy() if isinstance(y_nhwc, torch.Tensor) else y_nhwc
    N, H, W, C = y.shape
    return padded(pack_values(y.reshape(N, H, W, C // 32, 32), fmt, scale_log2), H, W)


# ----------------------------------------------------------------------------------------------------------------------
# operand-ordered weight layouts, by index arithmetic from the docstrings of ops.prepare_*
# canonical: int16 [T][nch][Cout][64] = 128-byte rows (ops.prepare_conv_split / prepare_conv_split_f16)
# ----------------------------------------------------------------------------------------------------------------------
def _np16(t):
    return np.ascontiguousarray(t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.int16)


def _bf16_operand_index(T, nch, Cout):
    """for every int16 of the canonical bf16 rows [t][c][co][part][k]: (t, c, co // 32, part, s = k >> 4, lane = 32 (k >> 3 & 1) + co % 32, j = k & 7)"""
    t, c, co, part, k = np.meshgrid(np.arange(T), np.arange(nch), np.arange(Cout), np.arange(2), np.arange(32), indexing="ij")
    return t, c, co // 32, part, k >> 4, 32 * ((k >> 3) & 1) + co % 32, k & 7


def pack_conv_s2(canon):
    """-> [T][nch][Cout/32][hi k0-15 | hi k16-31 | lo k0-15 | lo k16-31][lane][8]"""
    a = _np16(canon)
    T, nch, Cout, _ = a.shape
    t, c, ct, part, s, lane, j = _bf16_operand_index(T, nch, Cout)
    out = np.zeros((T, nch, Cout // 32, 4, 64, 8), np.int16)
    out[t, c, ct, 2 * part + s, lane, j] = a.reshape(T, nch, Cout, 2, 32)
    return out


def unpack_conv_s2(w):
    a = _np16(w)
    T, nch, nct = a.shape[:3]
    t, c, ct, part, s, lane, j = _bf16_operand_index(T, nch, nct * 32)
    return a[t, c, ct, 2 * part + s, lane, j].reshape(T, nch, nct * 32, 64)


def pack_conv64(canon):
    """-> [2 output tiles][9 taps][2 chunks][2 k-steps][hi | lo][lane][8]"""
    a = _np16(canon)
    t, c, ct, part, s, lane, j = _bf16_operand_index(9, 2, 64)
    out = np.zeros((2, 9, 2, 2, 2, 64, 8), np.int16)
    out[ct, t, c, s, part, lane, j] = a.reshape(9, 2, 64, 2, 32)
    return out


def unpack_conv64(w):
    a = _np16(w)
    t, c, ct, part, s, lane, j = _bf16_operand_index(9, 2, 64)
    return a[ct, t, c, s, part, lane, j].reshape(9, 2, 64, 64)


def _conv64_f16_index():
    """byte b of the canonical f16f8 row [t][c][co] -> (ct, t, c, byte offset within the (tile, tap, chunk)'s 4 KiB)"""
    t, c, co, b = np.meshgrid(np.arange(9), np.arange(2), np.arange(64), np.arange(128), indexing="ij")
    n, ct = co % 32, co // 32
    # f16 half of the row: byte b < 64 -> k-step s = b // 32, lane half = (b // 16) & 1, 16 bytes per lane
    f16_off = (b // 32) * 1024 + (32 * ((b // 16) & 1) + n) * 16 + (b % 16)
    # fp8 half: b - 64 = 32 which + 16 half + i -> 2048 + lane (= 32 half + n) * 32 + which * 16 + i
    r = b - 64
    x_off = 2048 + (32 * ((r // 16) & 1) + n) * 32 + (r // 32) * 16 + (r % 16)
    return ct, t, c, np.where(b < 64, f16_off, x_off)


def pack_conv64_f16(canon):
    """-> (2, 9, 2, 4096 B): [f16 k-step 0][64 lanes][16 B], [f16 k-step 1][64 lanes][16 B], [64 lanes][h8 16 B | l8 16 B]"""
    a = _np16(canon).view(np.uint8).reshape(9, 2, 64, 128)
    ct, t, c, off = _conv64_f16_index()
    out = np.zeros((2, 9, 2, 4096), np.uint8)
    out[ct, t, c, off] = a
    return out.view(np.int16)


def unpack_conv64_f16(w):
    a = _np16(w).view(np.uint8).reshape(2, 9, 2, 4096)
    ct, t, c, off = _conv64_f16_index()
    return np.ascontiguousarray(a[ct, t, c, off]).view(np.int16).reshape(9, 2, 64, 64)


def _stem7_index():
    """(co, ky, k = 4 kx + ch, part) -> index into [7 ky][2 k-steps][2 output tiles][hi | lo][lane = 32 (k >> 3 & 1) + co % 32][k & 7]"""
    co, ky, k, part = np.meshgrid(np.arange(64), np.arange(7), np.arange(32), np.arange(2), indexing="ij")
    return (co, ky, k, part), (ky, k >> 4, co // 32, part, 32 * ((k >> 3) & 1) + co % 32, k & 7)


def unpack_stem7(w):
    """-> hi, lo float64 (64, 3, 7, 7) and the int16 (64, 7, 32, 2) K blocks (k = 4 kx + c; c = 3 and kx = 7 must be zero)"""
    a = _np16(w)
    (co, ky, k, part), idx = _stem7_index()
    blocks = a[idx]                                       # (64, 7, 32, 2)
    v = _bf16_dec(blocks.view(np.uint16)).reshape(64, 7, 8, 4, 2)
    return v[:, :, :7, :3, 0].transpose(0, 3, 1, 2).copy(), v[:, :, :7, :3, 1].transpose(0, 3, 1, 2).copy(), blocks


def pack_stem7(hi, lo):
    v = np.zeros((64, 7, 8, 4, 2))
    v[:, :, :7, :3, 0], v[:, :, :7, :3, 1] = hi.transpose(0, 2, 3, 1), lo.transpose(0, 2, 3, 1)
    blocks = _bf16_enc(v.reshape(64, 7, 32, 2)).view(np.int16)
    _, idx = _stem7_index()
    out = np.zeros((7, 2, 2, 2, 64, 8), np.int16)
    out[idx] = blocks
    return out


def w_dense(canon, fmt, key):
    """canonical rows [T][nch][Cout][64] -> one part as a float64 conv weight (Cout, Cin, KS, KS)"""
    p = w_parts(_np16(canon), fmt)[key]                   # (T, nch, Cout, 32)
    T, nch, Cout, _ = p.shape
    KS = 3 if T == 9 else 1
    return torch.from_numpy(np.ascontiguousarray(p.transpose(2, 1, 3, 0).reshape(Cout, nch * 32, KS, KS)))


def canon_from_dense(parts, fmt, extra=None):
    """{part: (Cout, Cin, KS, KS) float64} (+ for f16f6 extra = {"sh", "sl": (T, nch, Cout)}) -> canonical int16 rows"""
    any_ = next(iter(parts.values()))
    Cout, Cin, KS, _ = any_.shape
    T, nch = KS * KS, Cin // 32
    p = {k: np.asarray(v).reshape(Cout, nch, 32, T).transpose(3, 1, 0, 2) for k, v in parts.items()}
    if extra:
        p.update(extra)
    return torch.from_numpy(np.ascontiguousarray(w_rows(p, fmt)).view(np.int16).reshape(T, nch, Cout, 64))


def x_dense(x_split, fmt, key):
    """padded split NHWC int16 -> one part as float64 (N, C, Hp, Wp), border included (the kernels read it)"""
    p = act_parts(_np16(x_split), fmt)[key]               # (N, Hp, Wp, nch, 32)
    N, Hp, Wp, nch, _ = p.shape
    return torch.from_numpy(np.ascontiguousarray(p.reshape(N, Hp, Wp, nch * 32).transpose(0, 3, 1, 2)))


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
class Conv:
    """One convolution as the kernel sees it: decoded operand parts, geometry, epilogue.
    xs / ws: lists of ({part: (N, Cin, Hr, Wr)}, {part: (Cout, Cin, KS, KS)}) -- the second entry is the folded projection's input.
    Activations are the region the taps read: padded rows 0 .. H + 1 for 3 x 3 (7 x 7: the frame with 3 zeros around), the interior
    for 1 x 1; `stride` 1 or 2."""

    def __init__(self, fmt, inputs, H, W, stride=1, acc_scale=1.0, bias=None, residual=None, relu=False, name=""):
        self.fmt, self.inputs, self.H, self.W, self.stride = fmt, inputs, H, W, stride
        self.acc_scale, self.bias, self.residual, self.relu, self.name = acc_scale, bias, residual, relu, name

    sums = None

    def copy(self, **kw):
        c = Conv(self.fmt, [({k: v for k, v in x.items()}, {k: v for k, v in w.items()}) for x, w in self.inputs], self.H, self.W,
                 self.stride, self.acc_scale, self.bias, self.residual, self.relu, self.name)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


def conv_from_buffers(fmt, x_split, w_canon, H, W, stride=1, in_scale_log2=0, bias=None, residual=None, relu=False, x2_split=None,
                      w2_canon=None, name=""):
    """x_split: padded split NHWC int16; w_canon: canonical rows; bias (Cout,) f32; residual dense NHWC f32 (N, Ho, Wo, Cout)"""
    inputs = []
    for xs, wc in ((x_split, w_canon), (x2_split, w2_canon)):
        if xs is None:
            continue
        KS = 3 if wc.shape[0] == 9 else 1
        keys = sorted({a for a, _, _ in terms_of(fmt)})
        sl = (slice(0, H + 2), slice(0, W + 2)) if KS == 3 else (slice(1, H + 1), slice(1, W + 1))
        X = {k: x_dense(xs, fmt, k)[:, :, sl[0], sl[1]] for k in keys}
        Wt = {k: w_dense(wc, fmt, k) for k in sorted({b for _, b, _ in terms_of(fmt)})}
        if fmt == 3:                                       # the scale exponents, for the exchanged-scales mutant
            ap = act_parts(_np16(xs), 3)
            X["_sh"] = torch.from_numpy(np.ascontiguousarray(ap["sh"][:, sl[0], sl[1]]))       # (N, Hr, Wr, nch)
            X["_sl"] = torch.from_numpy(np.ascontiguousarray(ap["sl"][:, sl[0], sl[1]]))
        inputs.append((X, Wt))
    b = None if bias is None else bias.double()
    r = None if residual is None else residual.double().permute(0, 3, 1, 2)
    return Conv(fmt, inputs, H, W, stride, 2.0 ** -in_scale_log2, b, r, relu, name)


def _epilogue(acc, A, cv):
    y, a = acc * cv.acc_scale, A * cv.acc_scale
    if cv.bias is not None:
        y, a = y + cv.bias.view(1, -1, 1, 1), a + cv.bias.abs().view(1, -1, 1, 1)
    if cv.residual is not None:
        y, a = y + cv.residual, a + cv.residual.abs()
    if cv.relu:
        y = y.clamp_min(0)
    return y, a


def model64(cv, with_abs=True):
    """-> (y, A) float64 (N, Cout, Ho, Wo)"""
    if getattr(cv, "sums", None) is not None:             # (acc, A) of the products, shared between cases that differ in the epilogue only
        return _epilogue(cv.sums[0], cv.sums[1], cv)
    acc = A = 0.0
    for X, Wt in cv.inputs:
        for a, b, wgt in terms_of(cv.fmt):
            acc = acc + wgt * F.conv2d(X[a], Wt[b], stride=cv.stride)
            if with_abs:
                A = A + wgt * F.conv2d(X[a].abs(), Wt[b].abs(), stride=cv.stride)
    return _epilogue(acc, A if with_abs else acc.abs(), cv)


def emu32(cv):
    """The same sum in float32, one addition per matrix instruction: input by input, chunk by chunk, tap by tap; per tap the 16-channel
    k-steps of the main product (the x3 forms: of all three products), then the K = 64 instruction of both cross sums (its two halves:
    two additions).  Epilogue: one rounding each for acc * scale + bias (an fma; bf16x3: an add), + residual."""
    acc = None
    terms = terms_of(cv.fmt)
    x3 = cv.fmt in (0, 2)
    for X, Wt in cv.inputs:
        Cout, Cin, KS, _ = next(iter(Wt.values())).shape
        Hr, Wr = X[terms[0][0]].shape[-2:]
        Ho, Wo = (Hr - KS) // cv.stride + 1, (Wr - KS) // cv.stride + 1
        if acc is None:
            acc = torch.zeros(X[terms[0][0]].shape[0], Cout, Ho, Wo, dtype=torch.float32)

        def inst(a, b, wgt, c0, c1, ky, kx):
            xs = X[a][:, c0:c1, ky:ky + cv.stride * (Ho - 1) + 1:cv.stride, kx:kx + cv.stride * (Wo - 1) + 1:cv.stride]
            return wgt * torch.einsum("nchw,oc->nohw", xs, Wt[b][:, c0:c1, ky, kx])

        if Cin < 32:                                      # the stem: one K block per kernel row, k = 4 kx + c: k-step s holds kx 4 s .. 4 s + 3
            for ky in range(KS):
                for s in range(2):
                    for a, b, wgt in terms:
                        part = sum(inst(a, b, wgt, 0, Cin, ky, kx) for kx in range(4 * s, min(4 * s + 4, KS)))
                        acc = (acc.double() + part).float()
            continue
        for ch in range(Cin // 32):
            for ky in range(KS):
                for kx in range(KS):
                    for s in range(2):
                        for a, b, wgt in (terms if x3 else terms[:1]):
                            acc = (acc.double() + inst(a, b, wgt, 32 * ch + 16 * s, 32 * ch + 16 * s + 16, ky, kx)).float()
                    if not x3:
                        for a, b, wgt in terms[1:]:
                            acc = (acc.double() + inst(a, b, wgt, 32 * ch, 32 * ch + 32, ky, kx)).float()
    y = acc.double() * cv.acc_scale
    if cv.bias is not None:
        y = y + cv.bias.view(1, -1, 1, 1)
    y = y.float()
    if cv.residual is not None:
        y = (y.double() + cv.residual).float()
    return y.clamp_min(0) if cv.relu else y


def rho(value, y, A):
    """max |value - model64| / (2^-24 A) over the entries with A > 0; an entry with A = 0 must be exact"""
    err = (value.double() - y).abs()
    live = A > 0
    assert bool((err[~live] == 0).all()), "an entry whose terms are all zero is not zero"
    return float((err[live] / (U24 * A[live])).max()) if bool(live.any()) else 0.0


def exact_unit(cv):
    """(q, max A): the power of two q that every term of an EXACT case is a multiple of, from the parts themselves (the largest power of
    two dividing every non-zero operand value, per part; q = acc_scale * min over the terms of q_x q_w wgt) -- None if some value is no
    dyadic rational above 2^-40"""
    def unit(t):
        v = t[t != 0].abs()
        if v.numel() == 0:
            return 1.0
        m, e = torch.frexp(v)                              # v = m 2^e, m in [0.5, 1)
        mi = (m * 2.0 ** 40).round()
        assert bool((mi == m * 2.0 ** 40).all())
        low = (mi.to(torch.int64) & -mi.to(torch.int64)).double()          # lowest set bit of the 40-bit mantissa
        return float((low * 2.0 ** -40 * torch.exp2(e.double())).min())
    q = None
    for X, Wt in cv.inputs:
        for a, b, wgt in terms_of(cv.fmt):
            u = unit(X[a]) * unit(Wt[b]) * wgt * cv.acc_scale
            q = u if q is None else min(q, u)
    for t in (cv.bias, cv.residual):
        if t is not None:
            q = min(q, unit(t))
    return q


# ----------------------------------------------------------------------------------------------------------------------
# mutant models (the sensitivity check): each returns a Conv whose model64 is what a subtly wrong kernel would add
# ----------------------------------------------------------------------------------------------------------------------
def mutants(cv):
    """{name: Conv}: only those that apply to the case's arithmetic and epilogue"""
    fmt = cv.fmt
    terms = terms_of(fmt)
    Cout, Cin, KS, _ = cv.inputs[0][1][terms[0][1]].shape
    nch = Cin // 32
    # the last chunk (of two: the first -- the `relu` rows' second is all zero; the stem has one K block); the bottom-left tap (7 x 7: the
    # centre, the one tap that meets a real pixel at every output of every image size)
    ch, (ky, kx) = (nch - 1 if nch > 2 else 0), ((KS - 1, 0) if KS <= 3 else (KS // 2, KS // 2))
    out = {}

    # one cross sum dropped at one tap of one chunk (the x3 forms: the lo.hi product of that tap and chunk).  `drop` = (term, chunk, ky,
    # kx[, channels]): the term's weights are zeroed there in model64_mutant (a part may feed two terms, so not in the part itself)
    c = cv.copy()
    c.drop = (1, ch, ky, kx)
    out["cross_sum_dropped_one_tap_one_chunk"] = c
    c = cv.copy()
    c.drop = (0, ch, ky, kx, 16)
    out["main_kstep_dropped_one_tap"] = c
    if fmt in (1, 3):
        c = cv.copy()
        k8 = "h8" if fmt == 1 else "h6"
        x = dict(c.inputs[0][0])
        x[k8] = x["h"] * (2.0 ** -F8_AX if fmt == 1 else 1.0)          # what the narrow copy approximates, unrounded
        c.inputs[0] = (x, c.inputs[0][1])
        out["h_in_place_of_narrow_h"] = c
    if fmt == 3:
        c = cv.copy()
        x = dict(c.inputs[0][0])
        d = (x["_sl"] - x["_sh"]).double()                 # (N, Hr, Wr, nch): the two scale bytes of a row exchanged
        f = torch.exp2(d).permute(0, 3, 1, 2).repeat_interleave(32, dim=1)
        x["h6"], x["l6"] = x["h6"] * f, x["l6"] / f
        c.inputs[0] = (x, c.inputs[0][1])
        out["fp6_scales_exchanged"] = c
    if KS > 1:
        c = cv.copy()
        c.inputs[0] = (c.inputs[0][0], {k: v.transpose(2, 3).contiguous() for k, v in c.inputs[0][1].items()})
        out["ky_kx_transposed"] = c
    if cv.bias is not None:
        out["bias_shifted_one_channel"] = cv.copy(bias=torch.roll(cv.bias, 1))
    if cv.residual is not None and cv.residual.shape[-1] > 1:
        out["residual_of_the_neighbouring_pixel"] = cv.copy(residual=torch.roll(cv.residual, 1, dims=3))
    return out


def model64_mutant(cv):
    """model64 of a Conv that may carry a `drop` = (term index, chunk, ky, kx[, channels]) attribute"""
    drop = getattr(cv, "drop", None)
    if drop is None:
        return model64(cv, with_abs=False)[0]
    ti, ch, ky, kx = drop[:4]
    nchan = drop[4] if len(drop) > 4 else 32
    acc = 0.0
    for i, (X, Wt) in enumerate(cv.inputs):
        for j, (a, b, wgt) in enumerate(terms_of(cv.fmt)):
            w = Wt[b]
            if i == 0 and j == ti:
                w = w.clone()
                w[:, 32 * ch:32 * ch + nchan, ky, kx] = 0
            acc = acc + wgt * F.conv2d(X[a], w, stride=cv.stride)
    return _epilogue(acc, acc.abs(), cv)[0]


# ----------------------------------------------------------------------------------------------------------------------
# operands: exact (planted) and realistic
# ----------------------------------------------------------------------------------------------------------------------
def _ints(rng, shape, lo, hi, density):
    v = rng.integers(lo, hi + 1, size=shape).astype(np.float64)
    return v * (rng.random(shape) < density)


def exact_parts(fmt, shape, rng, weight, density=0.5):
    """planted operand parts of `shape` (..., 32): hi / h integers in [-4, 4]; lo / l integers in [-3, 3] times 2^-6; the e4m3 copies
    independent integers in [-3, 3] (l8 times 2^-1 on the weight side); the FP6 blocks independent integers in [-3, 3] under scale
    exponents that vary from row to row (h6: 0 or 1, l6: -2 .. 0)"""
    if fmt in (0, 2):
        a, b = ("hi", "lo") if fmt == 0 else ("h", "l")
        return {a: _ints(rng, shape, -4, 4, density), b: _ints(rng, shape, -3, 3, density) * 2.0 ** -6}
    if fmt == 1:
        return {"h": _ints(rng, shape, -4, 4, density), "h8": _ints(rng, shape, -3, 3, density),
                "l8": _ints(rng, shape, -3, 3, density) * (0.5 if weight else 1.0)}
    sh, sl = rng.integers(0, 2, size=shape[:-1]), rng.integers(-2, 1, size=shape[:-1])
    return {"h": _ints(rng, shape, -4, 4, density), "h6": _ints(rng, shape, -3, 3, density) * np.exp2(sh)[..., None],
            "l6": _ints(rng, shape, -3, 3, density) * np.exp2(sl)[..., None], "sh": sh, "sl": sl}


def exact_act(fmt, N, C, H, W, seed, density=0.5):
    """padded split NHWC int16 of planted rows (border zero)"""
    rng = np.random.default_rng(seed)
    rows = act_rows(exact_parts(fmt, (N, H, W, C // 32, 32), rng, False, density), fmt)
    return padded(rows, H, W)


def exact_weights(fmt, Cout, Cin, KS, seed, density=0.5, exp=0):
    """canonical weight rows of planted parts; `exp` (the x3 forms, whose parts are free of one another): every part times 2^exp"""
    rng = np.random.default_rng(seed + 7)
    T = KS * KS
    parts = exact_parts(fmt, (T, Cin // 32, Cout, 32), rng, True, density)
    if exp:
        assert fmt in (0, 2)
        parts = {k: v * 2.0 ** exp for k, v in parts.items()}
    rows = w_rows(parts, fmt)
    return torch.from_numpy(np.ascontiguousarray(rows).view(np.int16).reshape(T, Cin // 32, Cout, 64))


def exact_bias_residual(N, Cout, Ho, Wo, seed, with_res):
    rng = np.random.default_rng(seed + 13)
    bias = torch.from_numpy(rng.integers(-9, 10, size=Cout).astype(np.float32))
    res = torch.from_numpy(rng.integers(-20, 21, size=(N, Ho, Wo, Cout)).astype(np.float32)) if with_res else None
    return bias, res


def realistic_x(kind, N, C, H, W, seed):
    """the rows the trunk produces: `gauss`, or `relu`: heavy-tailed, 40 % zeros, one all-zero 32-channel chunk (when C >= 64)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, H, W, generator=g)
    if kind == "relu":
        x = x.abs() ** 1.5 * (torch.rand(N, C, H, W, generator=g) > 0.4)
        if C >= 64:
            x[:, 32:64] = 0
    return x


def realistic_layer(Cout, Cin, KS, seed):
    """(weight, BatchNorm) as tests/test_gpu_parity.py draws them"""
    g = torch.Generator().manual_seed(seed + 1)
    wt = torch.randn(Cout, Cin, KS, KS, generator=g) * (2.0 / (Cin * KS * KS)) ** 0.5
    bn = torch.nn.BatchNorm2d(Cout).eval()
    bn.weight.data = torch.rand(Cout, generator=g) * 1.5 + 0.2
    bn.bias.data = torch.randn(Cout, generator=g) * 0.1
    bn.running_mean = torch.randn(Cout, generator=g) * 0.1
    bn.running_var = torch.rand(Cout, generator=g) + 0.5
    return wt, bn


def conv2d_64(x, wt, bn, stride=1, residual=None, relu=False):
    """F.conv2d in float64 of the EXACT operands, BatchNorm folded as the reference applies it"""
    KS = wt.shape[-1]
    ref = F.conv2d(x.double(), wt.double(), stride=stride, padding=KS // 2)
    sc = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).double().view(1, -1, 1, 1)
    ref = (ref - bn.running_mean.double().view(1, -1, 1, 1)) * sc + bn.bias.double().view(1, -1, 1, 1)
    if residual is not None:
        ref = ref + residual.double()
    return (ref.clamp_min(0) if relu else ref).detach()


# ----------------------------------------------------------------------------------------------------------------------
# case tables (the GPU module runs them; the CPU module shows each reaches what it names)
# ----------------------------------------------------------------------------------------------------------------------
HW_EDGES = [(1, 1), (7, 31), (8, 32), (9, 33), (16, 64), (5, 40), (12, 65)]


# conv_split_kernel's instances, as conv_split_launch / conv_split_dispatch select them: (KS, output channels per workgroup, 4-row form) ->
# every route (Cout, conv_cot_cap, conv_narrow) that reaches it.  COT = 256 / 128 / 64 for Cout % 256 / % 128 / else, lowered to the cap;
# 4-row tiles at COT 64 under conv_narrow & 1 and, 3 x 3 only, at COT 128 under conv_narrow & 2.
SPLIT_COUT, SPLIT_CAP, SPLIT_NARROW, SPLIT_CIN = [64, 128, 192, 256, 512], [0, 64, 128], [0, 1, 3], [32, 64, 96, 256]
OPTION_DEFAULTS = {"conv_narrow": 1, "conv_cot_cap": 0, "conv_debug": 0, "conv64_variant": 0}       # the statics of conv_split.hip / conv64.hip


def split_instance(KS, Cout, cap, narrow):
    cot = 256 if Cout % 256 == 0 else 128 if Cout % 128 == 0 else 64
    cot = min(cot, cap) if cap else cot
    return KS, cot, bool((cot == 64 and narrow & 1) or (cot == 128 and KS == 3 and narrow & 2))


def split_routes():
    """{instance: [(Cout, cap, narrow)]}: the whole product of the three axes, sorted into the instance each triple reaches"""
    out = {}
    for KS in (3, 1):
        for Cout in SPLIT_COUT:
            for cap in SPLIT_CAP:
                for narrow in SPLIT_NARROW:
                    out.setdefault(split_instance(KS, Cout, cap, narrow), []).append((Cout, cap, narrow))
    return out


def _covering_routes(routes, n):
    """n routes that show every Cout, every cap and every conv_narrow value the instance can be reached with (greedy), then repeat"""
    need = [{r[k] for r in routes} for k in range(3)]
    picked = []
    while any(need):
        best = max(routes, key=lambda r: sum(r[k] in need[k] for k in range(3)))
        picked.append(best)
        for k in range(3):
            need[k].discard(best[k])
    assert len(picked) <= n
    return [picked[i % len(picked)] for i in range(n)]


def split_cases():
    """conv_split_kernel through ops.conv_split.  Every instance (arithmetic, KS, COT, 4-row form; for bf16x3 at 3 x 3, COT 256 also PINNED /
    compiler-scheduled) runs at all seven edge shapes, and over them meets N = 1 and 3, every Cin, every Cout, conv_cot_cap and conv_narrow
    value that reaches it, every output format, residual and ReLU on and off."""
    out = []
    for ai, arith in enumerate(ARITHS):
        for ii, (inst, routes) in enumerate(sorted(split_routes().items())):
            KS, cot, four = inst
            # conv_debug: 1024 keeps f16f6 on conv_split_kernel (conv256p_cases() run the stream kernel); 16 = bf16x3's compiler-scheduled form
            debugs = [1024] if arith == "f16f6" else [0, 16] if (arith == "bf16x3" and inst == (3, 256, False)) else [0]
            for debug in debugs:
                picked = _covering_routes(routes, len(HW_EDGES))
                for si, (H, W) in enumerate(HW_EDGES):
                    i = si + ii + ai + (debug == 16)
                    Cout, cap, narrow = picked[si]
                    Cin = SPLIT_CIN[i % 4]
                    N = 3 if (si % 2 == 1 and not (Cin == 256 and H * W > 600)) else 1
                    out.append(dict(arith=arith, H=H, W=W, N=N, Cin=Cin, Cout=Cout, KS=KS, narrow=narrow, cot_cap=cap, res=bool(i & 1),
                                    relu=bool(i & 2), out_fmt=ARITHS[i % 4], f32=True, debug=debug, inst=inst + (debug == 16,)))
    for c in out:
        c["id"] = (f"{c['arith']}-{c['H']}x{c['W']}-n{c['N']}-ci{c['Cin']}-co{c['Cout']}-k{c['KS']}-nar{c['narrow']}-cap{c['cot_cap']}"
                   f"-res{int(c['res'])}-relu{int(c['relu'])}-out_{c['out_fmt']}" + ("-sched" if c["debug"] == 16 else ""))
    return out


CONV256P_FORMS = {   # name: (Cout, conv_cot_cap, out_fmt, residual, f32 out, default Cin) -> the instantiation conv_split_launch selects
    "c256_f6_cin128": (256, 0, "f16f6", False, False, 128),     # conv256p_kernel<256, 3, false, false, false, false, 1>: Cin = 128 only
    "c256_f6": (256, 0, "f16f6", False, False, 32),             # <256, 3, false, false, false>: any other Cin
    "c256_f6_f32": (256, 0, "f16f6", False, True, 256),         # <256, 3, false, true, false>
    "c256_f6_res_f32": (256, 0, "f16f6", True, True, 128),      # <256, 3, true, true, false>
    "c256_f6_res": (256, 0, "f16f6", True, False, 32),          # <256, 3, true, false, false>
    "c256_generic": (256, 0, "bf16x3", True, True, 256),        # <256, -1, false, false, true>: every other combination
    "c128_f6": (128, 0, "f16f6", False, False, 128),            # <128, 3, false, false, false>
    "c128_f6_res_f32": (128, 0, "f16f6", True, True, 32),       # <128, 3, true, true, false>
    "c128_f6_res": (256, 128, "f16f6", True, False, 256),       # <128, 3, true, false, false> (256 channels under conv_cot_cap 128)
    "c128_generic": (128, 0, "f16f8", False, True, 128)}        # <128, -1, false, false, true>


def conv256p_cases():
    """the ten forms conv_split_launch selects for the f16f6 3 x 3 convolution (the eleventh, the bank form, runs in BANK_CASES): every
    form at all seven edge shapes, with Cin 32 / 128 / 256 in turn where the form leaves it free (c256_f6_cin128: 128 only; c256_f6: 32
    and 256)"""
    out = []
    for fi, (name, (Cout, cap, out_fmt, res, f32, _)) in enumerate(CONV256P_FORMS.items()):
        cins = {"c256_f6_cin128": [128], "c256_f6": [32, 256]}.get(name, [32, 128, 256])
        for si, (H, W) in enumerate(HW_EDGES):
            Cin, N = cins[(si + fi) % len(cins)], 1 + (si % 3 == 1)
            out.append(dict(arith="f16f6", H=H, W=W, N=N, Cin=Cin, Cout=Cout, KS=3, narrow=1, cot_cap=cap, res=res,
                            relu=bool((si + fi) & 1), out_fmt=out_fmt, f32=f32, debug=0, form=name,
                            id=f"{name}-{H}x{W}-n{N}-ci{Cin}-relu{(si + fi) & 1}"))
    return out


# persistent kernels: (N, H, W) with cdiv(H, 4) cdiv(W, 32) N tiles
CONV64_GRID = 256
CONV64_SHAPES = [(1, 1, 1), (3, 5, 33), (255, 4, 32), (1, 4 * 256, 32), (257, 3, 30), (1, 1028, 31), (27, 2, 577)]
STEM7_GRID = 512
STEM7_SHAPES = [(1, 1, 1), (1, 3, 5), (1, 9, 65), (1, 8, 64), (2, 7, 63), (511, 8, 64), (1, 8 * 512, 64), (1, 8, 64 * 513), (5, 8 * 41 - 1, 64 * 5 - 1)]


def tiles64(N, H, W):
    return N * cdiv(H, 4) * cdiv(W, 32)


def stem7_tiles(N, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return N * cdiv(Ho, 4) * cdiv(Wo, 32)


S2_H = [1, 2, 7, 8, 9]
S2_W = [1, 2, 63, 64, 65, 66]
S2_CIN = [32, 64, 128]
S2_COUT = [32, 96, 128, 256]


def s2_cases():
    """(form, N, Cin, Cout, H, W, relu, proj_relu, id): form 3 = conv_s2_kernel<3>, 1 = <1>, "p" = <3, true>.  Every form at every H with
    every W; over them every (Cin, Cout) pair and, for the fused form, all four pairs of ReLU flags"""
    out = []
    for fi, form in enumerate((3, 1, "p")):
        i = 0
        for H in S2_H:
            for W in S2_W:
                j = i + fi
                Cin, Cout = S2_CIN[j % 3], S2_COUT[(j // 3) % 4]
                out.append((form, 2 if i % 5 == 0 else 1, Cin, Cout, H, W, bool(i & 1), bool(i & 2), f"s2_{form}-{H}x{W}-ci{Cin}-co{Cout}-relu{i & 1}{(i >> 1) & 1}"))
                i += 1
    return out


# ----------------------------------------------------------------------------------------------------------------------
# realistic cases: (kernel, arith, Cin, Cout, KS, N, H, W, rows, residual, relu).  kernel: "split" (ops.conv_split), "c64" (ops.conv64_split),
# "s2" (ops.conv_s2_split), "stem7".  Small shapes with ragged tiles; the data of tests/test_gpu_parity.py.
# ----------------------------------------------------------------------------------------------------------------------
REALISTIC = [(k, a, *rest) for a in ARITHS for k, *rest in (("split", 128, 256, 3, 1, 9, 33, "relu", True, True),
                                                              ("split", 256, 256, 3, 1, 8, 32, "gauss", False, True),
                                                              ("split", 64, 128, 1, 2, 5, 40, "relu", False, False),
                                                              ("split", 32, 192, 3, 1, 12, 65, "relu", True, False))]
REALISTIC += [("c64", a, 64, 64, 3, N, H, W, rows, res, relu) for a in ("bf16x3", "f16f8")
              for N, H, W, rows, res, relu in ((2, 9, 33, "relu", True, True), (1, 4, 32, "gauss", False, True), (1, 3, 5, "relu", True, False))]
REALISTIC += [("s2", "bf16x3", 64, 128, 3, 2, 9, 65, "gauss", False, True), ("s2", "bf16x3", 128, 256, 1, 1, 8, 66, "relu", False, False),
              ("s2", "bf16x3", 32, 96, 3, 1, 7, 63, "relu", False, True),
              ("stem7", "bf16x3", 3, 64, 7, 2, 9, 65, "gauss", False, True), ("stem7", "bf16x3", 3, 64, 7, 1, 3, 5, "gauss", False, False)]


def realistic_id(c):
    k, a, Cin, Cout, KS, N, H, W, rows, res, relu = c
    return f"{k}-{a}-ci{Cin}-co{Cout}-k{KS}-n{N}-{H}x{W}-{rows}-res{int(res)}-relu{int(relu)}"


@functools.lru_cache(maxsize=None)
def realistic(c):
    """One realistic case: operands packed on the host as the packers pack them, the model, its f32 emulation and the float64
    convolution of the exact operands.  -> dict(x, xs, w (canonical rows; stem7: (hi, lo) dense), bias, residual (NHWC f32 or None),
    in_scale, cv, y, A, emu, rho_emu, ref64, A0)"""
    from fgvc_amd import ops
    k, arith, Cin, Cout, KS, N, H, W, rows, res, relu = c
    fmt = FMT[arith]
    seed = sum(int(v) for v in (Cin, Cout, KS, N, H, W)) + 17 * fmt + (1000 if k != "split" else 0)
    stride = 1 if k in ("split", "c64") else 2
    Ho, Wo = ((H - 1) // stride + 1, (W - 1) // stride + 1)
    x = realistic_x(rows, N, Cin, H, W, seed)
    wt, bn = realistic_layer(Cout, Cin, KS, seed)
    g = torch.Generator().manual_seed(seed + 2)
    residual = torch.randn(N, Ho, Wo, Cout, generator=g) if res else None
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
    wfold = (wt.float() * scale.view(-1, 1, 1, 1)).detach()
    out = dict(x=x, residual=residual, relu=relu, stride=stride, Ho=Ho, Wo=Wo, fmt=fmt, wfold=wfold, sx=0, sw=0)
    if k == "stem7":
        _, bias = ops.prepare_stem7(wt, bn)
        bias = bias.detach()
        xsplit = VC.split_bf16_model(x.numpy())            # (N, 3, H, 2, W)
        xp = lambda i: F.pad(torch.from_numpy(_bf16_dec(np.ascontiguousarray(xsplit[:, :, :, i]).view(np.uint16))), (3, 3, 3, 3))
        wsplit = VC.split_bf16_model(wfold.numpy().reshape(-1, 1))          # (n, 2, 1)
        wp = lambda i: torch.from_numpy(_bf16_dec(np.ascontiguousarray(wsplit[:, i, 0]).view(np.uint16)).reshape(64, 3, 7, 7))
        cv = Conv(0, [({"hi": xp(0), "lo": xp(1)}, {"hi": wp(0), "lo": wp(1)})], H, W, 2, 1.0, bias.double(), None, relu, realistic_id(c))
        out.update(xs=None, w=(wp(0).numpy(), wp(1).numpy()), in_scale=0)
    else:
        sx = ops.act_scale_log2(float(x.abs().max())) if fmt else 0
        xs = pack_act(x, fmt, sx)
        if fmt == 0:
            w, bias = ops.prepare_conv_split(wt, bn)
            sw = 0
        else:
            w, bias, sw = ops.prepare_conv_split_f16(wt, bn, fmt)
        w, bias = w.detach(), bias.detach()
        cv = conv_from_buffers(fmt, xs, w, H, W, stride, sx + sw, bias, residual, relu, name=realistic_id(c))
        out.update(xs=xs, w=w, in_scale=sx + sw, sx=sx, sw=sw)
    y, A = model64(cv)
    emu = emu32(cv)
    ref = F.conv2d(x.double(), wfold.double(), stride=stride, padding=KS // 2) + bias.double().view(1, -1, 1, 1)
    A0 = F.conv2d(x.double().abs(), wfold.double().abs(), stride=stride, padding=KS // 2)
    if res:
        ref = ref + residual.double().permute(0, 3, 1, 2)
    out.update(bias=bias, cv=cv, y=y, A=A, emu=emu, rho_emu=rho(emu, y, A), ref64=ref.clamp_min(0) if relu else ref, A0=A0)
    return out


# ----------------------------------------------------------------------------------------------------------------------
# exact cases: planted buffers + their model.  Every builder returns dict(xs | x, w (canonical rows), bias, residual, in_scale, cv, y, A, q)
# ----------------------------------------------------------------------------------------------------------------------
EXACT_IN_SCALE = 3            # log2(s_x s_w) of the f16 forms' planted operands: acc_scale = 2^-3
EXACT_OUT_SCALE = 2           # log2(s_out) of an f16-format split output


def _seed(name):
    import zlib
    return zlib.crc32(name.encode()) & 0x7FFFFFFF


def _finish(out, cv):
    y, A = model64(cv)
    q = exact_unit(cv)
    out.update(cv=cv, y=y, A=A, q=q)
    return out


def exact_split(c):
    """one of split_cases() / conv256p_cases() / proj_cases()"""
    fmt, seed = FMT[c["arith"]], _seed(c["id"])
    N, H, W, Cin, Cout, KS = c["N"], c["H"], c["W"], c["Cin"], c["Cout"], c["KS"]
    xs, w = exact_act(fmt, N, Cin, H, W, seed), exact_weights(fmt, Cout, Cin, KS, seed, exp=c.get("w_exp", 0))
    bias, res = exact_bias_residual(N, Cout, H, W, seed, c["res"])
    in_scale = EXACT_IN_SCALE if fmt else 0
    x2 = w2 = None
    if c.get("Cin2"):
        x2, w2 = exact_act(fmt, N, c["Cin2"], H, W, seed + 1), exact_weights(fmt, Cout, c["Cin2"], 1, seed + 1)
    cv = conv_from_buffers(fmt, xs, w, H, W, 1, in_scale, bias, res, c["relu"], x2, w2, name=c["id"])
    return _finish(dict(xs=xs, w=w, x2=x2, w2=w2, bias=bias, residual=res, in_scale=in_scale), cv)


def proj_cases():
    """the folded projection (fgvc_conv_split_proj_fmt_f32: 3 x 3, 256 output channels + the 1 x 1 convolution of a second input)"""
    out = []
    for ai, arith in enumerate(ARITHS):
        for ci, Cin2 in enumerate((32, 64, 128)):
            H, W = HW_EDGES[(2 * ai + ci + 1) % 7]
            out.append(dict(arith=arith, H=H, W=W, N=1 + (ci == 0 and H * W < 300), Cin=(64, 128, 32)[ci], Cin2=Cin2, Cout=256, KS=3, narrow=1, cot_cap=0,
                            res=bool(ci & 1), relu=bool(ai & 1) or ci == 2, out_fmt=arith, f32=(ci != 1), debug=0))
            if arith == "f16f6":                           # conv_debug 1024: conv_split_kernel<..., X2> in place of the stream kernel
                out.append(dict(out[-1], debug=1024))
    for c in out:
        c["id"] = ("split-" if c["debug"] else "") + f"proj-{c['arith']}-{c['H']}x{c['W']}-n{c['N']}-ci{c['Cin']}-ci2_{c['Cin2']}-res{int(c['res'])}-relu{int(c['relu'])}-f32{int(c['f32'])}"
    return out


BANK_CASES = [(arith, H, W, N, Cin, res, dbg) for arith in ARITHS for H, W, N, Cin, res in ((9, 33, 1, 64, True), (1, 1, 2, 32, False), (12, 65, 1, 128, False))
              for dbg in ((0, 1024) if arith == "f16f6" else (0,))]        # (f16f6: conv256p_kernel's bank form and, conv_debug 1024, conv_split_kernel's)


def exact_bank(case):
    """the bank epilogues' planted convolution (3 x 3, 256 output channels, ReLU).  bf16x3 has no accumulator scale: its planted weights
    carry the 2^-3 instead, so that 256 |y| of the raw rows stays inside f16"""
    arith, H, W, N, Cin, res, dbg = case
    return exact_split(dict(arith=arith, H=H, W=W, N=N, Cin=Cin, Cout=256, KS=3, res=res, relu=True, id=f"bank-{arith}-{H}x{W}-ci{Cin}",
                            w_exp=-3 if arith == "bf16x3" else 0))


def conv64_cases():
    """(arith, N, H, W, residual: None | "f32" | "split", relu, out_fmt, f32 out, variant, id): conv64_kernel<0> (bf16x3), <1> (f16f8 with a
    combination the stream kernel does not take), conv64k_kernel (conv64_variant 32) and the four conv64p_kernel forms"""
    out = []
    forms = [("k0", "bf16x3", "f32", "bf16x3", True, 0), ("k0_rsplit", "bf16x3", "split", "bf16x3", True, 0), ("k0_plain", "bf16x3", None, "f16f8", True, 0),
             ("k1", "f16f8", None, "f16f8", True, 0), ("k1_bf16out", "f16f8", "f32", "bf16x3", True, 0),
             ("c64k", "f16f8", "f32", "f16f8", True, 32), ("c64k_plain", "f16f8", None, "f16f8", False, 32),
             ("p_plain", "f16f8", None, "f16f8", False, 0), ("p_res_f32", "f16f8", "f32", "f16f8", True, 0),
             ("p_res", "f16f8", "f32", "f16f8", False, 0), ("p_res_bf16", "f16f8", "f32", "bf16x3", False, 0)]
    for si, (N, H, W) in enumerate(CONV64_SHAPES):             # shape by shape: the forms share a shape's planted sums (_conv64_planted)
        for fi, (name, arith, res, out_fmt, f32, variant) in enumerate(forms):
            out.append((arith, N, H, W, res, bool((fi + si) & 1), out_fmt, f32, variant, f"{name}-n{N}-{H}x{W}-tiles{tiles64(N, H, W)}"))
    return out


@functools.lru_cache(maxsize=2)
def _conv64_planted(arith, N, H, W):
    """operands and their sums (before the epilogue) of one shape: the forms of conv64_cases() share them"""
    fmt, seed = FMT[arith], _seed(f"c64-{arith}-{N}-{H}-{W}")
    xs, w = exact_act(fmt, N, 64, H, W, seed), exact_weights(fmt, 64, 64, 3, seed)
    cv = conv_from_buffers(fmt, xs, w, H, W, 1, 0, None, None, False)
    return xs, w, cv, model64(cv), seed


def exact_conv64(c):
    arith, N, H, W, res, relu, out_fmt, f32, variant, name = c
    xs, w, cv0, sums, seed = _conv64_planted(arith, N, H, W)
    bias, r = exact_bias_residual(N, 64, H, W, seed + _seed(name) % 1000, res is not None)
    in_scale = EXACT_IN_SCALE if FMT[arith] else 0
    cv = cv0.copy(acc_scale=2.0 ** -in_scale, bias=bias.double(), residual=None if r is None else r.double().permute(0, 3, 1, 2), relu=relu, name=name)
    cv.sums = sums
    return _finish(dict(xs=xs, w=w, bias=bias, residual=r, in_scale=in_scale), cv)


def exact_s2(c):
    form, N, Cin, Cout, H, W, relu, proj_relu, name = c
    seed = _seed(name)
    KS = 1 if form == 1 else 3
    xs, w = exact_act(0, N, Cin, H, W, seed), exact_weights(0, Cout, Cin, KS, seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    bias, _ = exact_bias_residual(N, Cout, Ho, Wo, seed, False)
    out = _finish(dict(xs=xs, w=w, bias=bias, residual=None, in_scale=0), conv_from_buffers(0, xs, w, H, W, 2, 0, bias, None, relu, name=name))
    if form == "p":
        w2 = exact_weights(0, Cout, Cin, 1, seed + 1)
        bias2, _ = exact_bias_residual(N, Cout, Ho, Wo, seed + 1, False)
        out["proj"] = _finish(dict(w=w2, bias=bias2), conv_from_buffers(0, xs, w2, H, W, 2, 0, bias2, None, proj_relu, name=name + "-proj"))
    return out


def stem7_cases():
    """(N, H, W, relu, out_fmt, id)"""
    return [(N, H, W, bool(i & 1) or i == 0, ("bf16x3", "f16f8")[(i >> 1) & 1], f"stem7-n{N}-{H}x{W}-tiles{stem7_tiles(N, H, W)}")
            for i, (N, H, W) in enumerate(STEM7_SHAPES)]


def exact_stem7(c):
    N, H, W, relu, out_fmt, name = c
    rng = np.random.default_rng(_seed(name))
    a = _ints(rng, (N, 3, H, W), -7, 7, 0.6)                # hi = a: |b| 2^-10 lies below half a unit of a's 8 bits; where a = 0 the residual is 0 too
    x = (a + _ints(rng, (N, 3, H, W), -3, 3, 0.6) * 2.0 ** -10 * (a != 0)).astype(np.float32)
    xsplit = VC.split_bf16_model(x)                        # (N, 3, H, 2, W)
    xp = lambda i: F.pad(torch.from_numpy(_bf16_dec(np.ascontiguousarray(xsplit[:, :, :, i]).view(np.uint16))), (3, 3, 3, 3))
    hi, lo = _ints(rng, (64, 3, 7, 7), -4, 4, 0.5), _ints(rng, (64, 3, 7, 7), -3, 3, 0.5) * 2.0 ** -6
    bias = torch.from_numpy(rng.integers(-9, 10, size=64).astype(np.float32))
    cv = Conv(0, [({"hi": xp(0), "lo": xp(1)}, {"hi": torch.from_numpy(hi), "lo": torch.from_numpy(lo)})], H, W, 2, 1.0, bias.double(), None, relu, name)
    return _finish(dict(x=torch.from_numpy(x), w=torch.from_numpy(pack_stem7(hi, lo)), bias=bias), cv)


def format_bound(r):
    """Part 2 for the f16 forms, derived from the formats: a bound on |model64 - float64 convolution of the exact operands| per entry.
    With x' = s_x x = h + l exactly (h = f16(x'), l the f32 residual) and the cross terms fed L ~ l and H ~ h,
        x' w' - (h_x h_w + L_x H_w + H_x L_w) = (l_x h_w - L_x H_w) + (h_x l_w - H_x L_w) + l_x l_w,
        |l h - L H| <= dl |h| + (|l| + dl) dh,        dl >= |L - l|, dh >= |H - h|,
    and per element (half a unit of the narrow format at the value's magnitude, or of its subnormal range):
        f16x3   H = h;  L = f16(l):                      dl = max(2^-11 |l|, 2^-25)
        f16f8   L = e4m3(2^B l) 2^-B, H = e4m3(2^-A h) 2^A:   dl = max(|l| / 16, 2^-10 2^-B),  dh = max(|h| / 16, 2^-10 2^A)
        f16f6   H = e2m3 of h under the block's scale (block maximum m in (3.75, 7.5] 2^s):   dh = max(|h| / 16, m / 60);
                L likewise of f16(2^11 l) 2^-11:         dl = d1 + max((|l| + d1) / 16, m_l (1 + 2^-11) / 60),  d1 = max(2^-11 |l|, 2^-36)
    (a value that is exactly zero stays zero).  The sum of these over the taps and channels, times acc_scale -> (N, Cout, Ho, Wo)."""
    fmt, KS = r["fmt"], r["wfold"].shape[-1]
    assert fmt in (1, 2, 3)

    def parts(v):
        h = v.half().float()
        return h.double().abs(), (v - h).double().abs()

    hx, lx = parts(r["x"].float() * 2.0 ** r["sx"])
    hw, lw = parts(r["wfold"] * 2.0 ** r["sw"])

    def blockmax(t):                                       # over each 32-channel chunk of dim 1
        n = t.shape[1] // 32
        m = t.reshape(t.shape[0], n, 32, *t.shape[2:]).amax(2, keepdim=True)
        return m.expand(t.shape[0], n, 32, *t.shape[2:]).reshape(t.shape)

    def nz(t, d):
        return torch.where(t > 0, d, torch.zeros_like(d))

    z = torch.zeros_like
    if fmt == 2:
        dlx, dlw, dhx, dhw = nz(lx, (lx * 2.0 ** -11).clamp_min(2.0 ** -25)), nz(lw, (lw * 2.0 ** -11).clamp_min(2.0 ** -25)), z(hx), z(hw)
    elif fmt == 1:
        dlx, dhx = nz(lx, (lx / 16).clamp_min(2.0 ** (-10 - F8_BX))), nz(hx, (hx / 16).clamp_min(2.0 ** (-10 + F8_AX)))
        dlw, dhw = nz(lw, (lw / 16).clamp_min(2.0 ** (-10 - F8_BW))), nz(hw, (hw / 16).clamp_min(2.0 ** (-10 + F8_AW)))
    else:
        def d6(h, l):
            d1 = nz(l, (l * 2.0 ** -11).clamp_min(2.0 ** -36))
            return nz(l, d1 + torch.maximum((l + d1) / 16, blockmax(l) * (1 + 2.0 ** -11) / 60)), nz(h, torch.maximum(h / 16, blockmax(h) / 60))
        (dlx, dhx), (dlw, dhw) = d6(hx, lx), d6(hw, lw)
    conv = lambda a, b: F.conv2d(a, b, stride=r["stride"], padding=KS // 2)
    acc = conv(dlx, hw) + conv(lx + dlx, dhw) + conv(dhx, lw) + conv(hx + dhx, dlw) + conv(lx, lw)
    return acc * 2.0 ** -(r["sx"] + r["sw"])
