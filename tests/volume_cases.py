"""Case tables, seeded rows, float64 restatements and bounds shared by tests/test_gpu_volume_ops.py (the materialised correlation
volume: csrc/corr_volume.hip, corr_volume_f8.hip, corr_volume_f6.hip) and tests/test_volume_reference_share.py (the same statements
on the CPU, from the models alone).  No GPU code here: numpy integer arithmetic on bit patterns and plain float64 torch products.

Every kernel is held to a TWO-PART bound.

Part 1, kernel against its own model (GPU module, every entry): the model is the float64 sum of exactly the products the kernel adds,
formed from exactly the operand values the kernel reads, so what is left is f32 accumulation:
        |got - model64| <= n * 2^-24 * A / tau,     A = sum over every product the kernel adds of |a| |b|   (float64, per entry)
    f32     n = C / 2 + 3:  two independent chains (acc0, acc1) of C / 4 v_mfma_f32_32x32x2_f32 each, i.e. C / 2 fused products per
            chain (at most one rounding per product), + the add acc0 + acc1, + the division, + the distance of f32(tau) from tau
            (below 2^-24 relative).  Tighter than the (C + 4) 2^-24 of a single C-long chain because the kernel has two.
    bf16    n = C + 4 (the form tests/test_gpu_window_ops.py uses for the c2f logits): bf16 x bf16 products are exact in f32, a
            chain adds C of them (C - 1 roundings), + accx + accy and acc += (bf16x3), + inv_t = 1 / tau, + the multiply, + f32(tau).
    f16f8 / f16f6   n = C + 4 with A over all three sums (h.h + 2^-8 (h8.l8 + l8.h8)); f16 x f16 and 4-bit x 4-bit products are exact
            in f32, the scales are powers of two.  This one is an EMPIRICAL BAR, not a derived bound: the three sums share one
            accumulator, a strictly sequential chain of the 3 C products would need 3 C + 3, and C + 4 is simply the bar of the other
            kernels asked of this one too (the matrix instruction adds K = 32 / 128 products per step; measured: 0.05 of it).
    What this bound was seen to catch (one run of the GPU module per mutant library, table in docs/LAB_NOTES.md): a dropped bf16 cross
    term and an unmultiplied k16 group in every bf16 case at every C; the f32 kernel's second chain replaced by its first in every f32
    case; tau in place of 1 / tau in the ragged store branch in every case with a ragged tile (but the one shape whose only ragged
    column is all zeros); a dropped fp8 cross sum in every f16f8 case with more than one key row -- that sum is ~1e-4 logit rms on
    Gaussian unit rows against a bar of 2.2e-4 A, so it is the maximum over a volume's entries that crosses the bar, and a single key
    row (or an exact one-hot key, whose residual is zero) does not.

Part 2, model against volume64 (CPU module, from the models alone): the FORMAT's error, a property of the number format and not
derived tighter here.
    bf16x3  bf16 keeps 8 significant bits: with 2^E <= |x| < 2^(E+1), |x - hi| <= 2^(E-8) <= 2^-8 |x| (half a unit of hi).  The residual
            r = x - hi is either exactly 2^(E-8) (kept exactly) or lies below it, where half a unit of ITS 8 bits is 2^(E-17):
            x = hi + lo + e with |lo| <= 2^-8 |x| and |e| <= 2^-17 |x|.  Then
            k q - (kh qh + kh ql + kl qh) = k eq + ek q - ek eq + kl ql,  so  |.| <= (2^-17 + 2^-17 + 2^-34 + 2^-16) |k| |q| < 2.0001 * 2^-16 |k| |q|:
            BF16X3_FORMAT * A0 / tau with A0 = sum |k_c| |q_c|  (3.05e-5 A0 / tau; 4.4e-4 on unit rows at tau 0.07; measured far below).
    bf16    k q - kh qh = k dq + dk q - dk dq.  Asserted: the first-order bound the kernel family was given, BF16_FORMAT = 2 * 2^-9 |k| |q|,
            i.e. a MEAN rounding error of a quarter unit per operand.  It is not the worst case -- that is 2 * 2^-8, both operands half a
            unit off in the same direction in every channel -- and holds on every entry of these rows (the CPU module prints the
            ratios): a one-hot operand is exact, so such an entry carries the other operand's error only, at most 2^-8 / (1 + 2^-8) |k| |q|
            = 0.996 of the bound (0.987 is reached); sums over many channels average and stay far below.
    f16f8 / f16f6   the project bar 1e-3 on unit-norm rows at tau 0.07, as tests/test_gpu_parity.py states it.
"""
import functools

import numpy as np
import torch

TEMP = 0.07
TOL = 1e-3                # the project's bar on logits
U24 = 2.0 ** -24
GUARD = 4096              # floats of NaN in front of and behind every output view (a multiple of 4: the view stays 16-byte aligned)
BF16X3_FORMAT = 2.0001 * 2.0 ** -16
BF16_FORMAT = 2.0 * 2.0 ** -9
F_SCALE = 256.0           # F8_S / F6_S of the .hip files

# ----------------------------------------------------------------------------------------------------------------------
# case tables
# ----------------------------------------------------------------------------------------------------------------------
# f32 kernel: tile 128 queries x 32 keys, 16 key blocks (KCHUNK) per workgroup.  (HWq, HWk, what it reaches)
F32_SHAPES = [(1, 1, "smallest"), (31, 5, "subtile"), (128, 32, "exact_tiles"), (129, 33, "one_over"),
              (257, 513, "17blocks_chunk2_one_live_row"), (300, 1100, "35blocks_16_16_3")]
F32_C = [32, 64, 128, 256]
F32_TAU = [0.07, 1.0]
F32_TAU_SMALL = {32: (300, 1100), 64: (257, 513), 128: (129, 33), 256: (31, 5)}          # tau 0.01 on one shape per C
# bf16x3 / bf16, C = 64, 128: 4 waves (128 queries), 32-key register-staged stages, KCHUNK = 16
BF16_SMALL_C = [64, 128]
# bf16x3 / bf16, C = 256: 8 waves (256 queries), 64-key DMA stages (two key blocks), 16 key blocks per workgroup
BF16_256_SHAPES = [(1, 1, "smallest"), (255, 63, "under_one_tile"), (256, 64, "one_full_tile"), (257, 65, "over_one_tile"),
                   (513, 1056, "33blocks_16_16_1_half_stage"), (300, 1100, "35blocks_16_16_3_stage_then_half"),
                   (512, 1024, "all_full_two_chunks_counted_wait_only")]
KINDS3 = ["gauss", "relu", "raw30"]                  # f32 / bf16 kernels: rotated over the cases
KINDS4 = ["gauss", "relu", "onehot", "heavy"]        # f16f8 / f16f6: unit-norm rows as test_gpu_parity's ragged test makes them

# f16f8 / f16f6 (C = 256).  HWq: every row-class period on both sides of the +31 in n_q = cdiv(HWq + 31, 256)
F8_HWQ = [256, 240, 48, 232, 248, 40, 255, 33]       # m = 0 | m = 16, p = 2 | m = 8, 24, 8: p = 4 | odd m: the unshifted fallback
F8_HWK = [1, 2, 3, 5, 64, 65, 200, 609]              # 1, 2, 3: classes with no row at p = 2 / 4; 200: 7 virtual blocks at p = 1; 609: c_half = 5 admitted
F8_KC_CASES = [(hq, hk, kc) for hq in (256, 240, 248, 33) for hk in (3, 200, 609) for kc in (2, 4)]        # corr8_debug = kc << 8 (even only)
F8_KC_CASES.append((240, 129, 2))                    # p = 2, n_v = [65, 64]: 3 blocks against 2, class 1's second chunk starts behind its last block
# corr6_debug = c << 12, each c only where the launch's own search could have picked it (2 s_tile / c >= 4).  513 x 609: p = 1, three
# tiles = a whole pair + a pair without a second tile, the odd c run the two-segment piece across two real tiles; 48 x 1100: p = 2, the
# two-segment piece runs from the class-0 tile into the class-1 tile
F6_C_CASES = ([(hq, 609, c) for hq in (256, 33, 255) for c in (1, 2, 3, 4, 5)] + [(513, 609, c) for c in (2, 3, 5)] +
              [(48, 609, 1), (48, 609, 2), (240, 609, 2), (40, 609, 1), (48, 1100, 3), (48, 1100, 4), (256, 200, 1), (256, 65, 1)])
F6_SDMA_CASES = [(hq, hk) for hq in (256, 240, 40, 33) for hk in (3, 65, 609)]
BASE_SHAPE = (240, 65, "heavy")                      # the ragged shape whose default-option volume opens and closes the GPU module


def cdiv(a, b):
    return (a + b - 1) // b


def kind3(i):
    return KINDS3[i % 3]


def f32_cases():
    """(C, HWq, HWk, tau, kind, id)"""
    out = []
    for ci, C in enumerate(F32_C):
        for si, (HWq, HWk, what) in enumerate(F32_SHAPES):
            for ti, tau in enumerate(F32_TAU):
                out.append((C, HWq, HWk, tau, kind3(ci + si + ti), f"C{C}-{HWq}x{HWk}-{what}-tau{tau}"))
        HWq, HWk = F32_TAU_SMALL[C]
        out.append((C, HWq, HWk, 0.01, kind3(ci), f"C{C}-{HWq}x{HWk}-tau0.01"))
    return out


def bf16_cases():
    """(C, HWq, HWk, tau, kind, id) for the two bf16 kernels"""
    out = []
    for ci, C in enumerate(BF16_SMALL_C):
        for si, (HWq, HWk, what) in enumerate(F32_SHAPES):
            out.append((C, HWq, HWk, TEMP, kind3(ci + si), f"C{C}-{HWq}x{HWk}-{what}"))
    for si, (HWq, HWk, what) in enumerate(BF16_256_SHAPES):
        out.append((256, HWq, HWk, TEMP, kind3(si), f"C256-{HWq}x{HWk}-{what}"))
    return out


def f8_cases():
    """(HWq, HWk, kind, id): the id names the row-class period and whether some class has no row"""
    out = []
    for iq, HWq in enumerate(F8_HWQ):
        for ik, HWk in enumerate(F8_HWK):
            geo = f8_geometry(HWq, HWk)
            tag = "-nv0" if min(geo["n_v"]) == 0 else ""
            out.append((HWq, HWk, KINDS4[(iq + ik) % 4], f"q{HWq}-m{HWq & 31}-p{geo['period']}-k{HWk}{tag}"))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# launch geometry, written out from the comments and launch functions of corr_volume_f8.hip / corr_volume_f6.hip
# ----------------------------------------------------------------------------------------------------------------------
def row_class_period(HWq):
    """(period, shifted): vol row j starts at float offset (j HWq) mod 32 of a 128-byte line; with m = HWq mod 32 the phase has period
    32 / gcd(m, 32) in j; periods above 4 (odd m, and m = 2, 4, 6 ...) run unshifted as ONE class."""
    m = HWq & 31
    g = 32
    while g > 1 and m % g:
        g >>= 1
    p = 32 // g
    return (1, False) if p > 4 else (p, p > 1)


def f8_geometry(HWq, HWk, kc=0):
    p, shifted = row_class_period(HWq)
    n_q = cdiv(HWq + (31 if p > 1 else 0), 256)            # shifted classes start up to 31 queries early
    n_vb = cdiv(cdiv(HWk, p), 32)                          # 32-row blocks of virtual rows per class
    n_v = [(HWk - c + p - 1) // p for c in range(p)]       # virtual rows of class c: key rows j = p v + c
    kchunk, best = n_vb + (n_vb & 1), -1
    for c in range(1, 33):
        k = cdiv(n_vb, c)
        k += k & 1
        cost = ((n_q * p * cdiv(n_vb, k) + 255) // 256) * (20000 + 5800 * (k // 2))
        if best < 0 or cost < best:
            best, kchunk = cost, k
    if kc:
        kchunk = kc
    return dict(period=p, shifted=shifted, n_q=n_q, n_vb=n_vb, n_v=n_v, kchunk=kchunk, chunks=cdiv(n_vb, kchunk),
                last_chunk_blocks=n_vb - (cdiv(n_vb, kchunk) - 1) * kchunk)


def f6_geometry(HWq, HWk, c=0):
    p, shifted = row_class_period(HWq)
    n_q = cdiv(HWq + (31 if p > 1 else 0), 256)
    n_vb = cdiv(cdiv(HWk, p), 32)
    s_tile, n_tiles = cdiv(n_vb, 2), n_q * p               # 64-key stages per tile; tiles = (query tile, row class)
    n_pairs = cdiv(n_tiles, 2)
    c_half, best = 2, -1.0
    for cc in range(1, 65):
        stages = 2.0 * s_tile / cc
        if stages < 4:
            break
        pro = 1.0 + 1.0 / cc if cc & 1 else 1.0
        cost = float((n_pairs * cc + 255) // 256) * (20000 * pro + 5700 * stages)
        if best < 0 or cost < best:
            best, c_half = cost, cc
    admitted = 2.0 * s_tile / c >= 4 if c else True
    if c:
        c_half = c
    cuts = [i * 2 * s_tile // c_half for i in range(c_half + 1)]
    crossing = any(a < s_tile < b for a, b in zip(cuts[:-1], cuts[1:]))            # a piece that runs from one tile into the next
    return dict(period=p, shifted=shifted, n_q=n_q, n_vb=n_vb, s_tile=s_tile, n_tiles=n_tiles, n_pairs=n_pairs, c_half=c_half,
                admitted=admitted, cuts=cuts, crossing=crossing, n_v=[(HWk - cl + p - 1) // p for cl in range(p)])


# ----------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def feature_rows(kind, n, C, role):
    """(n, C) f32 rows.  gauss / relu / onehot / heavy: unit norm (relu: one shared positive direction + noise, large positive cosines
    between any two rows; onehot: 2 % live channels over a 1e-4 floor, row 0 a true one-hot, a negative zero; heavy: cubed Gaussians);
    raw30: NOT normalised, per-row scales up to 10, i.e. magnitudes up to about 30."""
    g = _gen(7919 * (["gauss", "relu", "raw30", "onehot", "heavy"].index(kind) + 1) + 31 * n + C + 100003 * role)
    x = torch.randn(n, C, generator=g)
    if kind == "raw30":
        return (x * (0.05 + 10.0 * torch.rand(n, 1, generator=g))).contiguous()
    if kind == "relu":
        base = torch.randn(1, C, generator=_gen(424242 + C))
        x = torch.relu(base + 0.3 * x)
    elif kind == "onehot":
        x = x * (torch.rand(n, C, generator=g) < 0.02) + 1e-4 * torch.randn(n, C, generator=g)
        x[0] = 0.0
        x[0, 5] = -1.0
        if n > 1:
            x[1, 7] = -0.0
    elif kind == "heavy":
        x = x ** 3
    return torch.nn.functional.normalize(x, dim=1).contiguous()


@functools.lru_cache(maxsize=64)
def pair_rows(kind, HWq, HWk, C, specials=True):
    """q (HWq, C), k (HWk, C) f32.  One q row equals one k row (cosine 1 on unit rows: the largest entry); with `specials` and at least
    four rows a side also an all-zero k row, a one-hot k row and a negative one-hot q row."""
    q, k = feature_rows(kind, HWq, C, 0), feature_rows(kind, HWk, C, 1)
    q[min(3, HWq - 1)] = k[min(3, HWk - 1)]
    if specials:
        amp = 30.0 if kind == "raw30" else 1.0
        if HWk >= 4:
            k[1] = 0.0
            k[2] = 0.0
            k[2, 5 % C] = amp
        if HWq >= 4:
            q[HWq - 1] = 0.0
            q[HWq - 1, C - 1] = -amp
    return q.contiguous(), k.contiguous()


def split_rows(n=67, C=64, seed=3):
    """(n, C) f32 built from bit patterns, magnitudes 2^-60 .. 2^60 (every non-zero value and every non-zero residual x - hi a normal
    f32).  Column class c % 8:  0 random;  1 a tie in the 16th bit above an even bf16 (rounds down);  2 a tie above an odd bf16 (rounds up,
    a carry into the exponent when the seven bits are all ones);  3 the low 16 bits zero (x - hi exactly 0);  4 / 5 one unit below / above
    the tie;  6 hi rounds down and the RESIDUAL is itself a tie of its own 8 bits;  7 zeros, +0 and -0 alternating."""
    rng = np.random.default_rng(seed)
    e = rng.integers(127 - 60, 127 + 61, size=(n, C)).astype(np.uint32)
    s = rng.integers(0, 2, size=(n, C)).astype(np.uint32)
    top = rng.integers(0, 1 << 7, size=(n, C)).astype(np.uint32)
    low = rng.integers(0, 1 << 16, size=(n, C)).astype(np.uint32)
    cls = np.arange(C)[None, :] % 8
    top = np.where(cls == 1, top & ~np.uint32(1), np.where(cls == 2, top | np.uint32(1), top))
    top[0, 2] = 0x7F                                                                   # the tie that carries into the exponent
    r7 = rng.integers(0, 1 << 7, size=(n, C)).astype(np.uint32)
    low = np.select([(cls == 1) | (cls == 2), cls == 3, cls == 4, cls == 5, cls == 6],
                    [np.uint32(0x8000), np.uint32(0), np.uint32(0x7FFF), np.uint32(0x8001), np.uint32(0x4000) | (r7 << 7) | np.uint32(0x40)], low)
    bits = (s << 31) | (e << 23) | (top << 16) | low
    bits = np.where(cls == 7, (np.arange(n, dtype=np.uint32)[:, None] & 1) << 31, bits).astype(np.uint32)
    return np.ascontiguousarray(bits).view(np.float32)


# ----------------------------------------------------------------------------------------------------------------------
# restatements
# ----------------------------------------------------------------------------------------------------------------------
def volume64(q, k, tau):
    """the float64 product k @ q.T / tau of the GIVEN rows: (HWk, HWq)"""
    return (k.double() @ q.double().t()) / tau


def abs64(q, k):
    """A0 = sum_c |k_c| |q_c| in float64"""
    return k.double().abs() @ q.double().abs().t()


def _bf16_rne(u):
    """f32 bit patterns (uint32, finite) -> bf16 bit patterns (uint16), round to nearest even"""
    u = u.astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_to_f32(h):
    return (h.astype(np.uint32) << 16).view(np.float32)


def split_bf16_model(x):
    """hi = bf16_rne(x), lo = bf16_rne(f32(x - hi)) on the f32 bit patterns -> int16 (..., 2, C), ops.split_bf16's layout.  x: numpy or
    torch f32."""
    x = np.ascontiguousarray(x.numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32)
    hi = _bf16_rne(x.view(np.uint32))
    res = (x - _bf16_to_f32(hi)).astype(np.float32)          # exact: x - hi has at most 16 significant bits
    lo = _bf16_rne(res.view(np.uint32))
    return np.stack([hi, lo], axis=-2).view(np.int16)


def bf16_parts(split):
    """int16 (n, 2, C) bf16 bit patterns (numpy or torch) -> hi, lo as float64 torch (n, C)"""
    s = split.cpu().numpy() if isinstance(split, torch.Tensor) else split
    f = _bf16_to_f32(np.ascontiguousarray(s).view(np.uint16)).astype(np.float64)
    return torch.from_numpy(f[:, 0]), torch.from_numpy(f[:, 1])


def sum_terms(terms, tau, unit=1.0):
    """terms: [(K (HWk, C), Q (HWq, C), weight)] float64, operands in units of sqrt(unit) -> (sum_t w K Q^T / unit / tau, A = sum_t w
    |K| |Q|^T / unit: the absolute products, in the units of <k, q>)"""
    val = sum(w * (K @ Q.t()) for K, Q, w in terms) / unit / tau
    A = sum(w * (K.abs() @ Q.abs().t()) for K, Q, w in terms) / unit
    return val, A


def f32_model64(q, k, tau):
    return sum_terms([(k.double(), q.double(), 1.0)], tau)


def bf16x3_model64(qs, ks, tau):
    """hi.hi + hi.lo + lo.hi of the split operands qs, ks (int16 (n, 2, C)) in float64, / tau -> (value, A)"""
    qh, ql = bf16_parts(qs)
    kh, kl = bf16_parts(ks)
    return sum_terms([(kh, qh, 1.0), (kh, ql, 1.0), (kl, qh, 1.0)], tau)


def bf16_model64(qs, ks, tau):
    qh, _ = bf16_parts(qs)
    kh, _ = bf16_parts(ks)
    return sum_terms([(kh, qh, 1.0)], tau)


def accum_n(prec, C):
    """roundings on the longest path of the kernel's f32 accumulation (module docstring)"""
    return C // 2 + 3 if prec == "f32" else C + 4


def accum_bound(prec, C, A, tau):
    return accum_n(prec, C) * U24 * A / tau


# e4m3 (OCP "fn": bias 7, no infinity, 0x7f / 0xff NaN) and e2m3 value tables
E4M3 = np.array([(m / 8.0) * 2.0 ** -6 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7) for e in range(16) for m in range(8)])
E4M3[127] = np.nan
E4M3 = np.concatenate([E4M3, -E4M3])
E2M3 = np.array([(m / 8.0 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 1)) for e in range(4) for m in range(8)])
E2M3 = np.concatenate([E2M3, -E2M3])


def _decode_f16f8(sp):
    """fgvc_split_f16f8 rows (n, 1024) uint8 -> h, h8, l8 as (n, 256) float64.  Layout (csrc/corr_volume_f8.hip, ops.split_f16f8): per
    pixel [h = f16(256 x), 512 B | h8 = e4m3(h), 256 B | l8 = e4m3(256 (256 x - h)), 256 B], channels in natural order."""
    sp = sp.cpu().numpy() if isinstance(sp, torch.Tensor) else sp
    h = sp[:, :512].copy().view(np.float16).astype(np.float64)
    return h, E4M3[sp[:, 512:768]], E4M3[sp[:, 768:1024]]


def _decode_f16f6(sp):
    """fgvc_split_f16f6 rows (n, 1024) uint8 -> h, h6, l6 as (n, 256) float64 (h6 / l6 dequantised with their 2^(s-4) scales);
    the layout is documented in fgvc_amd/csrc/corr_volume_f6.hip"""
    import numpy as np
    sp = sp.cpu().numpy()
    n = sp.shape[0]
    h = sp[:, :512].copy().view(np.float16).astype(np.float64)
    lut = np.array([(m / 8.0 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 1)) for e in range(4) for m in range(8)])
    lut = np.concatenate([lut, -lut])
    outs = []
    for base in (512, 704):
        vals = np.zeros((n, 256))
        for u in range(2):
            for g in range(4):
                b16 = sp[:, base + 96 * u + 16 * g: base + 96 * u + 16 * g + 16]
                b8 = sp[:, base + 96 * u + 64 + 8 * g: base + 96 * u + 64 + 8 * g + 8]
                bits = np.unpackbits(np.concatenate([b16, b8], axis=1), axis=1, bitorder="little")     # (n, 192)
                codes = (bits.reshape(n, 32, 6) * (1 << np.arange(6))).sum(-1)
                sc = sp[:, 896 + 4 * g + (u if base == 512 else 2 + u)].astype(np.int64) - 127
                vals[:, 128 * u + 32 * g: 128 * u + 32 * g + 32] = lut[codes] * (2.0 ** sc)[:, None]
        outs.append(vals)
    return h, outs[0], outs[1]


def f16f8_model64(q_parts, k_parts, tau):
    """The three sums of corr_volume_f16f8_v2_kernel from decoded rows (h, h8, l8): h.h on the f16 instruction, h8.l8 and l8.h8 on the
    scaled fp8 instruction with the A scale 2^-8; out_scale = 1 / (tau S S) -> (value, A)"""
    qh, q8, ql = (torch.from_numpy(np.ascontiguousarray(a)) for a in q_parts)
    kh, k8, kl = (torch.from_numpy(np.ascontiguousarray(a)) for a in k_parts)
    return sum_terms([(kh, qh, 1.0), (k8, ql, 2.0 ** -8), (kl, q8, 2.0 ** -8)], tau, F_SCALE * F_SCALE)


def f16f6_model64(q_parts, k_parts, tau):
    """As f16f8_model64 from _decode_f16f6's (h, h6, l6): each decoded 6-bit operand already carries the 2^-4 of its stored scale, so a
    cross product enters at 2^-8 -> (value, A)"""
    qh, q6, ql = (torch.from_numpy(np.ascontiguousarray(a)) for a in q_parts)
    kh, k6, kl = (torch.from_numpy(np.ascontiguousarray(a)) for a in k_parts)
    return sum_terms([(kh, qh, 1.0), (k6, ql, 1.0), (kl, q6, 1.0)], tau, F_SCALE * F_SCALE)


# ---- host statements of the two narrow formats (CPU module: the format halves of the f16f8 / f16f6 bounds from the models alone) ----
def _nearest_even(a, table):
    """a >= 0 (float64) -> the nearest value of the ascending `table` (code i = table[i]), a tie to the even code; clamps at the top"""
    a = np.minimum(a, table[-1])
    i = np.clip(np.searchsorted(table, a), 1, len(table) - 1)
    lo, hi = table[i - 1], table[i]
    up = (a - lo > hi - a) | ((a - lo == hi - a) & (i % 2 == 0))
    return np.where(up, hi, lo)


def f16_parts_host(x):
    """x (n, C) f32 -> h = f16(f32(256 x)) and l = f32(256 (256 x - h)), as float64"""
    xs = (x.numpy() if isinstance(x, torch.Tensor) else x).astype(np.float32) * np.float32(F_SCALE)
    h = xs.astype(np.float16)
    l = (xs - h.astype(np.float32)) * np.float32(F_SCALE)
    return h.astype(np.float64), l.astype(np.float64)


def split_f16f8_host(x):
    """(h, e4m3(h), e4m3(l)) in float64, round to nearest even: the format fgvc_split_f16f8 documents"""
    h, l = f16_parts_host(x)
    t = E4M3[:127]
    return h, np.sign(h) * _nearest_even(np.abs(h), t), np.sign(l) * _nearest_even(np.abs(l), t)


def split_f16f6_host(x):
    """(h, h6, l6) in float64, each narrow operand carrying 2^-4 as _decode_f16f6 returns it: per 32 channels the E8M0 scale 2^s with
    s = ceil(log2(max / 7.5)) (at least -40), e2m3 round to nearest even"""
    h, l = f16_parts_host(x)
    outs = []
    for v in (h, l):
        b = v.reshape(v.shape[0], -1, 32)
        m = np.abs(b).max(-1, keepdims=True)
        with np.errstate(divide="ignore"):
            s = np.where(m > 0, np.ceil(np.log2(np.maximum(m, 1e-300) / 7.5)), -40.0)
        s = np.maximum(s, -40.0)
        s = np.where(m * 2.0 ** -s > 7.5, s + 1, s)
        y = b * 2.0 ** -s
        outs.append((np.sign(y) * _nearest_even(np.abs(y), E2M3[:32]) * 2.0 ** s / 16.0).reshape(v.shape))
    return h, outs[0], outs[1]
