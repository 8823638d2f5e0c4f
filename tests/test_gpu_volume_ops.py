"""GPU: the materialised correlation volume (csrc/corr_volume.hip: fgvc_corr_volume_f32 / _bf16x3 / _bf16, fgvc_split_bf16;
corr_volume_f8.hip; corr_volume_f6.hip) against float64 restatements of the same sums, at its tile and chunk edges.

Run on an MI355X with `pytest -m gpu`.  Every case
  * checks EVERY entry of the volume against the kernel's own float64 model (tests/volume_cases.py: the very products the kernel adds,
    of the very operand values it reads) under the accumulation bound n 2^-24 A / tau derived there, and prints the largest
    measured / bound ratio (the closing test prints the per-kernel, per-C maxima);
  * writes into a view that starts 4096 floats into a NaN-filled buffer and ends 4096 floats before its end: every entry of the view
    must come back finite, both bands must still be NaN bit for bit (a store before row 0 or behind the last row is seen, not suffered).
The format halves of the bounds (model against the float64 product of the f32 rows) are asserted on the CPU, from the models alone, in
tests/test_volume_reference_share.py, which also shows by arithmetic that every case id reaches what it names.

What the cases reach that no small test reached before: blockIdx.y > 0 (`kb0 = blockIdx.y * kchunk`) and the ragged tail of a chunk in
corr_volume_f32_kernel<32|64|128|256> and corr_volume_bf16_kernel<64|128, 1|3, 4, 1>; corr_volume_f32_kernel<32> at all; for C = 256
the `kb + sb >= kb1` break inside a 64-key stage and both sides of the counted-wait choice; every row-class period of the f16f8 / f16f6
kernels with classes that hold no row (`n_v == 0`), forced key chunks (`corr8_debug >> 8`), forced half-chunks per tile pair
(`corr6_debug >> 12`: the two-segment piece, the pair without a second tile) and both `corr6_sdma` forms.  Only those three options are
touched, each inside try / finally that puts the default back; the module's last test shows the default volume is bit for bit the one
its first test computed.
"""
import contextlib
import math

import numpy as np
import pytest
import torch

from tests import test_gpu_window_ops as WO
from tests import volume_cases as VC

pytestmark = pytest.mark.gpu
TEMP, TOL = VC.TEMP, VC.TOL
NAN_BITS = int(torch.tensor([float("nan")]).view(torch.int32).item())
OPTION_DEFAULT = {"corr8_debug": 0, "corr6_debug": 0, "corr6_sdma": 1}
STATS = {}                 # (kernel, C) -> (largest measured / bound, the case that produced it)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()          # the HIP library must be the thing under test: fail loudly if it is missing
    return torch.device("cuda:0")


@contextlib.contextmanager
def option(name, value):
    """one of the three launch overrides, put back to its default whatever happens inside"""
    from fgvc_amd import ops
    try:
        ops.set_option(name, value)
        yield
    finally:
        ops.set_option(name, OPTION_DEFAULT[name])


def guarded_volume(dev, prec, qop, kop, tau, HWq, HWk):
    """ops.corr_volume into a (HWk, HWq) view between two NaN bands of VC.GUARD floats; the bands must survive bit for bit"""
    from fgvc_amd import ops
    n = HWk * HWq
    buf = torch.full((2 * VC.GUARD + n,), float("nan"), device=dev)
    out = buf[VC.GUARD:VC.GUARD + n].view(HWk, HWq)
    assert out.data_ptr() % 16 == 0
    ops.corr_volume(qop, kop, tau, prec, out=out)
    torch.cuda.synchronize()
    bits = buf.view(torch.int32)
    front, back = bits[:VC.GUARD] != NAN_BITS, bits[VC.GUARD + n:] != NAN_BITS
    assert not bool(front.any()), (prec, HWq, HWk, "stores in front of row 0", front.nonzero().flatten()[:8].tolist())
    assert not bool(back.any()), (prec, HWq, HWk, "stores behind the last row", back.nonzero().flatten()[:8].tolist())
    return out.cpu()


def check_entries(got, model, A, prec, C, tau, what):
    """every entry: finite, and within the accumulation bound of the kernel's own float64 model"""
    assert got.shape == model.shape
    holes = ~torch.isfinite(got)
    assert not bool(holes.any()), (what, "entries never written (or not finite)", int(holes.sum()), holes.nonzero()[:4].tolist())
    bound = VC.accum_bound(prec, C, A, tau)
    err = (got.double() - model).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"{what}: {got.numel()} entries, max |got - model64| {float(err.max()):.3e}, max bound {float(bound.max()):.3e}, "
          f"largest measured / bound {ratio:.3f} (n = {VC.accum_n(prec, C)})")
    key = (prec, C)
    if key not in STATS or ratio > STATS[key][0]:
        STATS[key] = (ratio, what)
    bad = err > bound                                                # an entry whose products are all zero must be exactly zero
    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero()[:4].tolist(), float((err / bound.clamp_min(1e-300))[bad].max()))
    return ratio


def narrow_tools(prec):
    from fgvc_amd import ops
    if prec == "f16f8":
        return ops.split_f16f8, VC._decode_f16f8, VC.f16f8_model64
    return ops.split_f16f6, VC._decode_f16f6, VC.f16f6_model64


def narrow_volume(dev, prec, HWq, HWk, kind, what, opt=None):
    """one f16f8 / f16f6 case: split on the GPU, decode the kernel's own operand rows, model, both parts of the bound, guard bands"""
    split, decode, model64 = narrow_tools(prec)
    q, k = VC.pair_rows(kind, HWq, HWk, 256, False)
    qs, ks = split(q.to(dev)), split(k.to(dev))
    with (option(*opt) if opt else contextlib.nullcontext()):
        got = guarded_volume(dev, prec, qs, ks, TEMP, HWq, HWk)
    model, A = model64(decode(qs), decode(ks), TEMP)
    check_entries(got, model, A, prec, 256, TEMP, f"{prec} {what} {kind}")
    e64 = float((got.double() - VC.volume64(q, k, TEMP)).abs().max())      # part 2 on the kernel's own output: the project bar, as today
    print(f"  vs volume64: {e64:.3e} (bar {TOL:.1e})")
    assert e64 < TOL, (prec, what, e64)
    return got


@pytest.fixture(scope="module")
def baseline(dev):
    """the default-option volumes of one ragged shape, computed before anything else in this module touches an option"""
    HWq, HWk, kind = VC.BASE_SHAPE
    return {prec: narrow_volume(dev, prec, HWq, HWk, kind, "baseline") for prec in ("f16f8", "f16f6")}


def test_default_volume_recorded_first(baseline):
    assert set(baseline) == {"f16f8", "f16f6"}


# ======================================================================================================================
# f32
# ======================================================================================================================
@pytest.mark.parametrize("case", VC.f32_cases(), ids=lambda c: c[-1])
def test_f32_volume(dev, case):
    """corr_volume_f32_kernel<32|64|128|256>: 128-query x 32-key tiles, 16 key blocks per workgroup.  513 keys = 17 blocks: the second
    chunk holds one block with one live row; 1100 keys = 16 + 16 + 3.  Unit-norm, ReLU-like and unnormalised (|x| up to 30) rows; an
    all-zero key row (entries exactly 0), one-hot rows, one query row equal to a key row."""
    C, HWq, HWk, tau, kind, name = case
    q, k = VC.pair_rows(kind, HWq, HWk, C)
    got = guarded_volume(dev, "f32", q.to(dev), k.to(dev), tau, HWq, HWk)
    model, A = VC.f32_model64(q, k, tau)
    check_entries(got, model, A, "f32", C, tau, f"f32 {name} {kind}")


# ======================================================================================================================
# bf16x3 / bf16
# ======================================================================================================================
def test_split_bf16_bitwise(dev):
    """fgvc_split_bf16 equals hi = bf16_rne(x), lo = bf16_rne(f32(x - hi)) bit for bit: ties to even in the 16th bit (up, down and with a
    carry into the exponent), x - hi exactly zero, a residual that is itself a tie, negative zero, magnitudes 2^-60 .. 2^60."""
    from fgvc_amd import ops
    for rows in (VC.split_rows(), VC.split_rows(n=1, C=4, seed=8), VC.split_rows(n=300, C=256, seed=9)):
        want = torch.from_numpy(VC.split_bf16_model(rows))
        got = ops.split_bf16(torch.from_numpy(rows).to(dev)).cpu()
        assert got.shape == want.shape and got.dtype == torch.int16
        diff = got != want
        assert not bool(diff.any()), (rows.shape, int(diff.sum()), diff.nonzero()[:4].tolist(),
                                      [hex(int(v) & 0xFFFF) for v in got[diff][:4]], [hex(int(v) & 0xFFFF) for v in want[diff][:4]])


@pytest.mark.parametrize("prec", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", VC.bf16_cases(), ids=lambda c: c[-1])
def test_bf16_volume(dev, prec, case):
    """corr_volume_bf16_kernel<64|128, 3|1, 4, 1> (32-key register-staged stages) and <256, 3|1, 8, 2> (64-key DMA stages, the `kb + sb >=
    kb1` break, the counted wait) from the MODEL's split operands, against hi.hi + hi.lo + lo.hi (bf16: hi.hi) of those operands."""
    C, HWq, HWk, tau, kind, name = case
    q, k = VC.pair_rows(kind, HWq, HWk, C)
    qs, ks = torch.from_numpy(VC.split_bf16_model(q)), torch.from_numpy(VC.split_bf16_model(k))
    got = guarded_volume(dev, prec, qs.to(dev), ks.to(dev), tau, HWq, HWk)
    model, A = (VC.bf16x3_model64 if prec == "bf16x3" else VC.bf16_model64)(qs, ks, tau)
    check_entries(got, model, A, prec, C, tau, f"{prec} {name} {kind}")
    # part 2 on the kernel's own output (the halves are asserted from the models alone in test_volume_reference_share.py)
    fmt = VC.BF16X3_FORMAT if prec == "bf16x3" else VC.BF16_FORMAT
    total = fmt * VC.abs64(q, k) / tau + VC.accum_bound(prec, C, A, tau)
    assert bool(((got.double() - VC.volume64(q, k, tau)).abs() <= total).all())


# ======================================================================================================================
# f16f8 / f16f6
# ======================================================================================================================
def test_split_f16f8_format(dev):
    """The operand rows of fgvc_corr_volume_f16f8 decoded on the host: h is exactly f16(256 x); h8 / l8 reproduce h and its residual to
    half an e4m3 step at their magnitude (2^-4 relative for normal values, 2^-10 absolute below 2^-6)."""
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(5)
    f = torch.nn.functional.normalize(torch.randn(2048, 256, generator=g), dim=1)
    f[:64] = 0
    f[:64, 3] = 1.0
    f[64:128] = torch.nn.functional.normalize(f[64:128] * (torch.rand(64, 256, generator=g) < 0.05) + 1e-6, dim=1)
    sp = ops.split_f16f8(f.to(dev))
    assert sp.shape == (2048, 1024) and sp.dtype == torch.uint8
    h, h8, l8 = VC._decode_f16f8(sp)
    x = f.double().numpy()
    h_ref = (f.numpy() * np.float32(256)).astype(np.float16).astype(np.float64)
    l_ref = (x * 256 - h_ref) * 256
    assert (h == h_ref).all()
    assert np.isfinite(h8).all() and np.isfinite(l8).all()
    for got, ref in ((h8, h_ref), (l8, l_ref)):
        bound = np.maximum(np.abs(ref) / 16, 2.0 ** -10) * 1.0001
        assert (np.abs(got - ref) <= bound).all(), float(np.abs(got - ref).max())
    k, q = slice(0, 1024), slice(1024, 2048)
    tot = h[k] @ h[q].T + (h8[k] @ l8[q].T + l8[k] @ h8[q].T) / 256.0
    assert float(np.abs(tot / 65536.0 / 0.07 - (x[k] @ x[q].T) / 0.07).max()) < TOL


@pytest.mark.parametrize("prec", ["f16f8", "f16f6"])
@pytest.mark.parametrize("case", VC.f8_cases(), ids=lambda c: c[-1])
def test_narrow_volume_row_classes(dev, prec, case):
    """corr_volume_f16f8_v2_kernel / corr_volume_f16f6_kernel at the launch's own chunking: periods 1, 2, 4 and the unshifted fallback on
    both sides of the +31 of n_q, key counts 1, 2, 3 (classes with no row at all), 5, 64, 65 (one stage, one row over), 200, 609."""
    HWq, HWk, kind, name = case
    narrow_volume(dev, prec, HWq, HWk, kind, name)


@pytest.mark.parametrize("case", VC.F8_KC_CASES, ids=lambda c: f"q{c[0]}-k{c[1]}-kc{c[2]}")
def test_f16f8_forced_key_chunks(dev, case):
    """corr8_debug = kc << 8 (key blocks per workgroup; even, as the launch itself picks them): chunk boundaries at every stage / every
    second stage, workgroups whose chunk starts behind a class's last row, and the same volume as the default chunking."""
    HWq, HWk, kc = case
    kind = VC.KINDS4[(HWq + HWk + kc) % 4]
    got = narrow_volume(dev, "f16f8", HWq, HWk, kind, f"q{HWq} k{HWk} kc{kc}", opt=("corr8_debug", kc << 8))
    assert torch.equal(got, narrow_volume(dev, "f16f8", HWq, HWk, kind, f"q{HWq} k{HWk} default"))      # an entry's sum does not depend on the chunking


@pytest.mark.parametrize("case", VC.F6_C_CASES, ids=lambda c: f"q{c[0]}-k{c[1]}-c{c[2]}")
def test_f16f6_forced_half_chunks(dev, case):
    """corr6_debug = c << 12 (half-chunks per tile pair) where the launch's search could have picked c: odd c run the piece of two
    segments (two prologues); 256 / 255 / 33 queries: the pair's second tile does not exist; 513: a whole pair and a lone tile."""
    HWq, HWk, c = case
    kind = VC.KINDS4[(HWq + HWk + c) % 4]
    got = narrow_volume(dev, "f16f6", HWq, HWk, kind, f"q{HWq} k{HWk} c{c}", opt=("corr6_debug", c << 12))
    assert torch.equal(got, narrow_volume(dev, "f16f6", HWq, HWk, kind, f"q{HWq} k{HWk} default"))


@pytest.mark.parametrize("case", VC.F6_SDMA_CASES, ids=lambda c: f"q{c[0]}-k{c[1]}")
def test_f16f6_sdma_forms_bit_identical(dev, case):
    """corr6_sdma = 0 (64-bit lane addresses, query fragments straight from memory) and 1 (scalar base, query rows through the LDS)"""
    HWq, HWk = case
    kind = VC.KINDS4[(HWq + HWk) % 4]
    a = narrow_volume(dev, "f16f6", HWq, HWk, kind, f"q{HWq} k{HWk} sdma0", opt=("corr6_sdma", 0))
    b = narrow_volume(dev, "f16f6", HWq, HWk, kind, f"q{HWq} k{HWk} sdma1", opt=("corr6_sdma", 1))
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ======================================================================================================================
# refusals, the caller, the closing check
# ======================================================================================================================
def test_refusals_before_any_launch(dev):
    """Every unsupported request raises FgvcHipError and leaves the NaN-filled output untouched: f32 at C = 96; bf16x3 / bf16 at C = 192
    (a multiple of 64, refused by the launch); f16f8 / f16f6 operands of C = 128; tau = 0 on every entry point."""
    from fgvc_amd import _lib, ops
    n = 8

    def refused(prec, qop, kop, tau):
        out = torch.full((n, n), float("nan"), device=dev)
        with pytest.raises(_lib.FgvcHipError):
            ops.corr_volume(qop, kop, tau, prec, out=out)
        torch.cuda.synchronize()
        assert bool((out.view(torch.int32) == NAN_BITS).all()), prec

    f = lambda C: torch.nn.functional.normalize(torch.randn(n, C, generator=torch.Generator().manual_seed(C)), dim=1).to(dev)
    refused("f32", f(96), f(96), TEMP)
    s192 = torch.from_numpy(VC.split_bf16_model(f(192).cpu())).to(dev)
    refused("bf16x3", s192, s192, TEMP)
    refused("bf16", s192, s192, TEMP)
    narrow128 = torch.zeros(n, 512, dtype=torch.uint8, device=dev)
    refused("f16f8", narrow128, narrow128, TEMP)
    refused("f16f6", narrow128, narrow128, TEMP)
    s64 = torch.from_numpy(VC.split_bf16_model(f(64).cpu())).to(dev)
    refused("f32", f(64), f(64), 0.0)
    refused("bf16x3", s64, s64, 0.0)
    refused("bf16", s64, s64, 0.0)
    refused("f16f8", ops.split_f16f8(f(256)), ops.split_f16f8(f(256)), 0.0)
    refused("f16f6", ops.split_f16f6(f(256)), ops.split_f16f6(f(256)), 0.0)


def test_dense_attend_bf16x3_two_key_chunks(dev):
    """ops.dense_attend(precision='bf16x3') at C = 64, T = 2, 33 x 17 = 561 keys (18 key blocks: two chunks of the C = 64 form) against
    the float64 attend over the bf16x3 kernel's own slabs (read back), under test_gpu_window_ops.sum_bound alone -- the attend kernel
    on GIVEN slabs; the f32 call likewise over the f32 slabs.  The slabs themselves differ by at most delta, the two volume kernels' own
    bounds on unit-norm rows (A <= 1)."""
    from fgvc_amd import ops
    C, T, (Hq, Wq), (Hk, Wk), P = 64, 2, (9, 13), (33, 17), 5
    HWq, HWk = Hq * Wq, Hk * Wk
    assert VC.cdiv(HWk, 32) > 16
    g = torch.Generator().manual_seed(91)
    q, key = torch.randn(1, C, Hq, Wq, generator=g), torch.randn(T, C, Hk, Wk, generator=g)
    labels = WO.make_labels(T, HWk, P, seed=4)
    qf, kf = ops.normalize_to_hwc(q.to(dev))[0], ops.normalize_to_hwc(key.to(dev))
    none = ops.MaskSpec.none()
    got3 = ops.dense_attend(qf, kf, labels.to(dev), Hq, Wq, Hk, Wk, none, TEMP, "softmax", precision="bf16x3").cpu()
    got32 = ops.dense_attend(qf, kf, labels.to(dev), Hq, Wq, Hk, Wk, none, TEMP, "softmax", precision="f32").cpu()
    vols = torch.stack([ops.corr_volume(qf, kf[t], TEMP, "f32").cpu() for t in range(T)], 0)
    qs, ks = ops.split_bf16(qf), ops.split_bf16(kf)
    vols3 = torch.stack([ops.corr_volume(qs, ks[t], TEMP, "bf16x3").cpu() for t in range(T)], 0)
    amax = 1.00001                                                            # |k| |q| of rows normalised in f32
    delta = (VC.BF16X3_FORMAT + (VC.accum_n("bf16x3", C) + VC.accum_n("f32", C)) * VC.U24) * amax / TEMP
    dv = float((vols3.double() - vols.double()).abs().max())
    want = WO.attend_ref(vols.double(), labels.double(), None, "softmax")
    bound, e32 = WO.sum_bound(want, WO.attend_ref(vols, labels, None, "softmax"), float(vols.max() - vols.min()), True)
    # the bf16x3 call against the float64 attend over ITS OWN slabs, under the attend bound alone (the slabs themselves: dv <= delta)
    want3 = WO.attend_ref(vols3.double(), labels.double(), None, "softmax")
    bound3, _ = WO.sum_bound(want3, WO.attend_ref(vols3, labels, None, "softmax"), float(vols3.max() - vols3.min()), True)
    ef, e3 = float((got32.double() - want).abs().max()), float((got3.double() - want3).abs().max())
    assert float((want3 - want).abs().max()) <= math.expm1(2 * delta)          # what a logit perturbation delta can do to a softmax mean of labels in [0, 1]
    print(f"dense_attend C64 T2 561 keys: slabs bf16x3 vs f32 {dv:.3e} (delta {delta:.3e}); f32 err {ef:.3e} (bound {bound:.3e}), "
          f"bf16x3 err {e3:.3e} (bound {bound3:.3e})")
    assert dv <= delta and ef <= bound and e3 <= bound3


def test_default_volume_unchanged_and_report(dev, baseline):
    """After every override above: the options are back at their defaults -- the default-option volume of the ragged shape is bit for bit
    the one the module's first test computed -- and the per-kernel, per-C maxima of measured / bound are printed."""
    HWq, HWk, kind = VC.BASE_SHAPE
    for prec in ("f16f8", "f16f6"):
        again = narrow_volume(dev, prec, HWq, HWk, kind, "closing")
        assert torch.equal(again.view(torch.int32), baseline[prec].view(torch.int32)), prec
    print("largest measured / bound per kernel and C:")
    for (prec, C), (ratio, what) in sorted(STATS.items()):
        print(f"  {prec:7s} C {C:3d}  n {VC.accum_n(prec, C):3d}  ratio {ratio:.3f}  ({what})")
