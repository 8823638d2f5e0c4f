"""GPU: the encoder's convolutions (csrc/conv_split.hip: conv_split_kernel, conv256p_kernel; conv64.hip: conv64_kernel<0|1>,
conv64k_kernel, conv64p_kernel; conv_s2.hip; stem7.hip) against float64 models of the sums they add, at their tile and chunk edges.

Run on an MI355X with `pytest -m gpu`.  tests/conv_cases.py has the decoders, the models and the case tables;
tests/test_conv_reference_share.py shows on the CPU that the decoders invert the packers, that every exact case satisfies
A < 2^24 q, that the bar separates every mutant model, and that the tables reach what they name.

* EXACT cases (tolerance zero): operands planted as bit patterns, every product a multiple of one power of two and every sum below
  2^24 of it, so the f32 output must equal model64 bit for bit whatever the order of additions -- at every tile border, every chunk,
  every tap; h8 / h6 are planted different from the e4m3 / e2m3 copy of h and lo independent of hi, so a wrong operand, tap or channel
  shows.  The split output must be, byte for byte, the host packer's encoding of the kernel's own f32 output (of the model where the
  form has no f32 output), in all four output formats; the overflow word must stay 0.
* REALISTIC cases: rho = max |got - model64| / (2^-24 A) must stay within 4 rho of the f32 emulation of the same sum, computed in the
  test from the model alone.  The closing test prints the table (docs/LAB_NOTES.md keeps a copy).
* GUARD BANDS everywhere: every f32 output, second output and bank is a view 4096 elements into a NaN-filled buffer (every entry must
  come back finite, both bands NaN bit for bit); every split output has a poisoned interior, a zero border and pattern bands around it,
  and is compared WHOLE with what it must hold.  100 % of the entries, no sampling.
Options (conv_narrow, conv_cot_cap, conv_debug 16 | 1024, conv64_variant 32 -- A/B switches between forms with identical results) are
set inside try / finally that puts the defaults back.
"""
import contextlib

import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import conv_cases as CC

pytestmark = pytest.mark.gpu
NAN_BITS = int(torch.tensor([float("nan")]).view(torch.int32).item())
BAND = 0x5A5A
POISON = 0x7FFF                      # a NaN as bf16 and as f16, NaN bytes as e4m3
DEFAULTS = CC.OPTION_DEFAULTS        # the library's own (its C ABI has no getter; test_conv_reference_share.py holds them to the sources)
STATS = {}                           # (kernel, arith) -> (rho_kernel / rho_emu, rho_kernel, rho_emu, case)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def options(**kw):
    from fgvc_amd import ops
    try:
        for k, v in kw.items():
            ops.set_option(k, v)
        yield
    finally:
        for k in kw:
            ops.set_option(k, DEFAULTS[k])


# ----------------------------------------------------------------------------------------------------------------------
# guarded outputs
# ----------------------------------------------------------------------------------------------------------------------
class F32Out:
    """a contiguous f32 view of `shape` between two NaN bands of CC.GUARD floats"""

    def __init__(self, dev, shape):
        self.n = int(np.prod(shape))
        self.buf = torch.full((2 * CC.GUARD + self.n,), float("nan"), device=dev)
        self.view = self.buf[CC.GUARD:CC.GUARD + self.n].view(*shape)
        assert self.view.data_ptr() % 16 == 0 and self.view.is_contiguous()

    def check(self, what):
        """bands intact, every entry finite -> the view on the CPU"""
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        front, back = bits[:CC.GUARD] != NAN_BITS, bits[CC.GUARD + self.n:] != NAN_BITS
        assert not bool(front.any()), (what, "stores in front of the tensor", front.nonzero().flatten()[:8].tolist())
        assert not bool(back.any()), (what, "stores behind the tensor", back.nonzero().flatten()[:8].tolist())
        got = self.view.cpu()
        holes = ~torch.isfinite(got)
        assert not bool(holes.any()), (what, "entries never written (or not finite)", int(holes.sum()), holes.nonzero()[:4].tolist())
        return got


class SplitOut:
    """a padded split NHWC int16 tensor between two pattern bands: interior poisoned, border zero"""

    def __init__(self, dev, N, C, H, W):
        Hp, Wp = CC.pad_dims(H, W)
        self.shape, self.H, self.W = (N, Hp, Wp, C // 32, 64), H, W
        self.n = int(np.prod(self.shape))
        self.buf = torch.full((2 * CC.GUARD + self.n,), BAND, dtype=torch.int16, device=dev)
        self.view = self.buf[CC.GUARD:CC.GUARD + self.n].view(*self.shape)
        self.view.zero_()
        self.view[:, 1:H + 1, 1:W + 1] = POISON
        assert self.view.data_ptr() % 16 == 0

    def check(self, want, what):
        """bands intact; no poison left in the interior; the border still zero; every int16 what `want` (padded, border zero) holds"""
        torch.cuda.synchronize()
        front, back = self.buf[:CC.GUARD] != BAND, self.buf[CC.GUARD + self.n:] != BAND
        assert not bool(front.any()) and not bool(back.any()), (what, "stores outside the split tensor")
        got = self.view.cpu()
        H, W = self.H, self.W
        inner = got[:, 1:H + 1, 1:W + 1]
        rows_left = (inner[..., :32] == POISON).all(-1)                      # the h / hi half of a row no kernel has written
        assert not bool(rows_left.any()), (what, "interior rows never written", int(rows_left.sum()), rows_left.nonzero()[:4].tolist())
        border = got.clone()
        border[:, 1:H + 1, 1:W + 1] = 0
        assert not bool(border.any()), (what, "the zero border was written", border.nonzero()[:4].tolist())
        assert tuple(want.shape) == tuple(got.shape)
        diff = got != want
        assert not bool(diff.any()), (what, "split bytes", int(diff.sum()), diff.nonzero()[:6].tolist(),
                                      [hex(int(v) & 0xFFFF) for v in got[diff][:6]], [hex(int(v) & 0xFFFF) for v in want[diff][:6]])
        return got


def nhwc(y):
    """model (N, C, H, W) float64 -> dense NHWC"""
    return y.permute(0, 2, 3, 1).contiguous()


def assert_bit_exact(got, y, what):
    want = nhwc(y)
    diff = got.double() != want
    assert not bool(diff.any()), (what, "f32 output differs from model64", int(diff.sum()), diff.nonzero()[:6].tolist(),
                                  got[diff][:6].tolist(), want[diff][:6].tolist())


def record(kernel, arith, rho_k, rho_e, what):
    ratio = rho_k / rho_e
    print(f"{kernel} {arith} {what}: rho_kernel {rho_k:.3f}, rho_emu {rho_e:.3f}, ratio {ratio:.3f}")
    if (kernel, arith) not in STATS or ratio > STATS[(kernel, arith)][0]:
        STATS[(kernel, arith)] = (ratio, rho_k, rho_e, what)
    assert rho_k <= CC.BAR_FACTOR * rho_e, (kernel, arith, what, rho_k, rho_e)


# ----------------------------------------------------------------------------------------------------------------------
# launchers: one call each, every output guarded
# ----------------------------------------------------------------------------------------------------------------------
def launch_split(dev, c, e, out_fmt, so, f32, split=True, set_options=True):
    """ops.conv_split under the case's options (set_options=False: under whatever is in force) -> (f32 output on the CPU or None,
    SplitOut or None)"""
    from fgvc_amd import ops
    N, H, W, Cout = c["N"], c["H"], c["W"], c["Cout"]
    of = F32Out(dev, (N, H, W, Cout)) if f32 else None
    os_ = SplitOut(dev, N, Cout, H, W) if split else None
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    dv = lambda t: None if t is None else t.to(dev)
    with (options(conv_narrow=c.get("narrow", 1), conv_cot_cap=c.get("cot_cap", 0), conv_debug=c.get("debug", 0)) if set_options else contextlib.nullcontext()):
        ops.conv_split(dv(e["xs"]), dv(e["w"]), dv(e["bias"]), H, W, c["relu"], residual=dv(e["residual"]), out_split=os_.view if split else None,
                       out_f32=of.view if f32 else None, in_fmt=CC.FMT[c["arith"]], in_scale_log2=e["in_scale"], out_fmt=out_fmt, out_scale_log2=so,
                       overflow=ovf, x2_split=dv(e.get("x2")), w2=dv(e.get("w2")))
        torch.cuda.synchronize()
    assert int(ovf.item()) == 0, (c["id"], "overflow word")
    return (of.check(c["id"]) if f32 else None), os_


def exact_split_case(dev, c):
    e = CC.exact_split(c)
    out_fmt = CC.FMT[c["out_fmt"]]
    got, os_ = launch_split(dev, c, e, out_fmt, CC.EXACT_OUT_SCALE, c["f32"])
    if got is not None:
        assert_bit_exact(got, e["y"], c["id"])
    src = got if got is not None else nhwc(e["y"]).float()
    os_.check(CC.expected_split(src, out_fmt, CC.EXACT_OUT_SCALE), c["id"])


@pytest.mark.parametrize("c", CC.split_cases(), ids=lambda c: c["id"])
def test_conv_split_exact(dev, c):
    """conv_split_kernel<KS, COT, ..., ARITH>: every instance conv_split_dispatch selects (3 x 3 and 1 x 1; 256 / 128 / 64 output channels
    per workgroup, 8-row and 4-row tiles; the PINNED bf16x3 form and the compiler-scheduled one), EACH at 1 x 1, 7 x 31, 8 x 32, 9 x 33,
    16 x 64, 5 x 40 and 12 x 65 pixels, and over them with N = 1 and 3, 1 / 2 / 3 / 8 input chunks, every Cout, conv_cot_cap and
    conv_narrow value that reaches it, every format out (tests/test_conv_reference_share.py asserts the coverage per instance)."""
    exact_split_case(dev, c)


@pytest.mark.parametrize("c", CC.conv256p_cases(), ids=lambda c: c["id"])
def test_conv256p_exact(dev, c):
    """conv256p_kernel in each of the ten forms conv_split_launch selects for the f16 + FP6 3 x 3 layers, each at all seven edge shapes,
    Cin 32 / 128 / 256 in turn where the form leaves it free"""
    exact_split_case(dev, c)


@pytest.mark.parametrize("c", CC.proj_cases(), ids=lambda c: c["id"])
def test_conv_split_folded_projection_exact(dev, c):
    """fgvc_conv_split_proj_fmt_f32: + the 1 x 1 convolution of a second input of 32 / 64 / 128 channels in the same sums (f16f6: the
    stream kernel's form; the others: conv_split_kernel<..., X2>)"""
    exact_split_case(dev, c)


@pytest.mark.parametrize("case", CC.BANK_CASES, ids=lambda c: f"bank-{c[0]}-{c[1]}x{c[2]}-n{c[3]}-ci{c[4]}-res{int(c[5])}-dbg{c[6]}")
def test_conv_split_bank_epilogues_exact(dev, case):
    """Both bank epilogues (f16f6p: 1 KiB rows; f16f6x: + the f32 channels), raw and normalised, on planted operands.  Raw: the f32
    channels of the f16f6x rows ARE model64, and both banks' FP6 halves are the oracle's encoding of them, byte for byte.  Normalised:
    the f32 channels are model64 / |model64| within 8 roundings (the sum of 256 squares as a tree of depth 8, square root, reciprocal,
    product), the FP6 halves encode those very channels, and the f16f6p bank holds the same rows."""
    from fgvc_amd import ops
    arith, H, W, N, Cin, res, dbg = case
    e = CC.exact_bank(case)
    assert float(e["y"].abs().max()) * 256 < 65504
    dv = lambda t: None if t is None else t.to(dev)
    y = nhwc(e["y"]).reshape(N, H * W, 256)

    def run(parts, normalize):
        n = N * H * W * parts * 256
        buf = torch.full((2 * CC.GUARD + n,), BAND, dtype=torch.int16, device=dev)
        bank = buf[CC.GUARD:CC.GUARD + n].view(N, H * W, parts, 256)
        bank.fill_(POISON)
        with options(conv_debug=dbg):
            ops.conv_split_to_bank(dv(e["xs"]), dv(e["w"]), dv(e["bias"]), H, W, True, bank, residual=dv(e["residual"]), in_fmt=CC.FMT[arith],
                                   in_scale_log2=e["in_scale"], normalize=normalize)
            torch.cuda.synchronize()
        assert bool((buf[:CC.GUARD] == BAND).all()) and bool((buf[CC.GUARD + n:] == BAND).all()), "stores outside the bank"
        return bank.cpu()

    for normalize in (False, True):
        bx = run(4, normalize)
        chan = ops.f32_of_f16f6x(bx).reshape(-1, 256)
        assert bool(torch.isfinite(chan).all())
        if normalize:
            want = y / y.norm(dim=2, keepdim=True).clamp_min(1e-12)
            err = (chan.double() - want.reshape(-1, 256)).abs()
            assert bool((err <= 8 * CC.U24 * want.reshape(-1, 256).abs() + 1e-30).all()), float(err.max())
        else:
            assert torch.equal(chan.double(), y.reshape(-1, 256))
        rows = torch.from_numpy(O.f16f6p_encode(chan.numpy())).view(torch.int16).reshape(N, H * W, 2, 256)
        assert torch.equal(bx[:, :, :2], rows), (case, normalize, "f16f6x: the first KiB")
        bp = run(2, normalize)
        assert torch.equal(bp, rows), (case, normalize, "f16f6p rows")
        h, h6, l6 = O.f16f6p_decode(bp.reshape(-1, 2, 256).view(torch.uint8).reshape(-1, 1024).numpy())
        assert np.array_equal(h, (chan.numpy() * np.float32(256)).astype(np.float16).astype(np.float64))


# ----------------------------------------------------------------------------------------------------------------------
# conv64
# ----------------------------------------------------------------------------------------------------------------------
def launch_conv64(dev, arith, N, H, W, e, res_kind, relu, out_fmt, so, f32, variant, what):
    from fgvc_amd import ops
    fmt = CC.FMT[arith]
    w = torch.from_numpy(CC.pack_conv64(e["w"]) if fmt == 0 else CC.pack_conv64_f16(e["w"])).to(dev)
    of = F32Out(dev, (N, H, W, 64)) if f32 else None
    os_ = SplitOut(dev, N, 64, H, W)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    r32 = e["residual"].to(dev) if res_kind == "f32" else None
    rs = CC.pack_act(e["residual"].permute(0, 3, 1, 2), 0).to(dev) if res_kind == "split" else None
    with options(conv64_variant=variant):
        ops.conv64_split(e["xs"].to(dev), w, e["bias"].to(dev), H, W, relu, residual=r32, out_split=os_.view, out_f32=of.view if f32 else None,
                         residual_split=rs, in_fmt=fmt, in_scale_log2=e["in_scale"], out_fmt=out_fmt, out_scale_log2=so, overflow=ovf)
        torch.cuda.synchronize()
    assert int(ovf.item()) == 0, (what, "overflow word")
    return (of.check(what) if f32 else None), os_


@pytest.mark.parametrize("c", CC.conv64_cases(), ids=lambda c: c[-1])
def test_conv64_exact(dev, c):
    """conv64_kernel<0>, <1>, conv64k_kernel and the four conv64p_kernel forms (4 x 32 tiles on min(tiles, 256) persistent workgroups) at
    1, 12, 255, 256, 257 and 513 tiles -- one tile, fewer tiles than workgroups, grid - 1, grid, grid + 1, 2 grid + 1 -- in factorisations
    that vary images, rows and columns, with ragged last tiles; the residual as f32 and as a split tensor."""
    arith, N, H, W, res_kind, relu, out_fmt, f32, variant, name = c
    e = CC.exact_conv64(c)
    of = CC.FMT[out_fmt]
    assert res_kind != "split" or bool((e["residual"].bfloat16().float() == e["residual"]).all())      # hi + lo of the split identity IS the f32 identity
    got, os_ = launch_conv64(dev, arith, N, H, W, e, res_kind, relu, of, CC.EXACT_OUT_SCALE, f32, variant, name)
    if got is not None:
        assert_bit_exact(got, e["y"], name)
    src = got if got is not None else nhwc(e["y"]).float()
    os_.check(CC.expected_split(src, of, CC.EXACT_OUT_SCALE), name)


# ----------------------------------------------------------------------------------------------------------------------
# stride 2
# ----------------------------------------------------------------------------------------------------------------------
def launch_s2(dev, form, N, H, W, Cout, e, relu, proj_relu, out_fmt, so, what):
    from fgvc_amd import ops
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    of, os_ = F32Out(dev, (N, Ho, Wo, Cout)), SplitOut(dev, N, Cout, Ho, Wo)
    o2 = F32Out(dev, (N, Ho, Wo, Cout)) if form == "p" else None
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    proj = None
    if form == "p":
        proj = (torch.from_numpy(CC.pack_conv_s2(e["proj"]["w"])).to(dev), e["proj"]["bias"].to(dev), o2.view)
    ops.conv_s2_split(e["xs"].to(dev), torch.from_numpy(CC.pack_conv_s2(e["w"])).to(dev), e["bias"].to(dev), H, W, relu, out_split=os_.view,
                      out_f32=of.view, out_fmt=out_fmt, out_scale_log2=so, overflow=ovf, proj=proj, proj_relu=proj_relu)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0, (what, "overflow word")
    return of.check(what), os_, (o2.check(what + " projection") if o2 is not None else None)


@pytest.mark.parametrize("c", CC.s2_cases(), ids=lambda c: c[-1])
def test_conv_s2_exact(dev, c):
    """conv_s2_kernel<3>, <1> and <3, true> (the projection in the same launch, both ReLU flags), each at every H in 1, 2, 7, 8, 9 with every
    W in 1, 2, 63 .. 66 -- the last input row / column read or not, ragged 4 x 32 output tiles, inputs smaller than a tile's reach -- Cin 32 / 64 / 128,
    Cout 32 / 96 / 128 / 256, the split output in each format in turn."""
    form, N, Cin, Cout, H, W, relu, proj_relu, name = c
    e = CC.exact_s2(c)
    out_fmt = (H + W + Cout // 32) % 4
    got, os_, got2 = launch_s2(dev, form, N, H, W, Cout, e, relu, proj_relu, out_fmt, CC.EXACT_OUT_SCALE, name)
    assert_bit_exact(got, e["y"], name)
    os_.check(CC.expected_split(got, out_fmt, CC.EXACT_OUT_SCALE), name)
    if got2 is not None:
        assert_bit_exact(got2, e["proj"]["y"], name + " projection")


# ----------------------------------------------------------------------------------------------------------------------
# the stem
# ----------------------------------------------------------------------------------------------------------------------
def launch_stem7(dev, x, w, bias, relu, out_fmt, so, what):
    from fgvc_amd import ops
    N, _, H, W = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    of, os_ = F32Out(dev, (N, Ho, Wo, 64)), SplitOut(dev, N, 64, Ho, Wo)
    ovf = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.stem7_split(x.to(dev), w.to(dev), bias.to(dev), relu, out_split=os_.view, out_f32=of.view, out_fmt=out_fmt, out_scale_log2=so, overflow=ovf)
    torch.cuda.synchronize()
    assert int(ovf.item()) == 0, (what, "overflow word")
    return of.check(what), os_


@pytest.mark.parametrize("c", CC.stem7_cases(), ids=lambda c: c[-1])
def test_stem7_exact(dev, c):
    """stem7_kernel (4 x 32 output tiles on min(tiles, 512) persistent workgroups): images smaller than the 7 x 7 window, odd and even
    sizes on both sides of a tile, 511, 512, 513 and 1025 tiles; f32 + bf16 split and f32 + f16f8 split outputs."""
    N, H, W, relu, out_fmt, name = c
    e = CC.exact_stem7(c)
    of = CC.FMT[out_fmt]
    got, os_ = launch_stem7(dev, e["x"], e["w"], e["bias"], relu, of, CC.EXACT_OUT_SCALE, name)
    assert_bit_exact(got, e["y"], name)
    os_.check(CC.expected_split(got, of, CC.EXACT_OUT_SCALE), name)


# ----------------------------------------------------------------------------------------------------------------------
# realistic cases: rho_kernel <= 4 rho_emu
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.REALISTIC, ids=CC.realistic_id)
def test_realistic_rho(dev, c):
    """The rows the trunk produces through every kernel that takes the case: conv_split_kernel (and, where the launch has two forms, the
    other one: PINNED / compiler-scheduled bf16x3, conv256p_kernel / conv_split_kernel f16f6), conv64_kernel<0 | 1>, conv64p_kernel,
    conv64k_kernel, conv_s2_kernel<3 | 1>, stem7_kernel.  The split output is the packer's encoding of the kernel's own f32 output."""
    from fgvc_amd import ops
    k, arith, Cin, Cout, KS, N, H, W, rows, res, relu = c
    r = CC.realistic(c)
    name = CC.realistic_id(c)
    fmt = r["fmt"]
    y, A = nhwc(r["y"]), nhwc(r["A"])
    so = ops.act_scale_log2(float(r["y"].abs().max())) if fmt else 0
    if k == "split":
        for dbg, kernel in ((0, "conv_split_pinned" if (fmt == 0 and KS == 3 and Cout % 256 == 0) else "conv256p" if (fmt == 3 and KS == 3 and Cout % 128 == 0) else "conv_split"),
                            (16, "conv_split"), (1024, "conv_split")):
            if (dbg == 16 and not (fmt == 0 and KS == 3 and Cout % 256 == 0)) or (dbg == 1024 and not (fmt == 3 and KS == 3 and Cout % 128 == 0)):
                continue
            cc = dict(arith=arith, N=N, H=H, W=W, Cout=Cout, relu=relu, debug=dbg, id=name)
            got, os_ = launch_split(dev, cc, r, fmt, so, True)
            record(kernel, arith, CC.rho(got, y, A), r["rho_emu"], name)
            os_.check(CC.expected_split(got, fmt, so), name)
    elif k == "c64":
        forms = [(0, "conv64_kernel<0>")] if fmt == 0 else [(0, "conv64p" if res else "conv64_kernel<1>"), (16, "conv64_kernel<1>"), (32, "conv64k")]
        for variant, kernel in forms:
            got, os_ = launch_conv64(dev, arith, N, H, W, r, "f32" if res else None, relu, fmt, so, True, variant, name)
            record(kernel, arith, CC.rho(got, y, A), r["rho_emu"], name)
            os_.check(CC.expected_split(got, fmt, so), name)
    elif k == "s2":
        got, os_, _ = launch_s2(dev, KS, N, H, W, Cout, r, relu, False, 0, 0, name)
        record(f"conv_s2<{KS}>", arith, CC.rho(got, y, A), r["rho_emu"], name)
        os_.check(CC.expected_split(got, 0, 0), name)
    else:
        w = torch.from_numpy(CC.pack_stem7(*r["w"]))
        got, os_ = launch_stem7(dev, r["x"], w, r["bias"], relu, 0, 0, name)
        record("stem7", arith, CC.rho(got, y, A), r["rho_emu"], name)
        os_.check(CC.expected_split(got, 0, 0), name)


def test_options_restored_and_report(dev):
    """After every override above the options are back at their defaults: a launch that sets nothing equals, bit for bit, the same launch
    with the defaults set explicitly.  Prints the rho table."""
    c = dict(arith="f16f6", H=9, W=33, N=1, Cin=64, Cout=128, KS=3, res=True, relu=True, id="closing")
    e = CC.exact_split(c)
    a, sa = launch_split(dev, dict(c, narrow=DEFAULTS["conv_narrow"]), e, 3, 0, True)
    b, sb = launch_split(dev, c, e, 3, 0, True, set_options=False)          # whatever the tests above left in force
    assert torch.equal(a, b) and torch.equal(sa.view.cpu(), sb.view.cpu())
    assert_bit_exact(b, e["y"], "closing")
    print("largest rho_kernel / rho_emu per kernel and arithmetic (bar: 4):")
    for (kernel, arith), (ratio, rk, re_, what) in sorted(STATS.items()):
        print(f"  {kernel:18s} {arith:7s} ratio {ratio:.3f}  rho_kernel {rk:.3f}  rho_emu {re_:.3f}  ({what})")
