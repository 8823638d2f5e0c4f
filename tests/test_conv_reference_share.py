"""CPU: what tests/test_gpu_conv_ops.py relies on, checked from the restatements alone (tests/conv_cases.py).

* The decoders are the inverse of the packers, byte for byte both ways: every row ops.prepare_conv_split / prepare_conv_split_f16 and
  the host statement of the epilogues (conv_cases.pack_values: split_bf16_4, split_f16_4, split_f16f6_chunk) make decodes and encodes
  back to itself, and planted parts encode and decode back to themselves; the operand-ordered weight tensors of prepare_conv64 /
  prepare_conv64_f16 / prepare_conv_s2 / prepare_stem7 are re-ordered copies of the canonical rows, index by index.
* Every exact case the GPU module runs satisfies A < 2^24 q at every entry (conv_cases' docstring: then any order of f32 additions
  is exact and tolerance zero is derived, not hoped for).
* Part 2 of the bounds -- the FORMAT's error, model64 against the float64 convolution of the exact operands: bf16x3 within
  2.0001 * 2^-16 A0 on every entry (volume_cases' derivation, the same split), the f16 forms within conv_cases.format_bound on every
  entry (half a unit of each narrow format per operand, summed over the products); the project's flat bars hold as well, which is all
  those bars are asked to carry from now on.
* Sensitivity: every mutant model differs from model64 by more than twice the bar 4 rho_emu 2^-24 A on at least one entry of every
  realistic case it applies to; the test prints which of them the old flat bars would have passed (docs/LAB_NOTES.md has the table).
* By arithmetic on the shapes, the case tables reach what they name.
"""
import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import conv_cases as CC
from tests import volume_cases as VC


def _layer(Cout, Cin, KS, seed=0):
    return CC.realistic_layer(Cout, Cin, KS, seed)


# ----------------------------------------------------------------------------------------------------------------------
# decoders against packers
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arith", CC.ARITHS)
def test_rows_round_trip_both_ways(arith):
    from fgvc_amd import ops
    fmt = CC.FMT[arith]
    # packers -> parts -> the same bytes: activation rows (heavy-tailed with zeros and an all-zero chunk, Gaussian with negative values
    # that round to a negative zero code) and weight rows
    for kind, C in (("relu", 64), ("gauss", 32)):
        x = CC.realistic_x(kind, 2, C, 5, 9, 3)
        sx = ops.act_scale_log2(float(x.abs().max())) if fmt else 0
        rows = CC._rows_u8(CC.pack_act(x, fmt, sx))
        assert np.array_equal(CC.act_rows(CC.act_parts(rows, fmt), fmt), rows), (arith, kind)
    wt, bn = _layer(96, 64, 3)
    w = ops.prepare_conv_split(wt, bn)[0] if fmt == 0 else ops.prepare_conv_split_f16(wt, bn, fmt)[0]
    rows = CC._rows_u8(w.detach())
    assert np.array_equal(CC.w_rows(CC.w_parts(rows, fmt), fmt), rows), arith
    # planted parts -> bytes -> the same parts
    rng = np.random.default_rng(5)
    for weight, enc, dec in ((False, CC.act_rows, CC.act_parts), (True, CC.w_rows, CC.w_parts)):
        p = CC.exact_parts(fmt, (3, 7, 2, 32), rng, weight)
        back = dec(enc(p, fmt), fmt)
        assert set(back) == set(p)
        for k in p:
            assert np.array_equal(np.asarray(back[k], np.float64), np.asarray(p[k], np.float64)), (arith, weight, k)
    # the narrow copies are planted DIFFERENT from what the format would derive from h
    if fmt == 1:
        assert (p["h8"] != CC._e4m3_round((p["h"] * 2.0 ** -CC.F8_AW).astype(np.float32))).mean() > 0.5
    if fmt == 3:
        assert (p["h6"] != p["h"]).mean() > 0.5


def test_activation_decoders_agree_with_the_projects_own():
    """act_parts against ops.unsplit_act (h + l) and oracle.act_f16f6_decode on packed rows"""
    from fgvc_amd import ops
    x = CC.realistic_x("relu", 1, 64, 4, 6, 11)
    for arith, fmt in CC.FMT.items():
        sx = ops.act_scale_log2(float(x.abs().max())) if fmt else 0
        xs = CC.pack_act(x, fmt, sx)
        p = CC.act_parts(CC._rows_u8(xs), fmt)
        lo = {0: lambda: p["lo"], 1: lambda: p["l8"] * 2.0 ** -CC.F8_BX, 2: lambda: p["l"], 3: lambda: p["l6"]}[fmt]()
        mine = (p["hi" if fmt == 0 else "h"] + lo) * 2.0 ** -sx
        theirs = ops.unsplit_act(xs, fmt, sx).double().numpy().reshape(mine.shape)
        assert np.allclose(mine, theirs, rtol=1e-6, atol=1e-12), arith
        if fmt == 3:
            h, h6, l6 = O.act_f16f6_decode(CC._rows_u8(xs).reshape(-1, 128))
            assert np.array_equal(h6, p["h6"].reshape(-1, 32)) and np.array_equal(l6, p["l6"].reshape(-1, 32)) and np.array_equal(h, p["h"].reshape(-1, 32))
    # the f16f8 scales: l8 carries 2^BX l, h8 carries 2^-AX h; the cross products enter at 2^(AW - BX) and 2^(AX - BW)
    assert CC.terms_of(1)[1][2] == 0.5 and CC.terms_of(1)[2][2] == 0.25
    assert (CC.F8_AX, CC.F8_BX, CC.F8_AW, CC.F8_BW) == (ops.F8_AX, ops.F8_BX, ops.F8_AW, ops.F8_BW)


def test_operand_ordered_weight_layouts():
    from fgvc_amd import ops
    wt, bn = _layer(64, 64, 3, 1)
    canon = ops.prepare_conv_split(wt, bn)[0].detach()
    w64 = ops.prepare_conv64(wt, bn)[0].detach()
    assert np.array_equal(CC.unpack_conv64(w64), CC._np16(canon)) and np.array_equal(CC.pack_conv64(canon), CC._np16(w64))
    canon8 = ops.prepare_conv_split_f16(wt, bn, ops.ACT_F16F8)[0].detach()
    w8 = ops.prepare_conv64_f16(wt, bn)[0].detach()
    assert np.array_equal(CC.unpack_conv64_f16(w8), CC._np16(canon8)) and np.array_equal(CC.pack_conv64_f16(canon8), CC._np16(w8))
    for Cout, Cin, KS in ((96, 64, 3), (32, 32, 1), (256, 128, 3)):
        wt, bn = _layer(Cout, Cin, KS, 2)
        canon = ops.prepare_conv_split(wt, bn)[0].detach()
        ws2 = ops.prepare_conv_s2(wt, bn)[0].detach()
        assert np.array_equal(CC.unpack_conv_s2(ws2), CC._np16(canon)) and np.array_equal(CC.pack_conv_s2(canon), CC._np16(ws2))
    wt, bn = _layer(64, 3, 7, 3)
    w7 = ops.prepare_stem7(wt, bn)[0].detach()
    hi, lo, blocks = CC.unpack_stem7(w7)
    b = blocks.reshape(64, 7, 8, 4, 2)
    assert not b[:, :, 7].any() and not b[:, :, :, 3].any()                      # kx = 7 and c = 3 are zero
    scale = (bn.weight / torch.sqrt(bn.running_var + bn.eps)).detach().float()
    wfold = (wt.float() * scale.view(-1, 1, 1, 1)).detach().numpy()
    want = VC.split_bf16_model(wfold.reshape(-1, 1)).view(np.uint16)
    assert np.array_equal(hi.ravel(), CC._bf16_dec(want[:, 0, 0])) and np.array_equal(lo.ravel(), CC._bf16_dec(want[:, 1, 0]))
    assert np.array_equal(CC.pack_stem7(hi, lo), CC._np16(w7))


def test_host_epilogue_formats():
    """pack_values: bf16 is volume_cases' split; f16f6 is the oracle's rows; f16f8 / f16x3 reproduce the value to the format's step"""
    g = torch.Generator().manual_seed(2)
    y = (torch.randn(50, 32, generator=g) * 40).numpy()
    y[3] = 0
    for fmt, tol in ((0, 2.0 ** -16), (1, 2.0 ** -15), (2, 2.0 ** -21), (3, 2.0 ** -13)):
        rows = CC.pack_values(y, fmt, 2)
        p = CC.act_parts(rows, fmt)
        lo = {0: lambda: p["lo"], 1: lambda: p["l8"] * 2.0 ** -CC.F8_BX, 2: lambda: p["l"], 3: lambda: p["l6"]}[fmt]()
        back = (p["hi" if fmt == 0 else "h"] + lo) * (1.0 if fmt == 0 else 0.25)
        assert np.abs(back - y).max() <= tol * np.abs(y).max(), (fmt, np.abs(back - y).max() / np.abs(y).max())


# ----------------------------------------------------------------------------------------------------------------------
# exact cases: A < 2^24 q everywhere
# ----------------------------------------------------------------------------------------------------------------------
def _assert_exact(e, name):
    q, A, y = e["q"], e["A"], e["y"]
    assert q is not None and q == 2.0 ** round(np.log2(q)) and q >= 2.0 ** -20, (name, q)
    assert float(A.max()) < 2.0 ** 24 * q, (name, float(A.max()), q)
    assert bool((torch.round(y / q) * q == y).all()) and bool((y.float().double() == y).all()), name        # multiples of q; f32 holds them
    assert float(A.max()) > 0
    return float(A.max()) / (2.0 ** 24 * q)


def test_exact_cases_are_exact_in_f32():
    worst = {}
    for kind, cases, build, ident in (("split", CC.split_cases(), CC.exact_split, lambda c: c["id"]),
                                      ("conv256p", CC.conv256p_cases(), CC.exact_split, lambda c: c["id"]),
                                      ("proj", CC.proj_cases(), CC.exact_split, lambda c: c["id"]),
                                      ("bank", CC.BANK_CASES, CC.exact_bank, str), ("s2", CC.s2_cases(), CC.exact_s2, lambda c: c[-1])):
        for c in cases:
            e = build(c)
            r = _assert_exact(e, ident(c))
            if "proj" in e:
                r = max(r, _assert_exact(e["proj"], ident(c) + "-proj"))
            worst[kind] = max(worst.get(kind, 0.0), r)
    for c in CC.conv64_cases():
        worst["c64"] = max(worst.get("c64", 0.0), _assert_exact(CC.exact_conv64(c), c[-1]))
    for c in CC.stem7_cases():
        worst["stem7"] = max(worst.get("stem7", 0.0), _assert_exact(CC.exact_stem7(c), c[-1]))
    print("largest A / (2^24 q) per family:", {k: f"{v:.4f}" for k, v in worst.items()})
    assert max(worst.values()) < 1.0
    # ... and the densest sum the tables ask for is among them: Cin = 256 with 3 x 3 taps
    assert any(c["Cin"] == 256 and c["KS"] == 3 for c in CC.split_cases())


# ----------------------------------------------------------------------------------------------------------------------
# realistic cases: the format half, the bar, the mutants
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CC.REALISTIC, ids=CC.realistic_id)
def test_format_bounds_and_mutants(c):
    r = CC.realistic(c)
    arith = c[1]
    y, A, ref = r["y"], r["A"], r["ref64"]
    ymax = float(ref.abs().max())
    err = (y - ref).abs()
    if arith == "bf16x3":
        bound = VC.BF16X3_FORMAT * r["A0"]
        assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    else:                                                # the f16 forms: the bound derived from the formats in conv_cases.format_bound
        bound = CC.format_bound(r)
        worst = float((err / bound.clamp_min(1e-300))[bound > 0].max())
        print(f"{CC.realistic_id(c)}: largest |model64 - conv2d64| / format bound {worst:.3f}; the bound is at most {float(bound.max()) / ymax:.2e} of max|y|")
        assert bool((err <= bound * (1 + 1e-9) + 1e-300).all()), worst
    assert float(err.max()) < CC.OLD_BARS[arith] * ymax, (float(err.max()) / ymax)
    assert 0.2 < r["rho_emu"] < 16.0, r["rho_emu"]       # an f32 chain of a few hundred additions: a few units of 2^-24 A
    bar = CC.BAR_FACTOR * r["rho_emu"] * CC.U24 * A
    assert float((r["emu"].double() - y).abs().max()) < CC.OLD_BARS[arith] * ymax / 8            # the bar itself lies far inside the old one
    line = []
    for name, m in CC.mutants(r["cv"]).items():
        d = (CC.model64_mutant(m) - y).abs()
        ratio = float((d / bar.clamp_min(1e-300))[A > 0].max())
        old = float(d.max()) / ymax
        line.append(f"{name} {ratio:.1f} x bar, {old:.1e} of max|y| ({'PASSES' if old < CC.OLD_BARS[arith] else 'fails'} the old bar)")
        assert ratio > 2.0, (name, ratio)
    print(f"{CC.realistic_id(c)}: rho_emu {r['rho_emu']:.2f}, model vs conv2d64 {float(err.max()) / ymax:.2e} of max|y|; " + "; ".join(line))
    names = set(CC.mutants(r["cv"]))
    assert {"cross_sum_dropped_one_tap_one_chunk", "main_kstep_dropped_one_tap", "bias_shifted_one_channel"} <= names
    assert ("h_in_place_of_narrow_h" in names) == (arith in ("f16f8", "f16f6")) and ("fp6_scales_exchanged" in names) == (arith == "f16f6")
    assert ("ky_kx_transposed" in names) == (c[4] > 1) and ("residual_of_the_neighbouring_pixel" in names) == bool(c[9])


def test_emu32_is_the_model_on_an_exact_case():
    c = dict(arith="f16f6", H=5, W=9, N=1, Cin=64, Cout=64, KS=3, res=True, relu=False, id="emu-exact")
    e = CC.exact_split(c)
    assert torch.equal(CC.emu32(e["cv"]).double(), e["y"]) and CC.rho(e["y"], e["y"], e["A"]) == 0.0


# ----------------------------------------------------------------------------------------------------------------------
# the tables reach what they name
# ----------------------------------------------------------------------------------------------------------------------
def test_tables_cover_their_axes():
    sc = CC.split_cases()
    assert len({c["id"] for c in sc}) == len(sc)
    routes = CC.split_routes()
    assert set(routes) == {(3, 256, False), (3, 128, True), (3, 128, False), (3, 64, True), (3, 64, False),
                           (1, 256, False), (1, 128, False), (1, 64, True), (1, 64, False)}
    # every value of every axis with every kernel instance it can reach: per (arithmetic, instance [, PINNED | compiler-scheduled])
    for arith in CC.ARITHS:
        insts = {c["inst"] for c in sc if c["arith"] == arith}
        assert insts == {i + (False,) for i in routes} | ({(3, 256, False, True)} if arith == "bf16x3" else set()), arith
        for inst in insts:
            mine = [c for c in sc if c["arith"] == arith and c["inst"] == inst]
            what = (arith, inst)
            assert all(CC.split_instance(c["KS"], c["Cout"], c["cot_cap"], c["narrow"]) == inst[:3] for c in mine), what
            assert all(c["debug"] == (1024 if arith == "f16f6" else 16 if inst[3] else 0) for c in mine), what
            assert [(c["H"], c["W"]) for c in mine] == CC.HW_EDGES, what
            assert {c["N"] for c in mine} == {1, 3} and {c["Cin"] for c in mine} == set(CC.SPLIT_CIN), what
            reach = routes[inst[:3]]
            for k, key in enumerate(("Cout", "cot_cap", "narrow")):
                assert {c[key] for c in mine} == {r[k] for r in reach}, (what, key)
            assert {c["out_fmt"] for c in mine} == set(CC.ARITHS) and {c["res"] for c in mine} == {False, True} == {c["relu"] for c in mine}, what
    assert {c["Cout"] for c in sc} == set(CC.SPLIT_COUT) and {c["cot_cap"] for c in sc} == set(CC.SPLIT_CAP) and {c["narrow"] for c in sc} == set(CC.SPLIT_NARROW)
    # the options' defaults the GPU module puts back are the library's own (the C ABI has no getter: read from the sources)
    import os
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fgvc_amd", "csrc")
    text = open(os.path.join(csrc, "conv_split.hip")).read() + open(os.path.join(csrc, "conv64.hip")).read()
    for name, value in CC.OPTION_DEFAULTS.items():
        m = re.search(r"static int g_%s = (-?\d+);" % name, text)
        assert m and int(m.group(1)) == value, name
    forms = {c["form"] for c in CC.conv256p_cases()}
    assert len(forms) == 10
    for f in forms:
        mine = [c for c in CC.conv256p_cases() if c["form"] == f]
        assert [(c["H"], c["W"]) for c in mine] == CC.HW_EDGES
        assert {c["Cin"] for c in mine} == {"c256_f6_cin128": {128}, "c256_f6": {32, 256}}.get(f, {32, 128, 256}), f
    assert {c["Cin"] for c in CC.conv256p_cases()} == {32, 128, 256}
    assert {(c["H"], c["W"]) for c in CC.conv256p_cases()} == set(CC.HW_EDGES)
    # conv_split_launch's own selection, restated: (COT, specialised f16f6 epilogue, residual, f32 out, the Cin = 128 loop)
    def inst256(c):
        cot = min(256 if c["Cout"] % 256 == 0 else 128, c["cot_cap"] or 256)
        special = c["out_fmt"] == "f16f6" and not (c["f32"] and not c["res"] and cot == 128)
        if not special:
            return cot, -1, False, False, 0
        return cot, 3, c["res"], c["f32"], int(cot == 256 and not c["res"] and not c["f32"] and c["Cin"] == 128)
    want = {"c256_f6_cin128": (256, 3, False, False, 1), "c256_f6": (256, 3, False, False, 0), "c256_f6_f32": (256, 3, False, True, 0),
            "c256_f6_res_f32": (256, 3, True, True, 0), "c256_f6_res": (256, 3, True, False, 0), "c256_generic": (256, -1, False, False, 0),
            "c128_f6": (128, 3, False, False, 0), "c128_f6_res_f32": (128, 3, True, True, 0), "c128_f6_res": (128, 3, True, False, 0),
            "c128_generic": (128, -1, False, False, 0)}
    for c in CC.conv256p_cases():
        assert inst256(c) == want[c["form"]], c["id"]
    assert all(c["Cin"] == 128 for c in CC.conv256p_cases() if c["form"] == "c256_f6_cin128")
    assert all(c["Cin"] != 128 for c in CC.conv256p_cases() if c["form"] == "c256_f6")
    assert len({c["id"] for c in CC.proj_cases()}) == len(CC.proj_cases()) and sum(c["debug"] == 1024 for c in CC.proj_cases()) == 3
    assert {c["Cin2"] for c in CC.proj_cases()} == {32, 64, 128} and {c["arith"] for c in CC.proj_cases()} == set(CC.ARITHS)
    # persistent kernels: one tile, grid - 1, grid, grid + 1, 2 grid + 1; ragged last tiles; N, rows and columns all vary
    t64 = [CC.tiles64(*s) for s in CC.CONV64_SHAPES]
    assert {1, 255, 256, 257, 513} <= set(t64) and t64[1] == 3 * 2 * 2
    assert any(H % 4 and W % 32 for _, H, W in CC.CONV64_SHAPES) and {N for N, _, _ in CC.CONV64_SHAPES} >= {1, 255, 257}
    t7 = [CC.stem7_tiles(*s) for s in CC.STEM7_SHAPES]
    assert {1, 511, 512, 513, 1025} <= set(t7), t7
    assert (1, 1, 1) in CC.STEM7_SHAPES and (1, 3, 5) in CC.STEM7_SHAPES
    assert {c[4] for c in CC.stem7_cases()} == {"bf16x3", "f16f8"}
    s2 = CC.s2_cases()
    assert len({c[-1] for c in s2}) == len(s2)
    for form in (3, 1, "p"):
        mine = [c for c in s2 if c[0] == form]
        assert sorted((c[4], c[5]) for c in mine) == sorted((h, w) for h in CC.S2_H for w in CC.S2_W)
        assert {(c[2], c[3]) for c in mine} == {(a, b) for a in CC.S2_CIN for b in CC.S2_COUT}
    assert {(c[6], c[7]) for c in s2 if c[0] == "p"} == {(False, False), (False, True), (True, False), (True, True)}
    assert CC.GUARD % 4 == 0
