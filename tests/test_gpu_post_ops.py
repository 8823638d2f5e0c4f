"""GPU: the kernels of csrc/post.hip against plain float64 evaluations of the same operations on the CPU (tests/post_cases.py).

Run on an MI355X with `pytest -m gpu`.  What each group pins:

* read-out (softargmax_pruned_kernel, softargmax_band_kernel, softargmax_merge_kernel): every case on BOTH routes (`readout_prune` 0 and
  the default), each held to the float64 restatement and not to the other route: ragged ratios, scale 8, identity, downsampling, bumps
  on the clamped border rows and in the corners, the tie rule at rank 5, the -1 rule, negative labels (the scan fallback), the analytic
  first frame, exact-arithmetic maps, and a geometry that skips coarse rows;
* merge (merge_topk_kernel<1|5|10|16>) from synthetic lists: every topk 1..16 (all `kout < K` instantiations, the 8-byte-load path of
  full even lists next to the generic one), unused slots, short lists, a pair in two slots;
* propagate (propagate_kernel): permuted and repeated slot_frame, idx < 0, window taps outside the image, P 1..40;
* Gaussian labels, normalise (the large-LDS branch, eps, raw mode, padding), BN (vector / scalar path, the grid-stride loop).

Read-out coordinates are compared on the CHECKABLE maps (tests/post_cases.py: clear gap at rank 5, structural tie or zero map), at least
95 % of every case; tests/test_post_reference_share.py shows the same shares and the tolerance from the reference alone.  Every other
bound is derived in the docstring of its test.  Each test prints its measured maximum next to the bound.
"""
import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import post_cases as PC

pytestmark = pytest.mark.gpu
U = 2.0 ** -24            # unit roundoff of f32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()          # the HIP library must be the thing under test: fail loudly if it is missing
    return torch.device("cuda:0")


def _ulp32(x: torch.Tensor) -> torch.Tensor:
    x = x.float().abs()
    return (torch.nextafter(x, torch.full_like(x, float("inf"))) - x).double()


def both_routes(fn):
    """[(route name, fn())] with the pruned read-out off, then on (the default, restored whatever happens)."""
    from fgvc_amd import ops
    out = []
    try:
        for prune in (0, 1):
            ops.set_option("readout_prune", prune)
            out.append(("pruned" if prune else "band", fn()))
    finally:
        ops.set_option("readout_prune", 1)
    return out


def hold(what, got, want, tol):
    """got (T, P, 2) against the restatement on its checkable maps; zero maps exactly -1"""
    ck = want["checkable"].numpy()
    share = float(ck.mean())
    err = np.abs(got - want["coords"]).max(-1)
    worst = float(err[ck].max())
    print(f"{what}: checkable {int(ck.sum())}/{ck.size} = {share:.4f}, max err {worst:.3e} px (tol {tol:.3e})")
    assert share >= PC.MIN_SHARE, (what, share)
    assert worst <= tol, (what, worst, np.argwhere(ck & (err > tol)).tolist())
    zero = want["zero"].numpy()
    assert np.array_equal(got[zero], np.full((int(zero.sum()), 2), -1.0)), what
    assert not bool((got[~zero] == -1.0).all(-1).any()), what


# ======================================================================================================================
# 1. read-out
# ======================================================================================================================
@pytest.mark.parametrize("case", PC.READOUT, ids=PC.case_id)
def test_readout_matches_float64_restatement(dev, case):
    """fgvc_softargmax_top5_f32 on both routes against img2coord of the float64 field.  Tolerance: tests/test_gpu_heatmap.py::_tol(False, .)
    (1e-5 px + 4 ulps of the largest coordinate), which tests/test_post_reference_share.py shows the reference's f32 pipeline to meet
    on the same maps."""
    from fgvc_amd import ops
    name, T, Hf, Wf, P, h, w = case
    labels = PC.readout_labels(case)
    want = PC.readout_want(case, labels)
    lab_d = labels.to(dev)
    for route, got in both_routes(lambda: ops.softargmax_top5(lab_d, Hf, Wf, h, w).cpu().numpy()):
        assert got.shape == (T, P, 2) and got.dtype == np.float64
        hold(f"read-out {name} {route}", got, want, PC.readout_tol(h, w))
        if name.startswith("special"):
            assert np.array_equal(got[:, 8], np.full((T, 2), -1.0))               # the all-zero channel
            assert bool((got[:, 9] >= 0).all())                                   # negative values, non-zero sum: a coordinate
            assert bool(want["structural"][:, :8].any())                          # border bumps: ties between replicated rows


@pytest.mark.parametrize("name", ["base", "odd"])
def test_readout_first_frame_points(dev, name):
    """gauss_points: frame 0 is the analytic Gaussian of the f32 points (inside, x.5 / y.5, on the border, 3 px outside, far outside =
    exactly -1), frames >= 1 the bilinear field.  expf and the distance arithmetic move a top-5 value by a few 1e-7 relative, a
    coordinate by that times the spread of the five pixels (<= 2 px): far inside the read-out tolerance."""
    from fgvc_amd import ops
    case = next(c for c in PC.READOUT if c[0] == name)
    _, T, Hf, Wf, _, h, w = case
    pts, exact, far = PC.readout_points(h, w)
    P = pts.shape[0]
    labels = PC.readout_labels((name, T, Hf, Wf, P, h, w))
    want0 = PC.first_frame_want(pts, exact, h, w)
    rest = PC.readout_picks(PC.field(labels[1:], Hf, Wf, h, w), PC.axis_class(Hf, h), PC.axis_class(Wf, w))
    want = {k: (np.concatenate if k == "coords" else torch.cat)([want0[k], rest[k]], 0) for k in ("coords", "checkable", "zero")}
    lab_d, pts_d = labels.to(dev), pts.to(dev)
    for route, got in both_routes(lambda: ops.softargmax_top5(lab_d, Hf, Wf, h, w, gauss_points=pts_d, sigma=6.0).cpu().numpy()):
        hold(f"first frame {name} {route}", got, want, PC.readout_tol(h, w))
        assert np.array_equal(got[0][far.numpy()], np.full((int(far.sum()), 2), -1.0))
        assert bool(want0["checkable"].all())                                     # every centre of frame 0 is held


@pytest.mark.parametrize("case", PC.EXACT, ids=PC.case_id)
def test_readout_exact_arithmetic(dev, case):
    """Labels on multiples of 2^-8 and a power-of-two scale: the interpolation weights have at most 4 bits, every product and sum of
    fine_value is exact, the f32 field IS the float64 field (tests/test_post_reference_share.py) and all five picks are determined,
    ties included (the higher flat index stays).  So the comparison is with O.img2coord of the f32 field on EVERY map; what is left is
    one rounding of the top-5 sum and one of each quotient: 2 * 2^-24 * max(h, w) px."""
    from fgvc_amd import ops
    name, Hf, Wf, scale = case
    h, w = Hf * scale, Wf * scale
    lab = PC.exact_labels(case)
    ref = np.transpose(O.img2coord(PC.field(lab, Hf, Wf, h, w, torch.float32).numpy()), (2, 1, 0))
    lab_d = lab.to(dev)
    tol = 2 * U * max(h, w)
    for route, got in both_routes(lambda: ops.softargmax_top5(lab_d, Hf, Wf, h, w).cpu().numpy()):
        err = float(np.abs(got - ref).max())
        print(f"exact read-out {name} {route}: max err {err:.3e} px (tol {tol:.3e}), bit-equal {np.array_equal(got, ref)}")
        assert err <= tol, (name, route, err)


def test_readout_skipped_rows(dev):
    """24 x 32 -> 8 x 8: ratio 3 samples the source rows 3d + 1 only (lambda 0), ratio 4 the columns 4d + 1 and 4d + 2, so two thirds of
    the rows and half of the columns never reach an output pixel.  Channel 0: positive on skipped cells only, the field is all zero,
    the answer is -1 on both routes ("the map sums to zero" is a statement about the FIELD, not about the coarse map).  Channel 1: the
    same plus one sampled positive cell: ranks 2..5 are zeros of weight 0, so the coordinate is the same whichever zeros are picked.
    Channel 2: positive everywhere, large on the skipped cells."""
    from fgvc_amd import ops
    Hf, Wf, h, w = 24, 32, 8, 8
    g = torch.Generator().manual_seed(77)
    yy, xx = torch.meshgrid(torch.arange(Hf), torch.arange(Wf), indexing="ij")
    sampled = (yy % 3 == 1) & ((xx % 4 == 1) | (xx % 4 == 2))
    lab = torch.zeros(1, Hf, Wf, 3)
    lab[0, :, :, 0] = torch.where(sampled, torch.zeros(Hf, Wf), torch.rand(Hf, Wf, generator=g) + 0.5)
    lab[0, :, :, 1] = lab[0, :, :, 0]
    lab[0, 4, 9, 1] = 0.75
    lab[0, :, :, 2] = torch.where(sampled, torch.rand(Hf, Wf, generator=g) * 0.9 + 0.1, torch.full((Hf, Wf), 5.0))
    lab = lab.reshape(1, Hf * Wf, 3)
    want = PC.readout_picks(PC.field(lab, Hf, Wf, h, w), PC.axis_class(Hf, h), PC.axis_class(Wf, w))
    assert bool(want["zero"][0, 0]) and bool(want["checkable"][0, 2]) and not bool(want["zero"][0, 1])
    assert abs(want["coords"][0, 1, 0] - 2.0) < 1e-6 and abs(want["coords"][0, 1, 1] - 1.0) < 1e-6       # cell (4, 9) -> pixel (x 2, y 1)
    lab_d = lab.to(dev)
    for route, got in both_routes(lambda: ops.softargmax_top5(lab_d, Hf, Wf, h, w).cpu().numpy()):
        err = np.abs(got - want["coords"]).max(-1)[0]
        print(f"skipped rows {route}: got {got[0].tolist()} want {want['coords'][0].tolist()}")
        assert np.array_equal(got[0, 0], [-1.0, -1.0]), (route, got[0, 0])
        assert float(err.max()) <= PC.readout_tol(h, w), (route, err)


def test_readout_cell_bound_at_threshold(dev):
    """The pruned route lists the cells whose corner maximum B reaches tau, the 5th largest value AROUND the maximum.  Here (identity
    scale, every pixel is its cell's own corner) the map's true 5th value, 0.6003, is an isolated pixel far from the maximum whose cell
    has B = 0.6003, just above tau = 0.6: a list cut that drops cells with B within 0.1 % of tau loses it and still has five
    candidates, so nothing falls back to the full scan.  Ranks 5 and 6 are 3e-4 apart: a clear map."""
    from fgvc_amd import ops
    Hf, Wf = 24, 32
    lab = torch.zeros(1, Hf, Wf, 1)
    for (y, x), v in {(10, 10): 1.0, (10, 11): 0.9, (11, 10): 0.8, (11, 11): 0.7, (10, 9): 0.6, (20, 25): 0.6003}.items():
        lab[0, y, x, 0] = v
    lab = lab.reshape(1, Hf * Wf, 1)
    want = PC.readout_picks(PC.field(lab, Hf, Wf, Hf, Wf), PC.axis_class(Hf, Hf), PC.axis_class(Wf, Wf))
    assert bool(want["checkable"].all())
    lab_d = lab.to(dev)
    for route, got in both_routes(lambda: ops.softargmax_top5(lab_d, Hf, Wf, Hf, Wf).cpu().numpy()):
        err = float(np.abs(got - want["coords"]).max())
        print(f"cell bound at threshold {route}: got {got[0, 0].tolist()} want {want['coords'][0, 0].tolist()}")
        assert err <= PC.readout_tol(Hf, Wf), (route, err)


# ======================================================================================================================
# 2. merge
# ======================================================================================================================
@pytest.mark.parametrize("topk", list(range(1, 17)))
def test_merge_synthetic_lists(dev, topk):
    """fgvc_merge_topk_f32 from lists built on the host.  Scores are inputs, so the selection is exact: idx equals the canonical list
    (score desc, gid = slot * HWk + id asc) on EVERY row.  logit = score / temperature is one f32 division by f32(0.07): half an ulp
    for the quotient plus the 0.89 * 2^-24 relative distance of f32(0.07) from 0.07, within 2 ulps.  Softmax: the lists' scores keep
    every logit below 8 in size, so the quotient's rounding moves a logit by at most 2^-22 and an argument l_j - l_0 by twice that (the
    common factor of f32(0.07) changes a difference d by 5.3e-8 d, and d exp(-d) <= 0.37); a softmax weight moves by w (1 - w) <= 1 / 4
    of its argument's error, 2^-23; expf, the sum of at most topk terms and the division add a few 2^-24 each: topk * 2^-23 absolute
    (the arguments' share does not grow with topk, so topk = 2 is where the bound is closest).  Cosine: the square of a 2-ulp logit, 4 ulps relative.  Rows with
    fewer than topk candidates: the valid prefix as above (its softmax weights sum to 1), idx -1 behind it; the tail's logit and
    weight are not asserted (the reference has no such row)."""
    from fgvc_amd import ops
    HWk = PC.MERGE_HWK
    worst = dict(logit=0.0, softmax=0.0, cosine=0.0)
    short_rows = 0
    for T in PC.MERGE_T:
        for HWq in PC.MERGE_HWQ:
            for n_out in (1, 3):
                seed = topk * 1000 + T * 10 + n_out
                pi, ps = PC.merge_lists(T + 1, HWq, HWk, topk, seed + HWq)
                sp = PC.merge_slot_pairs(n_out, T, T + 1, seed)
                want = PC.merge_restated(pi, ps, sp, HWk, topk)
                valid = want["valid"]
                short_rows += int((~valid.all(-1)).sum())
                for mode in ("softmax", "cosine"):
                    idx, logit, weight = ops.merge_topk(pi.to(dev), ps.to(dev), sp.to(dev), HWk, topk, PC.TEMP, mode)
                    what = (topk, T, HWq, n_out, mode)
                    assert torch.equal(idx.cpu().long(), want["idx"]), what
                    lerr = (logit.cpu().double() - want["logit"]).abs() / _ulp32(want["logit"])
                    worst["logit"] = max(worst["logit"], float(lerr[valid].max()) if valid.any() else 0.0)
                    got_w = torch.where(valid, weight.cpu().double(), torch.zeros_like(want[mode]))
                    if mode == "softmax":
                        some = valid[..., 0]
                        werr = (got_w - want[mode])[valid].abs()
                        worst[mode] = max([worst[mode]] + ([float(werr.max())] if valid.any() else []))
                        assert bool(((got_w.sum(-1) - 1.0).abs()[some] <= topk * 2 * U).all()), what
                    else:
                        werr = ((got_w - want[mode]).abs() / _ulp32(want[mode]))[valid]
                        worst[mode] = max([worst[mode]] + ([float(werr.max())] if valid.any() else []))
    print(f"merge topk {topk}: {short_rows} short rows; max logit err {worst['logit']:.2f} ulps (bound 2), softmax weight err "
          f"{worst['softmax']:.3e} (bound {topk * 2 * U:.3e}), cosine weight err {worst['cosine']:.2f} ulps (bound 4)")
    assert short_rows > 0
    assert worst["logit"] <= 2 and worst["softmax"] <= topk * 2 * U and worst["cosine"] <= 4


@pytest.mark.parametrize("topk", [5, 16])
def test_merge_large_logits(dev, topk):
    """Unnormalised features (normalize=False) give dot products far above 1: scores of up to 13 are logits of up to 188, and exp(188)
    is not an f32.  The softmax must be taken relative to the row's maximum (mathematically the same, and the only thing that tells
    `exp(l_j - l_0)` from `exp(l_j)`).  Bound: the argument l_j - l_0 is off by at most two logit errors of 2 ulps and one subtraction,
    5 ulps of the largest logit; a softmax moves by at most half of its largest argument error; expf, the sum and the division as in
    test_merge_synthetic_lists:  |dw| <= 2.5 * ulp(max |logit|) + topk * 2^-23."""
    from fgvc_amd import ops
    T, HWq, HWk = 7, 257, PC.MERGE_HWK
    pi, ps = PC.merge_lists(T + 1, HWq, HWk, topk, seed=99 + topk)
    ps = ps * 24
    sp = PC.merge_slot_pairs(3, T, T + 1, seed=99)
    want = PC.merge_restated(pi, ps, sp, HWk, topk)
    idx, logit, weight = ops.merge_topk(pi.to(dev), ps.to(dev), sp.to(dev), HWk, topk, PC.TEMP, "softmax")
    assert torch.equal(idx.cpu().long(), want["idx"])
    valid = want["valid"]
    lmax = want["logit"][valid].abs().max()
    bound = 2.5 * float(_ulp32(lmax)) + topk * 2 * U
    err = (weight.cpu().double() - want["softmax"])[valid].abs()
    print(f"merge large logits topk {topk}: max |logit| {float(lmax):.1f}, weight err {float(err.max()):.3e} (bound {bound:.3e})")
    assert float(lmax) > 100 and bool((err <= bound).all()), float(err.max())


# ======================================================================================================================
# 3. propagate
# ======================================================================================================================
@pytest.mark.parametrize("P", PC.PROP_P)
def test_propagate_direct(dev, P):
    """fgvc_propagate_topk_f32 against the float64 gather-sum.  Bound: the kernel accumulates acc = fmaf(w_r, v_r, acc) over the topk
    entries: the product is exact inside the fma, every step rounds once, by at most 2^-24 of a partial sum that never exceeds
    S = sum_r |w_r v_r|; topk steps give topk * 2^-24 * S to first order, one more unit covers the second-order terms, and a sum that
    lands in the subnormals is off by less than the smallest normal f32:  |got - want| <= (topk + 1) * 2^-24 * S + 2^-126."""
    from fgvc_amd import ops
    worst = 0.0
    cases = [(g, g, L) for g in PC.PROP_GRIDS for L in (0, 3, 9)] + [((5, 33), (17, 23), 0)]       # the last: Hk x Wk != Hq x Wq
    for (Hq, Wq), (Hk, Wk), L in cases:
        for slots in PC.PROP_SLOTS:
            for topk in PC.PROP_TOPK:
                labels, idx, weight = PC.propagate_inputs(P, topk, Hq, Wq, Hk, Wk, slots, L, seed=len(slots))
                want, mag = PC.propagate_restated(labels, slots, idx, weight, Hq, Wq, Hk, Wk, L)
                got = ops.propagate_topk(labels.to(dev), torch.tensor(slots, dtype=torch.int32, device=dev), idx.to(dev),
                                         weight.to(dev), Hq, Wq, Hk, Wk, window_L=L).cpu().double()
                bound = (topk + 1) * U * mag + PC.F32_MIN_NORMAL
                ratio = float(((got - want).abs() / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, (P, (Hq, Wq), (Hk, Wk), L, slots, topk, ratio)
                assert bool((idx < 0).any()) or topk * Hq * Wq < 20
                if L > 0:       # live taps outside the image on all four borders (propagate_inputs plants the corner ones)
                    tap = idx.long().clamp_min(0) % (L * L)
                    q = torch.arange(Hq * Wq).view(-1, 1)
                    ky, kx = q // Wq + tap // L - L // 2, q % Wq + tap % L - L // 2
                    live = idx >= 0
                    assert all(bool((c & live).any()) for c in (ky < 0, ky >= Hk, kx < 0, kx >= Wk))
    print(f"propagate P {P}: max |err| / bound {worst:.3f}")


# ======================================================================================================================
# 4. Gaussian labels
# ======================================================================================================================
@pytest.mark.parametrize("case", PC.GAUSS, ids=PC.case_id)
def test_gaussian_labels(dev, case):
    """fgvc_gaussian_labels_f32 against exp(-arg), arg = d^2 / (2 sigma^2), in float64 from the f32 points.  Bound: the kernel's arg carries
    a relative error of about 4 * 2^-24 (the two differences, the squares and their sum, the division), which exp amplifies by |arg|;
    expf itself and the final rounding are within 4 * 2^-24 of the value; a result below the smallest normal f32 may be a subnormal or
    flushed:  |got - want| <= (4 + 4 |arg|) * 2^-24 * want + 2^-126."""
    from fgvc_amd import ops
    Hf, Wf, stride, P, sigma = case
    pts = PC.gauss_points(case)
    want, arg = PC.gauss_frame(pts, Hf, Wf, sigma, stride)
    got = ops.gaussian_labels(pts.to(dev), Hf, Wf, stride, sigma).cpu().double().t().reshape(P, Hf, Wf)
    bound = (4 + 4 * arg) * U * want + PC.F32_MIN_NORMAL
    ratio = float(((got - want).abs() / bound).max())
    print(f"gaussian labels {case}: max |err| / bound {ratio:.3f}, zeros {int((got == 0).sum())}, subnormal-sized wants "
          f"{int(((want > 0) & (want < PC.F32_MIN_NORMAL)).sum())}")
    assert ratio <= 1.0, ratio


def test_gaussian_bank_row_is_readout_frame(dev):
    """Row 0 of the engine's bank (fgvc_gaussian_labels_f32 at stride h // Hf) and the read-out's analytic frame 0 are the same label by
    two expressions: the bank row equals the restatement of the read-out's frame (tests/post_cases.py::gauss_frame at full resolution)
    sampled at the same pixels, within the bound of test_gaussian_labels."""
    from fgvc_amd import ops
    Hf, Wf, h, w, sigma = 30, 54, 120, 216, 6.0
    pts, _, _ = PC.readout_points(h, w)
    stride = h // Hf
    frame, arg = PC.gauss_frame(pts, h, w, sigma)
    want, arg = frame[:, ::stride, ::stride], arg[:, ::stride, ::stride]
    got = ops.gaussian_labels(pts.to(dev), Hf, Wf, stride, sigma).cpu().double().t().reshape(-1, Hf, Wf)
    ratio = float(((got - want).abs() / ((4 + 4 * arg) * U * want + PC.F32_MIN_NORMAL)).max())
    print(f"bank row 0 vs read-out frame 0: max |err| / bound {ratio:.3f}")
    assert ratio <= 1.0, ratio


# ======================================================================================================================
# 5. normalise
# ======================================================================================================================
@pytest.mark.parametrize("case", PC.NORMALIZE, ids=PC.case_id)
def test_normalize_to_hwc(dev, case):
    """fgvc_normalize_chw_to_hwc_f32 against x / max(||x||, 1e-12) in float64, channels last.  C = 512 and 371 take the large-LDS branch
    (more than 48 KiB of tile).  Bound: a thread sums the squares of C / 8 channels in order (C / 8 roundings), eight partial sums are
    folded (8 more), the square root halves that relative error and adds half an ulp, the division half an ulp:
    2 ulps + 2^-24 * (C / 8 + 8) relative.  A pixel of 1e-20-sized values has a norm below eps in any arithmetic (its squares underflow in
    f32, and it does not matter): both sides divide by eps, so the float64 statement holds there too and F.normalize in f32 is not needed
    as a stand-in.  Raw mode (normalize=False) is bit-equal; padding channels are exactly 0."""
    from fgvc_amd import ops
    n, C, H, W = case
    x = PC.normalize_input(case)
    xd = x.to(dev)
    got = ops.normalize_to_hwc(xd).cpu()
    want = PC.normalize_restated(x)
    bound = 2 * _ulp32(want) + U * (C / 8 + 8) * want.abs()
    ratio = float(((got.double() - want).abs() / bound.clamp_min(1e-300)).max())
    print(f"normalise {case}: max |err| / bound {ratio:.3f}")
    assert got.shape == (n, H * W, C) and ratio <= 1.0, ratio
    if H * W >= 3:
        assert bool((got[:, 0] == 0).all())                                                        # the zero vector stays zero
        assert torch.allclose(got[:, 2].double().norm(dim=-1), torch.ones(n, dtype=torch.float64), atol=1e-5)       # 1e-9-sized: above eps
    raw = ops.normalize_to_hwc(xd, normalize=False).cpu()
    assert torch.equal(raw, x.reshape(n, C, H * W).permute(0, 2, 1))
    if C <= 256:
        Co = ops.padded_channels(C)
        pad = ops.normalize_to_hwc(xd, pad=True).cpu()
        assert pad.shape == (n, H * W, Co) and torch.equal(pad[..., :C], got) and bool((pad[..., C:] == 0).all())
        assert torch.equal(ops.normalize_to_hwc(xd, normalize=False, pad=True).cpu()[..., :C], raw)


# ======================================================================================================================
# 6. BN (+ residual) (+ ReLU)
# ======================================================================================================================
def _bn(dev, shape, with_res, relu, seed=0):
    from fgvc_amd import ops
    x, res, mean, var, gamma, beta = PC.bn_inputs(shape, seed)
    bn = torch.nn.BatchNorm2d(shape[1]).eval()
    with torch.no_grad():
        bn.running_mean.copy_(mean), bn.running_var.copy_(var), bn.weight.copy_(gamma), bn.bias.copy_(beta)
    bn = bn.to(dev)
    res = res if with_res else None
    got = ops.bn_act(x.to(dev), bn, residual=None if res is None else res.to(dev), relu=relu, inplace=False).cpu().double()
    want, mag = PC.bn_restated(x, res, mean, var, gamma, beta, bn.eps, relu)
    return float(((got - want).abs() / (4 * _ulp32(mag))).max()), got, want


@pytest.mark.parametrize("shape", [(2, 8, 8, 12), (2, 8, 5, 7)], ids=["vector", "scalar"])
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
def test_bn_act_paths(dev, shape, with_res, relu):
    """fgvc_bn_act_f32: HW % 4 == 0 takes the float4 path, 5 x 7 the scalar one; residual None / given, ReLU on / off.  Bound: x - m, the
    three operations of 1 / sqrtf(var + eps), two products and up to two additions round once each, every one by at most half an ulp
    of a quantity no larger than A = |x - m| * inv * |g| + |b| + |res|: 4 ulps of A."""
    ratio, got, want = _bn(dev, shape, with_res, relu)
    print(f"bn_act {shape} residual {with_res} relu {relu}: max |err| / (4 ulps) {ratio:.3f}")
    assert ratio <= 1.0, ratio
    assert bool((got < 0).any()) != relu


def test_bn_act_grid_stride(dev):
    """(1, 3, 1400, 1000): 1 050 000 float4 items against the launch's 256 * 16 * 256 = 1 048 576 threads, so the grid-stride loop takes a second
    trip for the last 1 424 items (the end of channel 2), with a residual and ReLU."""
    shape = (1, 3, 1400, 1000)
    assert shape[1] * shape[2] * shape[3] // 4 > 256 * 16 * 256
    ratio, got, want = _bn(dev, shape, True, True, seed=3)
    tail = (got - want).abs().reshape(-1)[-4 * 1424:]
    print(f"bn_act grid-stride {shape}: max |err| / (4 ulps) {ratio:.3f}, second trip max err {float(tail.max()):.3e}")
    assert ratio <= 1.0, ratio
