"""GPU: the kernels of csrc/local.hip and csrc/dense_attend.hip against plain float64 evaluations of the same operations on the CPU.

Run on an MI355X with `pytest -m gpu`.  What each group pins (branches named so that a reader can see they ran):

* local window (local_merge_kernel<1|5|10|16>, local_merge_plan_kernel<1|5|10|16>, local_merge_slot's padding loop and its `done`
  early-out, topk_coord_kernel, topk_coord_rows_kernel), on the f32 and the f16x3 route;
* c2f fine stage (c2f_refine_kernel<1|5|10|16>): the one-lane-per-candidate FALLBACK (Cf = 12, 24, 48, 512), the ROW-COOPERATIVE path
  at both ends (Cf = 4: one lane per row, no shuffle; Cf = 256: one candidate per wave instruction), scale 1..4, T 1..3, Rf 0..10,
  P = 70 (second trip of the `pl += 64` loop), coarse cells forced to the corners and edges, both weight modes;
* dense attend (dense_attend_kernel<8|16|32> = PMAX, merge_state with empty splits, the online-softmax rescale, the masked band's
  jbeg / jend, dead lanes), dense_kth_kernel<16|64>, and propagate's RAW / SHIFT modes.

Index lists go through O.check_topk(structural=...): canonical order (score desc, candidate id asc) is demanded on every query whose
float64 ranks 1..k+1 are separated by more than 1e-5 OR tie exactly by construction (zero-padded taps; one key frame in two slots).
Every case asserts that at least 95 % of its queries are held to that (tests/test_window_reference_share.py shows the same shares
from the reference alone) and prints the share.  Bounds are derived, not fitted: see each helper.
"""
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import window_cases as WC

pytestmark = pytest.mark.gpu
TOL = 1e-3                # the project's bar on scores, weights and propagated values
TEMP, GAP = WC.TEMP, WC.GAP


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()          # the HIP library must be the thing under test: fail loudly if it is missing
    return torch.device("cuda:0")


def strict(dense, cls, idx, score, k, tol, what):
    """O.check_topk under the structural rule + the cap: at least 95 % of the queries are held to the exact list."""
    st = O.check_topk(dense, idx.cpu().long(), score.cpu(), k, tol=tol, gap=GAP, structural=cls)
    n = st["queries"]
    print(f"{what}: checkable {st['checkable']}/{n} = {st['checkable'] / n:.4f}, exact {st['exact']}/{n}, max score err {st['max_score_err']:.3e} (tol {tol:.3e})")
    assert st["checkable"] >= WC.MIN_SHARE * n, (what, st["checkable"], n)
    return st["checkable_mask"]


# ======================================================================================================================
# 2. local window
# ======================================================================================================================
def run_local(dev, q, keys, H, W, R, topk, route):
    from fgvc_amd import ops
    qf = ops.normalize_to_hwc(q[None].to(dev), pad=True)
    kf = ops.normalize_to_hwc(keys.to(dev), pad=True)
    if route == "f16x3":
        assert ops.split_path_ok(qf.shape[-1], H, W, topk, True, None, ops.MaskSpec(ry=R, rx=R), True)      # the 16-bit route is taken
    return ops.local_corr_topk(qf, kf, H, W, R, topk, TEMP, normalized=(route == "f16x3"))


def check_local(dev, shape, route, twin=False, zero_rows=False):
    from fgvc_amd import ops
    C, K, H, W, R, topk = shape
    q, keys, vals = WC.local_inputs(shape, twin=twin, zero_rows=zero_rows)
    idx, logit, weight = run_local(dev, q, keys, H, W, R, topk, route)
    dense, cls = WC.local_slab(q, keys, R, frames=[0] * K if twin else None)
    m = strict(dense, cls, idx, logit, topk, TOL, f"local {route} {shape}{' twin' if twin else ''}")
    # weights: float64 softmax over the float64 logits of the candidates the kernel listed (every query).  |dw| <= max|dlogit| / 2
    # for a softmax, so the bar on the logits carries over.
    want_w = dense.t().gather(1, idx.cpu().long()).softmax(1)
    werr = float((weight.cpu().double() - want_w).abs().max())
    print(f"  weight err {werr:.3e}")
    assert werr <= TOL, werr
    assert torch.allclose(weight.sum(1).cpu(), torch.ones(H * W), atol=1e-5)
    # propagated labels against the oracle's own out, on the queries whose list is pinned
    labels = vals.permute(0, 2, 3, 1).reshape(K, H * W, -1).contiguous().to(dev)
    out = ops.propagate_topk(labels, torch.arange(K, dtype=torch.int32, device=dev), idx, weight, H, W, H, W, window_L=2 * R + 1)
    o_out, o_idx, o_logit = O.local_corr_topk(q.double(), keys.double(), vals.double(), R, topk, TEMP)
    oerr = float((out.cpu().double() - o_out.flatten(1).t())[m].abs().max())
    print(f"  propagate err {oerr:.3e}")
    assert oerr <= TOL, oerr
    return idx, logit, weight, m


@pytest.mark.parametrize("shape", WC.LOCAL_F32, ids=WC.case_id)
def test_local_f32_route_sweep(dev, shape):
    """fgvc_local_corr_topk_f32.  topk 1 / 5, 6 / 10 / 16 = local_merge_kernel<1>, <5>, <10>, <16>; R = 0; 3x4 with R = 6: a window larger
    than the grid (the pair list ends in -1, padded zeros fill the list: local_merge_slot's padding loop); K = 1..7 slots."""
    idx, _, _, _ = check_local(dev, shape, "f32")
    C, K, H, W, R, topk = shape
    if (H, W, R) == (3, 4, 6):
        out = WC.window_outside(H, W, R)
        n_pad = out.t().gather(1, idx.cpu().long() % out.shape[0]).sum(1)
        assert int(n_pad.min()) >= topk - H * W              # only 12 in-image taps: at least 4 padded zeros in every list
    assert int(idx.min()) >= 0


@pytest.mark.parametrize("shape", WC.LOCAL_ZERO_ROWS, ids=WC.case_id)
def test_local_zero_key_rows(dev, shape):
    """Key rows that are all zero score exactly 0 inside the image, as the padded taps do outside it.  local_merge_slot meets the in-image
    zeros FIRST (they come with the pair list) and the padded zeros of LOWER candidate id afterwards: the only place in local.hip where
    the id clause of TopK::accepts decides (everywhere else equal scores arrive in ascending id order), followed by its `done`
    early-out.  topk 1 / 5 = local_merge_kernel<1>, <5>; the same lists through local_merge_plan_kernel."""
    from fgvc_amd import ops
    C, K, H, W, R, topk = shape
    idx, logit, weight, m = check_local(dev, shape, "f32", zero_rows=True)
    assert bool((idx.cpu().long() == torch.arange(topk)).all()) and bool((logit == 0).all())
    q, keys, _ = WC.local_inputs(shape, zero_rows=True)
    feats = ops.normalize_to_hwc(torch.cat([q[None], keys], 0).to(dev), pad=True)
    pairs = ops.make_pairs([(0, 1 + t) for t in range(K)], dev)
    pidx, pscore = ops.pair_topk(feats, feats, pairs, H, W, H, W, ops.MaskSpec(ry=R, rx=R), topk)
    assert int(((pscore[0] == 0) & (pidx[0] >= 0)).all(1).sum()) >= 0.9 * H * W       # slot 0's pair list is full of in-image zeros
    slot_pair = torch.arange(K, dtype=torch.int32, device=dev).view(1, K)
    pi, pl, pw = ops.local_merge_plan(pidx, pscore, slot_pair, H, W, R, topk, TEMP)
    assert torch.equal(pi[0], idx) and torch.equal(pl[0], logit) and torch.equal(pw[0], weight)


@pytest.mark.parametrize("shape", WC.LOCAL_F16X3, ids=WC.case_id)
def test_local_f16x3_route(dev, shape):
    """fgvc_local_corr_topk_f16x3 (C = 256, normalised rows, topk <= 10) at the project's bars: gap 1e-5, scores 1e-3."""
    check_local(dev, shape, "f16x3")
    from fgvc_amd import ops
    assert not ops.pair_f16x3_timed_out()


@pytest.mark.parametrize("case", [(WC.LOCAL_TIES[0], "f32"), (WC.LOCAL_TIES[1], "f32"), (WC.LOCAL_TIES[1], "f16x3")],
                         ids=lambda c: WC.case_id(c[0]) + "-" + c[1])
def test_local_exact_ties_across_slots(dev, case):
    """One key frame in both slots: every score appears twice, bit for bit.  The merged list interleaves slot 0 before slot 1 for each
    tap (and lists the padded zeros of slot 0 before those of slot 1): TopK::accepts / insert's id tie-break."""
    shape, route = case
    C, K, H, W, R, topk = shape
    idx, logit, _, m = check_local(dev, shape, route, twin=True)
    LL = (2 * R + 1) ** 2
    i, l = idx.cpu().long(), logit.cpu()
    inside = (~WC.window_outside(H, W, R).t().gather(1, i % LL)).long().cumprod(1).bool()       # (S,k) entries before the first padded zero
    first = inside[:, 0::2] & inside[:, 1::2]                                                    # a pair of in-image entries
    a, b = i[:, 0::2], i[:, 1::2]
    pinned = m.view(-1, 1) & first
    assert bool(((a < LL) & (b == a + LL))[pinned].all())                                        # slot 0 then slot 1 of the same tap
    assert bool((l[:, 0::2] == l[:, 1::2])[pinned].all())                                        # bitwise equal scores
    assert int(pinned.sum()) > H * W


@pytest.mark.parametrize("topk", WC.PLAN_TOPK)
def test_local_merge_plan_rows(dev, topk):
    """fgvc_local_merge_plan_f32, topk 1 / 5 / 10 / 16 = local_merge_plan_kernel<1>, <5>, <10>, <16>: a -1 slot, a pair id >= n_pairs (no
    slot), a pair in two slot positions (exact ties across slots) and a single-slot row, each against its float64 restatement."""
    from fgvc_amd import ops
    C, K, H, W, R = WC.PLAN_SHAPE
    q, keys, _ = WC.local_inputs((C, K, H, W, R, topk))
    feats = ops.normalize_to_hwc(torch.cat([q[None], keys], 0).to(dev), pad=True)
    pairs = ops.make_pairs([(0, 1 + t) for t in range(K)], dev)
    pidx, pscore = ops.pair_topk(feats, feats, pairs, H, W, H, W, ops.MaskSpec(ry=R, rx=R), topk)
    slot_pair = torch.tensor(WC.PLAN_ROWS, dtype=torch.int32, device=dev)
    idx, logit, weight = ops.local_merge_plan(pidx, pscore, slot_pair, H, W, R, topk, TEMP)
    for r, row in enumerate(WC.PLAN_ROWS):
        dense, cls = WC.local_slab(q, keys, R, frames=WC.plan_frames(row, K))
        strict(dense, cls, idx[r], logit[r], topk, TOL, f"plan row {row} topk {topk}")
        want_w = dense.t().gather(1, idx[r].cpu().long()).softmax(1)
        assert float((weight[r].cpu().double() - want_w).abs().max()) <= TOL
        LL = (2 * R + 1) ** 2
        live = [j for j, p in enumerate(row) if 0 <= p < K]
        assert set((idx[r].cpu().long() // LL).unique().tolist()) <= set(live)                   # no candidate of an empty slot


def coord_bound(k, scale, H, W, werr):
    """f32 rounding of a k-term weighted sum of coordinates <= scale * max(H, W): k * 2^-23 * scale * max(H, W); a weight error `werr`
    per term moves the sum by at most k * werr * scale * max(H, W)."""
    return k * (2.0 ** -23 + werr) * scale * max(H, W)


@pytest.mark.parametrize("case", WC.COORD, ids=WC.case_id)
def test_topk_coord_vs_get_coord(dev, case):
    """topk_coord_kernel and topk_coord_rows_kernel on border-heavy windows: (a) for the lists the kernels are GIVEN (with -1 entries
    and padded taps, which contribute (0, 0)) against the float64 sum over those very lists -- f32 rounding only; (b) end to end
    against O.get_coord in float64 on the queries whose list is pinned, with the weight error the local test allows (1e-3)."""
    from fgvc_amd import ops
    C, H, W, R, topk, scale = case
    shape = (C, 1, H, W, R, topk)
    q, keys, _ = WC.local_inputs(shape)
    idx, logit, weight = run_local(dev, q, keys, H, W, R, topk, "f32")
    dense, cls = WC.local_slab(q, keys, R)
    keff = min(topk, dense.shape[0])
    m = strict(dense, cls, idx[:, :keff], logit[:, :keff], keff, TOL, f"coord {case}")
    if keff < topk:
        assert bool((idx[:, keff:] == -1).all()) and bool((weight[:, keff:] == 0).all())
    rows_i, rows_w = [idx], [weight]
    g = torch.Generator().manual_seed(5)
    for drop in (0.3, 0.7):                       # the same lists with entries struck out (-1) and other weights (summing to 1 over the whole list)
        kill = (torch.rand(idx.shape, generator=g) < drop).to(dev)
        rows_i.append(torch.where(kill, torch.full_like(idx, -1), idx))
        w = torch.rand(weight.shape, generator=g)
        rows_w.append((w / w.sum(1, keepdim=True)).to(dev))
    ri, rw = torch.stack(rows_i, 0).contiguous(), torch.stack(rows_w, 0).contiguous()
    fields = ops.topk_coord_rows(ri, rw, H, W, R, scale).cpu().double()
    tight = coord_bound(topk, scale, H, W, 0.0)
    for r in range(ri.shape[0]):
        want = WC.coord_of_lists(ri[r].cpu().long(), rw[r].cpu(), H, W, R, scale)
        one = ops.topk_coord(ri[r].contiguous(), rw[r].contiguous(), H, W, R, scale).cpu().double()
        e1, e2 = float((one - want).abs().max()), float((fields[r] - want).abs().max())
        print(f"  row {r}: topk_coord err {e1:.3e}, topk_coord_rows err {e2:.3e} (bound {tight:.3e})")
        assert e1 <= tight and e2 <= tight
    ref = O.get_coord(q.double(), keys[0].double(), R, topk, TEMP, scale).reshape(2, H * W).t()
    err = float((fields[0] - ref)[m].abs().max())
    loose = coord_bound(topk, scale, H, W, TOL)
    print(f"  vs get_coord: err {err:.3e} (bound {loose:.3e})")
    assert err <= loose


# ======================================================================================================================
# 3. coarse-to-fine fine stage
# ======================================================================================================================
def c2f_score_tol(Cf):
    """worst-case f32 FMA chain over Cf products of unit-norm rows (+ the shuffle adds and the division): (Cf + 4) * 2^-24 / temperature"""
    return (Cf + 4) * 2.0 ** -24 / TEMP


def check_c2f(dev, shape, P=3, forced=False, twin=False, what=""):
    from fgvc_amd import ops
    Cf, T, H, W, scale, Rf, topk = shape
    c = WC.c2f_case(shape, P=P, forced=forced, twin=twin)
    assert c2f_score_tol(Cf) < TOL
    qf = c["qfine"].reshape(Cf, -1).t().contiguous().to(dev)                                     # (sHsW, Cf) unit-norm rows, as given
    kf = c["kfine"].reshape(Cf, T, -1).permute(1, 2, 0).contiguous().to(dev)                     # (T, sHsW, Cf)
    vf = c["v"].reshape(P, T, -1).permute(1, 2, 0).contiguous().to(dev)                          # (T, sHsW, P)
    arg = c["arg"].to(dev, torch.int32).contiguous()
    res = {}
    for mode in ("softmax", "cosine"):
        out, idx, logit = ops.c2f_refine(arg, qf, kf, vf, H, W, scale, Rf, topk, TEMP, mode=mode)
        m = strict(c["dense"], c["cls"], idx, logit, topk, c2f_score_tol(Cf), f"c2f {what}{shape} {mode}")
        want, _, _ = WC.c2f_out(c["dense"], c["pix"], c["v"], topk, mode)
        bound = TOL if mode == "softmax" else 1e-5 * max(1.0, float(want.abs().max()))
        err = float((out.cpu().double() - want.t())[m].abs().max())
        print(f"  out err {err:.3e} (bound {bound:.3e})")
        assert err <= bound, (mode, err, bound)
        res[mode] = (out, idx, logit, m)
    assert torch.equal(res["softmax"][1], res["cosine"][1]) and torch.equal(res["softmax"][2], res["cosine"][2])   # one selection, two weightings
    return c, res


@pytest.mark.parametrize("shape", WC.C2F_SWEEP, ids=WC.case_id)
def test_c2f_refine_sweep(dev, shape):
    """c2f_refine_kernel<1|5|10|16> (topk 1 / 5 / 9, 10 / 16).  Cf = 12, 24, 48, 512: the FALLBACK (one lane per candidate); Cf = 4: the
    ROW-COOPERATIVE path with one lane per row (no shuffle); Cf = 256: one candidate per wave instruction; Cf = 8, 16 in between.
    scale 2 / 3 / 4, T 1 / 2 / 3, Rf 0 / 1 / 2 / 3 / 6.  Both weight modes; padded taps are structural candidates."""
    check_c2f(dev, shape)


@pytest.mark.parametrize("name", list(WC.C2F_EXTRA))
def test_c2f_refine_extra(dev, name):
    """scale = 1; P = 70 (the second trip of the `pl += 64` loop); coarse cells forced to the four corners and the edge cells for every
    query, so that most of the fine window lies outside the map (row-cooperative and fallback path)."""
    shape, P, forced = WC.C2F_EXTRA[name]
    check_c2f(dev, shape, P=P, forced=forced, what=name + " ")


@pytest.mark.parametrize("name", list(WC.C2F_TIES))
def test_c2f_refine_exact_ties(dev, name):
    """One key frame in both slots with equal coarse cells: the scores are bitwise equal across lanes and lane groups; the butterfly
    arg-max and TopK::accepts must put the lower candidate id first.  Row-cooperative (Cf = 16, 256) and fallback (Cf = 12)."""
    shape = WC.C2F_TIES[name]
    Cf, T, H, W, scale, Rf, topk = shape
    c, res = check_c2f(dev, shape, twin=True, what=name + " ")
    out, idx, logit, m = res["softmax"]
    LL = (2 * Rf + 1) ** 2
    i, l = idx.cpu().long(), logit.cpu()
    inside = (c["cls"].t().gather(1, i) != 1).long().cumprod(1).bool()                          # entries before the first padded zero
    pairs = inside[:, 0:-1:2] & inside[:, 1::2] & m.view(-1, 1)
    a, b = i[:, 0:-1:2], i[:, 1::2]
    assert bool(((a < LL) & (b == a + LL))[pairs].all())
    assert bool((l[:, 0:-1:2] == l[:, 1::2])[pairs].all())
    assert int(pairs.sum()) > H * W


# ======================================================================================================================
# 4. dense attend, k-th largest, propagate
# ======================================================================================================================
MODES = {"softmax": 0, "cosine": 1, "raw": 2}


def attend_ref(vols, labels, keep, mode):
    """The topk=None branch (local_attention.py:376-383) from GIVEN affinity slabs, in the dtype of `vols`: vols (T,HWk,HWq), labels
    (T,HWk,P), keep (T,HWk,HWq) bool or None -> (HWq,P)."""
    T, HWk, HWq = vols.shape
    a = vols.reshape(T * HWk, HWq)
    if keep is not None:
        a = a.masked_fill(~keep.reshape(T * HWk, HWq), O.NEG_INF)
    if mode == "softmax":
        w = a.softmax(0)
    elif mode == "cosine":
        w = a.clamp(min=0) ** 2
    else:
        w = torch.where(torch.isinf(a), torch.zeros_like(a), a)
    return (labels.reshape(T * HWk, -1).t() @ w).t()


def sum_bound(want64, got32_formula, logit_range, fast_exp):
    """The bound on a weighted sum over at most T * HWk terms.  Ceiling: the project's 1e-3, absolute.  Asserted: 16 x the error of the
    SAME formula in plain float32 torch on the CPU (room for another summation order), + logit_range * 2^-22 relative for the fast
    exponential (v_exp_f32 after an f32 multiply by log2 e: the argument's rounding scales with its magnitude; softmax outputs are
    <= 1, so relative is absolute there), floor 2e-6."""
    fin = torch.isfinite(want64)
    e32 = float((got32_formula.double() - want64)[fin].abs().max())
    b = 16.0 * e32 + (logit_range * 2.0 ** -22 if fast_exp else 0.0)
    return min(TOL, max(2e-6, b)), e32


def make_slabs(T, HWk, HWq, temperature, seed, C=32):
    """f32 affinity slabs cos / temperature of random unit rows: (T, HWk, HWq).  These f32 numbers are the kernels' INPUT."""
    g = torch.Generator().manual_seed(seed)
    qn = O.l2_normalize(torch.randn(HWq, C, generator=g), 1)
    kn = O.l2_normalize(torch.randn(T, HWk, C, generator=g), 2)
    return (torch.einsum("tjc,ic->tji", kn, qn) / temperature).contiguous()


def make_labels(T, HWk, P, seed, planted=None):
    """random labels in [0, 1]; the first channels are INDICATORS (1 at one key row, 0 elsewhere: the output is that key's weight):
    the first key row, the last key row of the last slot, the planted row, a middle row."""
    g = torch.Generator().manual_seed(seed)
    lab = torch.rand(T, HWk, P, generator=g)
    rows = [(0, 0), (T - 1, HWk - 1), planted if planted is not None else (T // 2, HWk // 3), (T // 2, HWk // 2)]
    for p, (t, j) in enumerate(rows[:max(1, P // 2)]):
        lab[:, :, p] = 0.0
        lab[t, j, p] = 1.0
    return lab


def keep_mask(H, W, T, r2max, ry, rx, non_mask_len):
    """keep[t, key, query] of the kernel's predicate dy^2 + dx^2 <= r2max, |dy| <= ry, |dx| <= rx; slots below non_mask_len unmasked"""
    ys, xs = torch.arange(H * W) // W, torch.arange(H * W) % W
    dy, dx = ys.view(-1, 1) - ys.view(1, -1), xs.view(-1, 1) - xs.view(1, -1)
    k = (dy * dy + dx * dx <= r2max) & (dy.abs() <= ry) & (dx.abs() <= rx)
    k = k.unsqueeze(0).expand(T, -1, -1).clone()
    k[:non_mask_len] = True
    return k


def attend_direct(dev, vols, labels, Hq, Wq, Hk, Wk, mode, nsplit, mask=None, non_mask_len=0):
    """fgvc_dense_attend_f32 per key slot + fgvc_dense_attend_finish_f32 with the test's own nsplit; the state starts as NaN, so a state
    row that a split failed to write cannot pass."""
    from fgvc_amd import _lib, ops
    T, HWk, HWq = vols.shape
    P = labels.shape[2]
    NO = _lib.NO_LIMIT
    r2max, ry, rx = mask if mask is not None else (NO, NO, NO)
    vd, ld = vols.to(dev), labels.contiguous().to(dev)
    state = torch.full((nsplit, HWq, P + 2), float("nan"), device=dev)
    for t in range(T):
        masked = int(mask is not None and t >= non_mask_len)
        _lib.call("fgvc_dense_attend_f32", ops._ptr(vd[t]), ops._ptr(ld[t]), Hq, Wq, Hk, Wk, P, masked, min(r2max, NO), min(ry, NO), min(rx, NO),
                  MODES[mode], int(t == 0), ops._ptr(state), nsplit, ops._stream(vd))
    out = torch.full((HWq, P), float("nan"), device=dev)
    _lib.call("fgvc_dense_attend_finish_f32", ops._ptr(state), nsplit, HWq, P, MODES[mode], ops._ptr(out), ops._stream(vd))
    return out.cpu()


def check_attend(dev, vols, labels, Hq, Wq, Hk, Wk, mode, nsplit, what, mask=None, non_mask_len=0):
    T = vols.shape[0]
    keep = keep_mask(Hk, Wk, T, *mask, non_mask_len) if mask is not None else None
    want = attend_ref(vols.double(), labels.double(), keep, mode)
    f32 = attend_ref(vols, labels, keep, mode)
    rng = float(vols.max() - vols.min())
    bound, e32 = sum_bound(want, f32, rng, mode == "softmax")
    got = attend_direct(dev, vols, labels, Hq, Wq, Hk, Wk, mode, nsplit, mask, non_mask_len)
    err = float((got.double() - want).abs().max())
    print(f"dense_attend {what} {mode} nsplit {nsplit}: err {err:.3e}, bound {bound:.3e} (f32 torch formula {e32:.3e}, |want|max {float(want.abs().max()):.3e})")
    assert err <= bound, (err, bound)
    return got, want


# (P, nsplit, mode, (Hq, Wq), (Hk, Wk), T, temperature): P = 1, 8 -> dense_attend_kernel<8>, 9, 16 -> <16>, 17, 32 -> <32>; HWq = 5, 64, 65,
# 851 (dead lanes below and beside a full band); nsplit 16 / 64 > HWk / 4: some splits see no key row and hand (-inf, 0, 0...) to the merge
ATTEND = [(1, 1, "softmax", (1, 5), (6, 7), 1, 0.07), (8, 3, "softmax", (8, 8), (6, 7), 3, 0.01), (9, 64, "cosine", (5, 13), (6, 7), 3, 0.07),
          (16, 16, "raw", (5, 13), (6, 7), 1, 0.07), (17, 3, "softmax", (23, 37), (6, 7), 3, 0.07), (32, 64, "softmax", (5, 13), (9, 5), 3, 0.01),
          (32, 1, "cosine", (8, 8), (6, 7), 3, 1.0), (17, 16, "raw", (1, 5), (6, 7), 3, 0.07), (8, 16, "softmax", (5, 13), (6, 7), 3, 0.07),
          (16, 64, "softmax", (8, 8), (6, 7), 1, 0.07), (9, 3, "softmax", (5, 13), (6, 7), 3, 0.01)]


@pytest.mark.parametrize("case", ATTEND, ids=lambda c: f"P{c[0]}-ns{c[1]}-{c[2]}-q{c[3][0]}x{c[3][1]}-T{c[5]}-t{c[6]}")
def test_dense_attend_forced_splits(dev, case):
    """fgvc_dense_attend_f32 / _finish_f32 called directly so that the test chooses nsplit.  Query grid != key grid (unmasked).  In the
    softmax cases the column maximum of every query is PLANTED in the last key slot, in a key row of the highest split: the
    running-max rescale (`a > m`), merge_state across waves, splits and key slots (first = 0) all carry weight."""
    P, nsplit, mode, (Hq, Wq), (Hk, Wk), T, temp = case
    HWq, HWk = Hq * Wq, Hk * Wk
    vols = make_slabs(T, HWk, HWq, temp, seed=P + nsplit)
    planted = None
    if mode == "softmax":
        js = [j for j in range(HWk) if (j // 4) % nsplit == min(nsplit, (HWk + 3) // 4) - 1]
        planted = (T - 1, js[-1])
        vols[T - 1, js[-1], :] = vols.amax((0, 1)) + 1.5           # the maximum by 1.5: its neighbours keep e^-1.5 of weight and more
    labels = make_labels(T, HWk, P, seed=P, planted=planted)
    got, want = check_attend(dev, vols, labels, Hq, Wq, Hk, Wk, mode, nsplit, f"P{P} q{Hq}x{Wq} k{Hk}x{Wk} T{T} t{temp}")
    if mode == "softmax" and P >= 6:
        assert float(want[:, 2].min()) > 0.05                      # the planted key's indicator channel: it holds real weight everywhere


# (mask (r2max, ry, rx), non_mask_len, mode, P, nsplit, (H, W), T, temperature)
NO = 0x3FFFFFFF
MASKED = [((10, NO, NO), 0, "softmax", 8, 3, (23, 37), 3, 0.07), ((NO, 2, 5), 1, "cosine", 9, 1, (23, 37), 3, 0.07),
          ((13, 3, 2), 0, "raw", 17, 64, (23, 37), 2, 0.07), ((2, NO, NO), 1, "softmax", 8, 7, (23, 37), 3, 0.01),
          ((NO, 1, 2), 0, "softmax", 4, 3, (5, 13), 2, 0.07), ((5, NO, NO), 0, "raw", 8, 2, (5, 13), 1, 0.07),
          ((NO, 0, 0), 0, "cosine", 8, 5, (9, 11), 1, 1.0)]


@pytest.mark.parametrize("case", MASKED, ids=lambda c: f"r{c[0][0] if c[0][0] < NO else 'x'}-{c[0][1] if c[0][1] < NO else 'x'}-{c[0][2] if c[0][2] < NO else 'x'}-nml{c[1]}-{c[2]}-P{c[3]}-ns{c[4]}-{c[5][0]}x{c[5][1]}")
def test_dense_attend_masked_band(dev, case):
    """Disc and box masks whose reach cuts the first and the last 64-query band (jbeg clamps at 0, jend at HWk; 851 = 13 bands + 19 live
    lanes), non_mask_len = 1 (slot 0 unmasked).  'raw' and 'cosine' weight every reachable key alike, so one key row dropped at
    either end of the band moves the sum far beyond the bound."""
    mask, nml, mode, P, nsplit, (H, W), T, temp = case
    vols = make_slabs(T, H * W, H * W, temp, seed=P + nsplit + H)
    labels = make_labels(T, H * W, P, seed=P + 1)
    check_attend(dev, vols, labels, H, W, H, W, mode, nsplit, f"mask {mask} nml {nml} {H}x{W} T{T}", mask, nml)


@pytest.mark.parametrize("mode", ["softmax", "cosine", "raw"])
def test_dense_attend_api_all_masked_column(dev, mode):
    """ops.dense_attend (nsplit from fgvc_dense_attend_splits) with a dense mask that masks one query column entirely and a query grid
    unlike the key grid: the softmax of that column is NaN on both sides (0 / 0, as the reference), 0 in the other modes; every other
    column is checked as usual, from the slabs fgvc_corr_volume_f32 produced (read back: they are the attend kernel's input)."""
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(77)
    C, (Hq, Wq), (Hk, Wk), T, P = 32, (5, 13), (6, 7), 3, 5
    HWq, HWk = Hq * Wq, Hk * Wk
    q, key = torch.randn(1, C, Hq, Wq, generator=g), torch.randn(T, C, Hk, Wk, generator=g)
    labels = make_labels(T, HWk, P, seed=3)
    dm = torch.rand(HWk, HWq, generator=g) < 0.6
    dead = 37
    dm[:, dead] = False
    qf = ops.normalize_to_hwc(q.to(dev))[0]
    kf = ops.normalize_to_hwc(key.to(dev))
    got = ops.dense_attend(qf, kf, labels.to(dev), Hq, Wq, Hk, Wk, ops.MaskSpec.none(), TEMP, mode, 0, dm.to(dev)).cpu()
    vols = torch.stack([ops.corr_volume(qf, kf[t], TEMP, "f32").cpu() for t in range(T)], 0)
    keep = dm.unsqueeze(0).expand(T, -1, -1)
    want = attend_ref(vols.double(), labels.double(), keep, mode)
    bound, e32 = sum_bound(want, attend_ref(vols, labels, keep, mode), float(vols.max() - vols.min()), mode == "softmax")
    live = torch.arange(HWq) != dead
    if mode == "softmax":
        assert bool(torch.isnan(want[dead]).all()) and bool(torch.isnan(got[dead]).all())
    else:
        assert bool((want[dead] == 0).all()) and bool((got[dead] == 0).all())
    err = float((got.double() - want)[live].abs().max())
    print(f"dense_attend api {mode}: err {err:.3e}, bound {bound:.3e} (f32 torch formula {e32:.3e})")
    assert err <= bound
    if mode != "raw":   # and against the oracle from the features (its own f64 volume): the project's bar (the oracle has no 'raw' mode)
        o = O.masked_attention_efficient(q.double(), key.transpose(0, 1)[None].double(), labels.permute(2, 0, 1).reshape(1, P, T, Hk, Wk).double(),
                                         mask=dm, temperature=TEMP, topk=None, mode=mode)[0].reshape(P, HWq).t()
        bar = TOL if mode == "softmax" else 1e-5 * max(1.0, float(o[live].abs().max()))      # cosine: the API golden's bar
        eo = float((got.double() - o)[live].abs().max())
        print(f"  vs the oracle from the features: err {eo:.3e} (bar {bar:.3e})")
        assert eo <= bar


# (HWk, HWq, k, nsplit): k 1, 5, 16 -> dense_kth_kernel<16>; 17, 64 -> dense_kth_kernel<64>; k == HWk; nsplit > HWk / 4
KTH = [(90, 65, 1, 1), (90, 65, 5, 3), (90, 65, 16, 64), (90, 65, 17, 3), (90, 5, 64, 30), (90, 64, 64, 1), (17, 65, 17, 3), (64, 5, 64, 64),
       (5, 65, 5, 3), (16, 851, 16, 2), (90, 851, 17, 64)]


@pytest.mark.parametrize("case", KTH, ids=lambda c: f"HWk{c[0]}-HWq{c[1]}-k{c[2]}-ns{c[3]}")
def test_dense_kth_bitwise(dev, case):
    """fgvc_dense_kth_f32 on a slab quantised to steps of 0.5 (runs of duplicated values straddle the k-th rank of every column): thr is
    one of the f32 inputs, so it equals torch.topk's k-th value in float64 bit for bit."""
    from fgvc_amd import _lib, ops
    HWk, HWq, k, nsplit = case
    g = torch.Generator().manual_seed(HWk + k)
    vol = (torch.randn(HWk, HWq, generator=g) * 2).round() / 2
    K = 16 if k <= 16 else 64
    vd = vol.to(dev)
    part = torch.full((nsplit, HWq, K), float("nan"), device=dev)
    thr = torch.full((HWq,), float("nan"), device=dev)
    _lib.call("fgvc_dense_kth_f32", ops._ptr(vd), HWk, HWq, k, ops._ptr(part), nsplit, ops._ptr(thr), ops._stream(vd))
    want = vol.double().topk(k, dim=0).values[k - 1]
    dup = (vol.double() == want.view(1, -1)).sum(0)
    if HWk >= 64 and k >= 5:
        assert float((dup > 1).float().mean()) > 0.5                      # the k-th value is a duplicated one in most columns
    assert torch.equal(thr.cpu().double(), want), int((thr.cpu().double() != want).sum())


@pytest.mark.parametrize("topk", [None, 1, 5, 17, 64])
def test_dense_propagate_vs_oracle(dev, topk):
    """ops.dense_propagate (P = 40: two chunks of <= 32 label channels; HWq = 65: a band with one live lane) against O.propagate in
    float64: mode RAW (topk None: the entry is the weight) and mode SHIFT (max(a - k-th largest, 0) / their sum)."""
    from fgvc_amd import ops
    g = torch.Generator().manual_seed(11)
    H, W, P = 5, 13, 40
    aff = (torch.rand(1, H * W, H * W, generator=g) * 8).round() / 8 if topk else torch.randn(1, H * W, H * W, generator=g)
    img = torch.rand(1, P, H, W, generator=g)
    got = ops.dense_propagate(aff[0].contiguous().to(dev), img[0].reshape(P, -1).t().contiguous().to(dev), topk).cpu()
    want = O.propagate(img.double(), aff.double(), topk)[0].reshape(P, -1).t()
    f32 = O.propagate(img, aff, topk)[0].reshape(P, -1).t()
    bound, e32 = sum_bound(want, f32, 0.0, False)
    err = float((got.double() - want).abs().max())
    print(f"dense_propagate topk {topk}: err {err:.3e}, bound {bound:.3e} (f32 torch formula {e32:.3e})")
    assert err <= bound
