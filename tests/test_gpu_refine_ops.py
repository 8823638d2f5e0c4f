"""GPU: fgvc_merge_refine_topk_f32 (csrc/refine.hip) ALONE, on pair lists built on the host (tests/refine_cases.py), against the plain
restatement of the rule in the header of refine.hip.  tests/test_gpu_refine.py runs the merge behind the real f16 + FP6 pair kernel,
whose error is a third of `eps`; here the approximate scores sit AT the bound (|a - s32| <= eps - 2^-23, pushed across the k-th place
and across every slot's own last entry), so an implementation that needed eps / 2 to be right fails.

Run on an MI355X with `pytest -m gpu`.  The entry point is called through ctypes with the three outputs as views 4096 elements inside
larger buffers, prefilled with a sentinel (idx: -7) or a NaN pattern (logit, weight): every entry is written, nothing outside is.

What every case asserts (check()):
* idx equals the restatement's list EXACTLY on every held query (refine_cases: no f64 dot product of its first k + 1 within 1e-12 of an
  f32 rounding midpoint -- the only way the kernel's own sum order can change an s32), at least 95 % of the case;
* logit: the score the restatement says the entry carries (s32 where re-scored or from scratch, the approximate a otherwise) divided by
  tau, within 2 ulps -- one f32 division (half an ulp) plus the 0.89 * 2^-24 relative distance of f32(0.07) from 0.07, the bound of
  tests/test_gpu_post_ops.py::test_merge_synthetic_lists; on held queries (elsewhere the lists themselves may differ);
* weights: rf_write is expression for expression merge_topk_kernel, so that module's bounds: topk * 2^-23 absolute for softmax (derived for
  logits below 8 in size; 2.5 ulps of the largest logit more where a case exceeds that, as test_merge_large_logits derives), 4 ulps for
  cosine; a tail behind a short list is idx -1, logit -inf, weight 0;
* statistics words 0 (minus word 7), 1, 2, 3, 6, 7 equal the restatement's counts -- the path of every query is decided by the input
  scores alone, in f32 expressions the restatement repeats bit for bit;
* word 4 <= eps and within 2^-24 (one f32 unit of a score below 1: the kernel's sum order) of the largest |a - s32| over the entries the
  restatement re-scores; word 5 the same over the unbiased sample, never above the largest |a - s32| over all listed entries;
* ops.pair_f16x3_timed_out() stays false.
Each test prints its measured maxima next to the bounds.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import refine_cases as RC

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SENTINEL = -7
NAN_BITS = 0x7FC0BEEF


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


def _banks(b, dev, bank):
    """(q tensor, byte offset, frame bytes, row bytes, k tensor, ...) in one of the forms the entry point takes"""
    one = b.q_rows is b.k_rows
    if bank == "f32":                    # 1024-byte rows; one tensor for both sides where the grids are equal
        k = torch.from_numpy(b.k_rows).to(dev)
        q = k if one else torch.from_numpy(b.q_rows).to(dev)
        return q, 0, q.shape[1] * 1024, 1024, k, 0, k.shape[1] * 1024, 1024
    if bank == "separate":               # two tensors, each NaN where only the other may be read
        assert one
        n_key = 1 + int(b.pairs[:, 1].max())
        qn, kn = b.q_rows.copy(), b.k_rows.copy()
        qn[:n_key], kn[n_key:] = np.nan, np.nan
        q, k = torch.from_numpy(qn).to(dev), torch.from_numpy(kn).to(dev)
        return q, 0, q.shape[1] * 1024, 1024, k, 0, k.shape[1] * 1024, 1024
    if bank == "f16f6x":                 # 2 KiB rows, the f32 channels in the second KiB (ops.split_f16f6x); the first KiB is not the merge's to read
        assert one
        raw = np.full(b.k_rows.shape[:2] + (2048,), 0xFF, np.uint8)
        raw[:, :, 1024:] = b.k_rows.view(np.uint8).reshape(b.k_rows.shape[:2] + (1024,))
        k = torch.from_numpy(raw).to(dev)
        return k, 1024, k.shape[1] * 2048, 2048, k, 1024, k.shape[1] * 2048, 2048
    raise ValueError(bank)


def launch(b, dev, bank="f32", mode="softmax", ws=None):
    """fgvc_merge_refine_topk_f32 through ctypes into guarded views; returns the views' contents on the CPU and the eight statistics words"""
    from fgvc_amd import _lib, ops
    case = b.case
    Hq, Wq = case.grid
    Hk, Wk = case.kgrid or case.grid
    n_out, T = b.slot_pair.shape
    n = n_out * Hq * Wq * case.k
    idx_buf = torch.full((n + 2 * RC.GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    lg_buf = torch.full((n + 2 * RC.GUARD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    w_buf = torch.full((n + 2 * RC.GUARD,), NAN_BITS, dtype=torch.int32, device=dev).view(torch.float32)
    views = [x[RC.GUARD:RC.GUARD + n] for x in (idx_buf, lg_buf, w_buf)]
    if ws is None:
        ws = ops.merge_refine_workspace(n_out, Hq * Wq, dev)
        ws.fill_(0x5A5A5A5A)                                                      # nothing but what the launch itself zeroes may be relied on
    assert ws.numel() * 4 >= _lib.load().fgvc_merge_refine_workspace_bytes(n_out, Hq * Wq)
    pi, ps = torch.from_numpy(b.pair_idx).to(dev), torch.from_numpy(b.pair_score).to(dev)
    sp, pr = torch.from_numpy(b.slot_pair).to(dev), torch.from_numpy(b.pairs).to(dev)
    q, qo, qfb, qrb, k, ko, kfb, krb = _banks(b, dev, bank)
    wm = {"softmax": _lib.WEIGHT_SOFTMAX, "cosine": _lib.WEIGHT_COSINE}[mode]
    r2max, ry, rx = case.mask
    _lib.call("fgvc_merge_refine_topk_f32", ops._ptr(pi), ops._ptr(ps), ops._ptr(sp), ops._ptr(pr),
              C.c_void_p(q.data_ptr() + qo), C.c_int64(qfb), qrb, C.c_void_p(k.data_ptr() + ko), C.c_int64(kfb), krb,
              n_out, T, Hq, Wq, Hk, Wk, 256, case.k, RC.TEMP, wm, b.eps, r2max, ry, rx,
              ops._ptr(views[0]), ops._ptr(views[1]), ops._ptr(views[2]), ops._ptr(ws), ops._stream(pi))
    torch.cuda.synchronize()
    stats = ws[:8].cpu().tolist()
    shape = (n_out, Hq * Wq, case.k)
    idx = views[0].cpu().reshape(shape)
    logit, weight = views[1].cpu().reshape(shape), views[2].cpu().reshape(shape)
    # every entry written, nothing outside the views touched
    assert not bool((idx == SENTINEL).any()), case.name
    assert not bool(torch.isnan(logit).any()) and not bool(torch.isnan(weight).any()), case.name
    for buf, pat in ((idx_buf, SENTINEL), (lg_buf.view(torch.int32), NAN_BITS), (w_buf.view(torch.int32), NAN_BITS)):
        assert bool((buf[:RC.GUARD] == pat).all()) and bool((buf[RC.GUARD + n:] == pat).all()), case.name
    assert not ops.pair_f16x3_timed_out()
    return dict(idx=idx, logit=logit, weight=weight, stats=stats)


def check(b, want, got, mode="softmax", what=None):
    case, k = b.case, b.case.k
    what = what or case.name
    held = torch.from_numpy(b.held)
    w_idx = torch.from_numpy(want["idx"])
    same = (got["idx"].long() == w_idx).all(-1)
    share = float(held.double().mean())
    bad = (held & ~same).nonzero()
    assert bad.numel() == 0, (what, "lists differ on held queries", bad[:5].tolist(), got["idx"][tuple(bad[0])].tolist(), w_idx[tuple(bad[0])].tolist(),
                              RC.PATHS[int(want["path"][tuple(bad[0].tolist())])])
    assert share >= RC.MIN_SHARE, (what, share)
    # logits and weights, on the held queries
    valid = (w_idx >= 0) & held.unsqueeze(-1)
    tail = (w_idx < 0) & held.unsqueeze(-1)
    w_lg = torch.from_numpy(want["score"]).double() / RC.TEMP
    lmax = float(w_lg[valid].abs().max())
    lerr = ((got["logit"].double() - w_lg).abs() / _ulp32(w_lg))[valid]
    exact = torch.from_numpy(want["exact"])
    e_x = float(lerr[exact[valid]].max()) if bool(exact[valid].any()) else 0.0
    e_a = float(lerr[~exact[valid]].max()) if bool((~exact[valid]).any()) else 0.0
    if mode == "softmax":
        w_w = torch.softmax(torch.where(w_idx >= 0, w_lg, torch.full_like(w_lg, float("-inf"))), -1)
        werr = float((got["weight"].double() - w_w).abs()[valid].max())
        # (logits of 8 and more -- the unnormalised dyadic rows -- take that module's bound for large logits, test_merge_large_logits)
        wbound, wunit = k * 2 * U + (0.0 if lmax < 8.0 else 2.5 * float(_ulp32(torch.tensor(lmax)))), ""
    else:
        w_w = w_lg.clamp_min(0.0) ** 2
        werr = float(((got["weight"].double() - w_w).abs() / _ulp32(w_w).clamp_min(1e-300))[valid].max())
        wbound, wunit = 4.0, " ulps"
    s = list(got["stats"])
    w4, w5 = (float(np.array([x], np.int32).view(np.float32)[0]) for x in s[4:6])
    print(f"{what} [{mode}]: held {int(held.sum())}/{held.numel()}, lists equal on {int(same.sum())}; logit err re-scored / from scratch {e_x:.2f} ulps, "
          f"as it stood {e_a:.2f} ulps (bound 2); weight err {werr:.3e}{wunit} (bound {wbound:.3e}); max |logit| {lmax:.2f}; words {s[:4]} + sample {s[6:8]} "
          f"(restated {want['words']}); word 4 {w4:.6e} vs {want['err_rescored']:.6e}, word 5 {w5:.6e} vs {want['err_sampled']:.6e} (eps {b.eps:.3e}); "
          f"paths {want['counts']}")
    assert e_x <= 2 and e_a <= 2 and werr <= wbound, (what, e_x, e_a, werr)
    if bool(tail.any()):
        assert bool((got["idx"][tail] == -1).all()) and bool((got["logit"][tail] == float("-inf")).all()) and bool((got["weight"][tail] == 0).all()), what
    ww = want["words"]
    assert [s[0] - s[7], s[1], s[2], s[3], s[6], s[7]] == [ww[0], ww[1], ww[2], ww[3], ww[6], ww[7]], (what, s, ww)
    assert w4 <= b.eps and abs(w4 - want["err_rescored"]) <= U, (what, w4, want["err_rescored"])
    assert w5 <= want["err_listed"] and abs(w5 - want["err_sampled"]) <= U, (what, w5, want["err_sampled"], want["err_listed"])
    if want["unflagged"] > 1000:
        assert s[7] > 0 and s[6] > 0 and w5 > 0, (what, s)


@pytest.mark.parametrize("case", RC.CASES, ids=RC.case_id)
def test_refining_merge_matches_the_restated_rule(dev, case):
    """Every case of the table (refine_cases.CASES: what each one reaches is in its name and in its floors, which the CPU module asserts)."""
    b, want = RC.built(case.name), RC.restated(case.name)
    check(b, want, launch(b, dev))


def test_cosine_weights(dev):
    """weight_mode = cosine on the case with partly open scans: the same lists and logits, weights max(logit, 0)^2 within 4 ulps."""
    name = "c02_neartie_alt_some_open"
    b, want = RC.built(name), RC.restated(name)
    got = launch(b, dev, mode="cosine")
    check(b, want, got, mode="cosine")
    soft = launch(b, dev)
    assert torch.equal(got["idx"], soft["idx"]) and torch.equal(got["logit"], soft["logit"])
    assert bool((got["weight"] > 0).any())


@pytest.mark.parametrize("name", ["c02_neartie_alt_some_open", "c03_twins_neartie_edge"])
def test_bank_forms_agree(dev, name):
    """One f32 tensor for both sides, query and key rows in two tensors (each NaN where only the other may be read), and 2 KiB
    f16f6x rows with the f32 channels in their second KiB: the same bits out."""
    b, want = RC.built(name), RC.restated(name)
    outs = {bank: launch(b, dev, bank=bank) for bank in ("f32", "separate", "f16f6x")}
    for bank, got in outs.items():
        check(b, want, got, what=f"{name} bank {bank}")
        for key in ("idx", "logit", "weight"):
            assert torch.equal(got[key], outs["f32"][key]), (bank, key)
        assert got["stats"] == outs["f32"]["stats"], bank


def test_wrapper_is_the_entry_point(dev):
    """ops.merge_refine_topk on the same lists: the bits of the direct call, its statistics tensor the workspace's first eight words."""
    from fgvc_amd import ops
    name = "c03_twins_neartie_edge"
    b, want = RC.built(name), RC.restated(name)
    direct = launch(b, dev)
    Hq, Wq = b.case.grid
    rows = torch.from_numpy(b.k_rows).to(dev)
    t = lambda x: torch.from_numpy(x).to(dev)
    idx, logit, weight, stats = ops.merge_refine_topk(t(b.pair_idx), t(b.pair_score), t(b.slot_pair), t(b.pairs), rows, rows, Hq, Wq, Hq, Wq,
                                                      ops.MaskSpec(*b.case.mask), b.case.k, RC.TEMP, "softmax", eps=b.eps)
    got = dict(idx=idx.cpu(), logit=logit.cpu(), weight=weight.cpu(), stats=stats.cpu().tolist())
    assert got["idx"].dtype == torch.int32 and got["idx"].shape == (1, Hq * Wq, b.case.k)
    for key in ("idx", "logit", "weight", "stats"):
        assert (got[key] == direct[key]) if key == "stats" else torch.equal(got[key], direct[key]), key
    check(b, want, got, what=f"{name} through ops.merge_refine_topk")


def test_from_scratch_beyond_the_scan_queue_with_two_slots(dev):
    """66 x 64 = 4224 queries, every one from scratch with both slots open, against a scan queue of 4096: the statistics report 128
    items beyond it, recomputed candidate by candidate inside refine_inline_kernel (every slot under the square mask's ry / rx), and
    every one is right.  Which 128 queries overflow depends on the order the waves reach the queue: all are held to one statement."""
    b, want = RC.built(RC.OVERFLOW.name), RC.restated(RC.OVERFLOW.name)
    assert want["words"][1] == 4224 and want["words"][3] == 128
    check(b, want, launch(b, dev))


def test_workspace_reuse(dev):
    """Two different cases through ONE workspace, then the first again: counters and scan_done are zeroed by every launch, no result
    depends on what the previous call left behind (items, queue, parts)."""
    from fgvc_amd import ops
    A, B = "c03_twins_neartie_edge", "c10_product_layout_two_rows"
    ba, bb = RC.built(A), RC.built(B)
    ws = ops.merge_refine_workspace(2, bb.pair_idx.shape[1], dev)
    ws.fill_(-1)
    first = launch(ba, dev, ws=ws)
    check(ba, RC.restated(A), first, what=f"{A} first")
    check(bb, RC.restated(B), launch(bb, dev, ws=ws), what=f"{B} in the same workspace")
    again = launch(ba, dev, ws=ws)
    check(ba, RC.restated(A), again, what=f"{A} again")
    for key in ("idx", "logit", "weight"):
        assert torch.equal(first[key], again[key]), key
    assert first["stats"] == again["stats"]


def test_three_launches_bit_identical(dev):
    """The queue order, the scan's last-workgroup merge and the atomics differ from launch to launch; the outputs may not."""
    name = "c03_twins_neartie_edge"
    b = RC.built(name)
    outs = [launch(b, dev) for _ in range(3)]
    for o in outs[1:]:
        for key in ("idx", "logit", "weight"):
            assert torch.equal(o[key], outs[0][key]), key
        assert o["stats"] == outs[0]["stats"]
