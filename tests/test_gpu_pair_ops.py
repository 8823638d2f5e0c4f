"""GPU: the four pair top-k kernels -- fgvc_pair_topk_f32 (csrc/pair_topk.hip), fgvc_pair_topk_f16x3[_runs] (pair_topk_v5.hip),
fgvc_pair_topk_f16f6[x][_runs] (pair_topk_v7.hpp) and the opt-in v8 (pair_topk_v8.hpp) -- held to EXACT lists on planted rows
(tests/pair_cases.py; what the rows and the checker are worth is shown on the CPU by tests/test_pair_reference_share.py).

Every planted score is exact in every arithmetic, so PC.check_lists runs without a tolerance: the k scores equal the float64 top-k scores
bit for bit on EVERY query (short windows, fully rejected queries, ties across the k-th place included), indices are distinct, admitted by
the mask and in (score descending, index ascending) order, empties are exactly the missing ones and sit at the tail; on the graded family
and for v8 the index list is the canonical one.  Real-valued rows get the same structural rules and the score bar of each kernel's
existing test (1e-3 logit f32: test_gpu_parity.TOL; 5e-5 logit f16x3; 2e-4 logit f16f6)."""
import ctypes

import pytest
import torch

from tests import pair_cases as PC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fgvc_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _mask(case):
    from fgvc_amd import ops
    return ops.MaskSpec(*case.mask)


def _check(b, rows, idx, score, k, canonical, tol=0.0):
    idx, score = idx.cpu(), score.cpu()
    stats = []
    for pi, row in enumerate(rows):
        try:
            stats.append(PC.check_lists(PC.slab64(b, row), idx[pi], score[pi], k, canonical=canonical, tol=tol))
        except AssertionError as e:
            raise AssertionError(f"{b.case.name} pair {pi} {row} k={k}: {e}") from None
    return stats


def _f32(b, dev, rows, k):
    from fgvc_amd import ops
    c = b.case
    qf = b.qfeat.to(dev)
    kf = qf if b.kfeat is b.qfeat else b.kfeat.to(dev)
    dm = None if b.dense_mask is None else b.dense_mask.to(dev)
    return ops.pair_topk(qf, kf, ops.make_pairs(rows, dev), *c.qgrid, *c.kgrid, _mask(c), k, dense_mask=dm)


def _split(b, dev, rows, k, fmt, all_masked, v8=False):
    """(idx, score) of the split kernel of `fmt` with runs, after requiring the launch without runs to give the same bits"""
    from fgvc_amd import ops
    c = b.case
    splitter = {"f16": ops.split_f16x2, "f16f6": ops.split_f16f6p, "f16f6x": ops.split_f16f6x}[fmt]
    qs = splitter(b.qfeat.to(dev))
    ks = qs if b.kfeat is b.qfeat else splitter(b.kfeat.to(dev))
    pairs = ops.make_pairs(rows, dev)
    if v8:
        ops.set_option("pair_f16_debug", PC.V8)
    try:
        ia, sa = ops.pair_topk_split(qs, ks, pairs, *c.qgrid, *c.kgrid, _mask(c), k, all_masked=all_masked, fmt=fmt)
        ib, sb = ops.pair_topk_split(qs, ks, pairs, *c.qgrid, *c.kgrid, _mask(c), k, all_masked=all_masked, fmt=fmt, use_runs=False)
        torch.cuda.synchronize()
    finally:
        if v8:
            ops.set_option("pair_f16_debug", 0)
    assert torch.equal(ia, ib) and torch.equal(sa, sb), f"{c.name} {fmt}{' v8' if v8 else ''}: runs and single pairs differ"
    return ia, sa


@pytest.mark.parametrize("case", PC.ALL_PLANTED, ids=PC.case_id)
def test_pair_f32_planted_lists_are_exact(dev, case):
    """fgvc_pair_topk_f32 on every planted case: analytic masks, none, dense user masks (a pair without PAIR_MASKED in the same launch),
    unequal grids, C = 32 .. 256, k = 1 .. 16 (every K instantiation and the kout < K cases 2, 6, 11)"""
    from fgvc_amd import ops
    b = PC.built(case.name)
    if case.dense:
        assert any(r[2] for r in b.rows) and any(not r[2] for r in b.rows)
    for k in sorted({case.k32, case.ksplit} - {0}):
        idx, score = _f32(b, dev, b.rows, k)
        _check(b, b.rows, idx, score, k, canonical=case.family == "graded")
    assert not ops.pair_f16x3_timed_out()


@pytest.mark.parametrize("case", [c for c in PC.PLANTED_EQUAL + PC.UNEQUAL if c.split_ok], ids=PC.case_id)
def test_pair_split_planted_lists_are_exact(dev, case):
    """fgvc_pair_topk_f16x3 (masked and unmasked rows mixed; unequal grids without a mask) and, where every pair can be masked within 64
    key blocks, fgvc_pair_topk_f16f6, fgvc_pair_topk_f16f6x and v8 of both: with runs and pair by pair, bit-identical, exact"""
    from fgvc_amd import ops
    b = PC.built(case.name)
    k, graded = case.ksplit, case.family == "graded"
    mask = _mask(case)
    assert ops.split_path_ok(256, *case.kgrid, k, True, None, mask, False)
    idx, score = _split(b, dev, b.rows, k, "f16", all_masked=False)
    _check(b, b.rows, idx, score, k, canonical=graded)
    if case.has_mask and case.equal:
        rows = b.rows_for(True)
        if rows != b.rows:                                           # every pair masked: only the mask's reach is listed
            idx, score = _split(b, dev, rows, k, "f16", all_masked=True)
            _check(b, rows, idx, score, k, canonical=graded)
        if ops.pair_f16f6_ok(256, *case.kgrid, k, True, None, mask, True):
            for fmt in ("f16f6", "f16f6x"):
                i7, s7 = _split(b, dev, rows, k, fmt, all_masked=True)
                _check(b, rows, i7, s7, k, canonical=graded)
                i8, s8 = _split(b, dev, rows, k, fmt, all_masked=True, v8=True)
                _check(b, rows, i8, s8, k, canonical=True)
                assert torch.equal(s7, s8)
    assert not ops.pair_f16x3_timed_out()


@pytest.mark.parametrize("big", PC.BIG, ids=[f"{g[0]}x{g[1]}-{n}blocks-{what}" for g, n, what in PC.BIG])
def test_pair_f16x3_list_size_boundaries(dev, big):
    """one unmasked pair, a one-tile query grid against a key grid of 2048 blocks (the three-role form's capacity), 2080 (the two-role
    form takes over) and 4096 (the list's capacity): exact lists, and the f32 kernel's scores bit for bit"""
    from fgvc_amd import ops
    kgrid, blocks, _ = big
    assert ops.pair_blocks_needed(*kgrid) == blocks and ops.split_path_ok(256, *kgrid, PC.BIG_K, True)
    qf, kf, slab = PC.big_rows(kgrid)
    qf, kf = qf.to(dev), kf.to(dev)
    pairs = ops.make_pairs([(0, 0, False)], dev)
    none = ops.MaskSpec.none()
    i32, s32 = ops.pair_topk(qf, kf, pairs, *PC.BIG_Q, *kgrid, none, PC.BIG_K)
    qs, ks = ops.split_f16x2(qf), ops.split_f16x2(kf)
    ia, sa = ops.pair_topk_split(qs, ks, pairs, *PC.BIG_Q, *kgrid, none, PC.BIG_K, fmt="f16")
    ib, sb = ops.pair_topk_split(qs, ks, pairs, *PC.BIG_Q, *kgrid, none, PC.BIG_K, fmt="f16", use_runs=False)
    timed_out = ops.pair_f16x3_timed_out()                             # read (and cleared) before anything below can raise
    assert torch.equal(ia, ib) and torch.equal(sa, sb)
    assert torch.equal(sa, s32), f"{int((sa != s32).sum())} scores differ from the f32 kernel's"
    PC.check_lists(slab, ia[0].cpu(), sa[0].cpu(), PC.BIG_K)
    assert not timed_out


def test_pair_f16x3_refuses_one_block_more(dev):
    """4160 key blocks, one block column more than the list holds: ops.split_path_ok, the C entry and the Python wrapper refuse alike"""
    from fgvc_amd import _lib, ops
    Hk, Wk = PC.BIG_REFUSED
    Hq, Wq = PC.BIG_Q
    assert ops.pair_blocks_needed(Hk, Wk) == 4160 and not ops.split_path_ok(256, Hk, Wk, PC.BIG_K, True)
    lib = _lib.load()
    qs = torch.zeros((1, Hq * Wq, 2, 256), dtype=torch.int16, device=dev)
    ks = torch.zeros((1, Hk * Wk, 2, 256), dtype=torch.int16, device=dev)
    pairs = ops.make_pairs([(0, 0, False)], dev)
    idx = torch.empty((1, Hq * Wq, PC.BIG_K), dtype=torch.int32, device=dev)
    sc = torch.empty((1, Hq * Wq, PC.BIG_K), dtype=torch.float32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = lib.fgvc_pair_topk_f16x3(P(qs), P(ks), P(pairs), 1, 256, Hq, Wq, Hk, Wk, _lib.NO_LIMIT, _lib.NO_LIMIT, _lib.NO_LIMIT, PC.BIG_K, 0,
                                  P(idx), P(sc), None)
    assert rc == _lib.ERR_UNSUPPORTED
    with pytest.raises(_lib.FgvcHipError):
        ops.pair_topk_split(qs, ks, pairs, Hq, Wq, Hk, Wk, ops.MaskSpec.none(), PC.BIG_K, fmt="f16")
    torch.cuda.synchronize()
    assert not ops.pair_f16x3_timed_out()


def test_pair_f16f6_block_limit(dev):
    """the masks the CPU sweep finds at 64 key blocks run (and give exact lists on an 8 x 16 grid); the smallest masks above 64 are
    refused by the C entry (FGVC_ERR_UNSUPPORTED) and by ops.pair_f16f6_ok alike"""
    from fgvc_amd import _lib, ops
    H, W, k = 8, 16, 10
    at, above = PC.limit_masks()
    lib = _lib.load()
    b0 = PC.built(next(c.name for c in PC.PLANTED_EQUAL if c.qgrid == (H, W) and c.family == "codebook"))
    feats = b0.qfeat.to(dev)
    sp = ops.split_f16f6p(feats)
    rows = [(0, 0, True), (0, 1, True), (1, 0, True)]
    pairs = ops.make_pairs(rows, dev)
    idx = torch.empty((3, H * W, k), dtype=torch.int32, device=dev)
    sc = torch.empty((3, H * W, k), dtype=torch.float32, device=dev)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda m: lib.fgvc_pair_topk_f16f6(P(sp), P(sp), P(pairs), 3, 256, H, W, H, W, m[0], m[1], m[2], k, 1, P(idx), P(sc), None)
    for m in at:
        assert ops.pair_f16f6_ok(256, H, W, k, True, None, ops.MaskSpec(*m), True), m
        assert call(m) == 0, m
        torch.cuda.synchronize()
        adm = PC.analytic_admit((H, W), m)
        for pi, (q, kk, _) in enumerate(rows):
            slab = (b0.kfeat[kk].double() @ b0.qfeat[q].double().t()).masked_fill(~adm, PC.NEG_INF)
            PC.check_lists(slab, idx[pi].cpu(), sc[pi].cpu(), k)
    for m in above:
        assert not ops.pair_f16f6_ok(256, H, W, k, True, None, ops.MaskSpec(*m), True), m
        assert call(m) == _lib.ERR_UNSUPPORTED, m
        with pytest.raises(ValueError):
            ops.pair_topk_split(sp, sp, pairs, H, W, H, W, ops.MaskSpec(*m), k, all_masked=True, fmt="f16f6")
    torch.cuda.synchronize()
    assert not ops.pair_f16x3_timed_out()


@pytest.mark.parametrize("case", PC.GAUSS, ids=PC.case_id)
def test_pair_kernels_real_valued_rows(dev, case):
    """Gaussian unit rows at the short-window shapes: distinct, admitted, ordered, empties at the tail exactly; scores at each kernel's
    existing bar (raw dot products: logit bar x 0.07)"""
    from fgvc_amd import ops
    b = PC.built(case.name)
    mask = _mask(case)
    idx, score = _f32(b, dev, b.rows, case.k32)
    _check(b, b.rows, idx, score, case.k32, False, tol=1e-3 * PC.TAU)
    k = case.ksplit
    idx, score = _split(b, dev, b.rows, k, "f16", all_masked=False)
    _check(b, b.rows, idx, score, k, False, tol=5e-5 * PC.TAU)
    if case.has_mask and ops.pair_f16f6_ok(256, *case.kgrid, k, True, None, mask, True):
        rows = b.rows_for(True)
        for fmt in ("f16f6", "f16f6x"):
            for v8 in (False, True):
                idx, score = _split(b, dev, rows, k, fmt, all_masked=True, v8=v8)
                _check(b, rows, idx, score, k, False, tol=2e-4 * PC.TAU)
    assert not ops.pair_f16x3_timed_out()
