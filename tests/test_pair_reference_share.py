"""CPU: what tests/test_gpu_pair_ops.py relies on, checked from the planted rows and the oracle alone (tests/pair_cases.py).

* Every planted case is EXACT: the float64 slab is integral at the family's scale, equals the f32 product, the f16-parts model (l = 0) and
  O.f16f6_cosines of the encoded rows (FP6 residuals 0), and stays within |q.k| <= 1 wherever a split kernel sees it.
* Every case reaches the edge it is named for; the counts are printed (docs/LAB_NOTES.md) and held to floors that follow from the masks
  and the frame kinds alone.
* check_lists passes the canonical list and raises on five mutants of it.
* ops.pair_blocks_reached agrees with a brute-force count over pixels on 1485 masks, and the masks at and just above the 64-block limit
  that the GPU module sends to the C entry are what the sweep says they are.
"""
import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import pair_cases as PC
from tests import volume_cases as VC


def _enc(frame):
    return O.f16f6p_encode(frame.numpy())


@pytest.mark.parametrize("case", PC.ALL_PLANTED, ids=PC.case_id)
def test_planted_case_is_exact(case):
    b = PC.built(case.name)
    assert b.scale > 0
    enc = {}
    for (q, k, _) in sorted(set((q, k, True) for q, k, _ in b.rows)):
        s = PC.raw64(b, q, k)
        assert bool((s * b.scale == (s * b.scale).round()).all()), "the slab is not integral at the family's scale"
        assert torch.equal((b.kfeat[k] @ b.qfeat[q].t()).double(), s), "the f32 product differs from float64"
        if not case.split_ok:
            continue
        assert float(s.abs().max()) <= 1.0
        parts = []
        for x in (b.qfeat[q], b.kfeat[k]):
            h, l = VC.f16_parts_host(x)                                   # h = f16(256 x), l = 256 (256 x - h)
            assert not l.any() and np.array_equal(h / 256.0, x.double().numpy()), "the f16 part is not the value itself"
            x14 = x.numpy() * np.float32(16384.0)                         # fgvc_split_f16x2: h = f16(2^14 x), l = f16(2^14 x - h)
            assert np.array_equal(x14.astype(np.float16).astype(np.float32), x14)
            parts.append(torch.from_numpy(h))
        assert torch.equal(parts[1] @ parts[0].t() / 65536.0, s), "the f16-parts model differs from float64"
        for side, f, t in (("q", q, b.qfeat), ("k", k, b.kfeat)):
            if (side, f) not in enc:
                enc[(side, f)] = _enc(t[f])
                hh, _, l6 = O.f16f6p_decode(enc[(side, f)])
                assert not l6.any() and np.array_equal(hh / 256.0, t[f].double().numpy()), "an FP6 residual is not zero"
        assert np.array_equal(O.f16f6_cosines(enc[("q", q)], enc[("k", k)]), s.numpy()), "O.f16f6_cosines differs from float64"


def _floors(b, row, k):
    """what the masks and the frame kinds alone promise of one (pair row, k): lower bounds on edge_counts' figures"""
    q, kk, masked = row
    HWk, HWq = b.kfeat.shape[1], b.qfeat.shape[1]
    adm = PC.admitted(b, masked)
    nwin = torch.full((HWq,), HWk) if adm is None else adm.sum(0)
    f = dict(short=int(((nwin < k) & (nwin > 0)).sum()), rejected=int((nwin == 0).sum()), tied_kth=0, minus1=0, zero=0, plus1=0)
    kind = b.kinds[kk]
    if b.case.family == "codebook" and b.case.equal:
        unit = (b.qfeat[q].double() ** 2).sum(1) == 1.0                   # the pixels that drew a unit row (the others drew a zero row)
        self_in = torch.ones(HWq, dtype=torch.bool) if adm is None else adm.diagonal()
        if kind == "zero":
            f["zero"] = int((nwin > 0).sum())                              # every admitted score is 0
            f["tied_kth"] = int((nwin > k).sum())
        elif kk == q and b.kinds[q] != "zero":
            f["plus1"] = int((unit & self_in).sum())                       # 1 is the largest score there is: always listed
        elif {b.kinds[q], kind} == {"draw", "neg0"} and 0 in (q, kk):
            f["minus1"] = int((unit & self_in & (nwin <= k)).sum())        # -1 is the smallest: listed where the window holds at most k
    return f


@pytest.mark.parametrize("case", PC.ALL_PLANTED, ids=PC.case_id)
def test_case_reaches_its_edge(case):
    b = PC.built(case.name)
    total, floor = {}, {}
    for row in b.rows + ([r for r in b.rows_for(True) if r not in b.rows] if case.split_ok and case.has_mask else []):
        for k in sorted({case.k32, case.ksplit} - {0}):
            slab = PC.slab64(b, row)
            got, want = PC.edge_counts(slab, k), _floors(b, row, k)
            if case.family == "graded":
                assert not got["any_tie"], "two finite scores of one window tie in a graded case"
            for name in want:
                assert got[name] >= want[name], (case.name, row, k, name, got, want)
                total[name] = total.get(name, 0) + got[name]
                floor[name] = floor.get(name, 0) + want[name]
    print(f"{case.name}: rows {len(b.rows)} " + " ".join(f"{n} {total[n]} (>= {floor[n]})" for n in total))
    # the edge in the case's name
    if case.has_mask and PC.window_size(case.mask) < max(case.k32, case.ksplit):      # the whole window is smaller than a list
        assert total["short"] >= b.qfeat.shape[1]
    if case.dense == "bern":
        assert total["rejected"] >= 3
    if case.family == "codebook" and case.equal:
        assert total["plus1"] > 0 and (total["zero"] > 0 or "zero" not in b.kinds)


def test_the_table_reaches_every_edge():
    """summed over the planted table: each edge is met on hundreds of queries (per case figures: the test above)"""
    total = {}
    for case in PC.ALL_PLANTED:
        b = PC.built(case.name)
        for row in b.rows:
            for name, v in PC.edge_counts(PC.slab64(b, row), case.k32).items():
                total[name] = total.get(name, 0) + int(v)
    print(total)
    n_bern = sum(c.dense == "bern" for c in PC.DENSE)                      # three all-false columns in at least one masked pair each
    for name, floor in (("short", 1000), ("tied_kth", 1000), ("minus1", 100), ("zero", 1000), ("plus1", 1000), ("rejected", 3 * n_bern)):
        assert total[name] >= floor, (name, total)


def _find(pred):
    """the first (slab, canonical idx, canonical score, query, k) over the codebook cases for which pred(...) returns a mutant"""
    for case in PC.PLANTED_EQUAL:
        if case.family != "codebook" or not case.has_mask:
            continue
        b = PC.built(case.name)
        for row in b.rows:
            if not row[2]:
                continue
            slab = PC.slab64(b, row)
            k = case.k32
            ci, cv = PC.canonical_lists(slab, k)
            for s in range(slab.shape[1]):
                m = pred(slab, PC.raw64(b, row[0], row[1]), ci[s].clone(), cv[s].clone(), s, k)
                if m is not None:
                    ci, cv = ci.clone(), cv.clone()
                    ci[s], cv[s] = m
                    return slab, ci, cv, k
    raise AssertionError("no query of the table admits this mutant")


def _dup(slab, raw, i, v, s, k):
    if k >= 2 and i[1] >= 0:
        i[1], v[1] = i[0], v[0]
        return i, v


def _swap_tied(slab, raw, i, v, s, k):
    for j in range(k - 1):
        if i[j + 1] >= 0 and v[j] == v[j + 1]:
            i[j], i[j + 1] = i[j + 1].clone(), i[j].clone()
            return i, v


def _outside(slab, raw, i, v, s, k):
    for j in range(k):
        if i[j] >= 0:
            out = ((raw[:, s] == v[j]) & ~torch.isfinite(slab[:, s])).nonzero()
            if len(out) and (j == 0 or v[j - 1] > v[j]) and (j == k - 1 or v[j + 1] < v[j]):      # order stays valid whatever the index
                i[j] = out[0, 0]
                return i, v


def _empty_inside(slab, raw, i, v, s, k):
    live = int((i >= 0).sum())
    if 1 <= live < k:
        i[live], v[live], i[live - 1], v[live - 1] = i[live - 1].clone(), v[live - 1].clone(), -1, PC.NEG_INF
        return i, v


def _tie_for_better(slab, raw, i, v, s, k):
    if k >= 2 and i[k - 1] >= 0 and v[0] > v[k - 1]:
        spare = ((slab[:, s] == v[k - 1]) & ~torch.isin(torch.arange(slab.shape[0]), i)).nonzero()
        if len(spare):                                  # drop the best entry, append an unlisted member of the k-th-place tie (a higher index)
            return torch.cat([i[1:], spare[-1]]), torch.cat([v[1:], v[k - 1:]])


MUTANTS = [(_dup, "distinct"), (_swap_tied, "order"), (_outside, "not admitted"), (_empty_inside, "empties"),
           (_tie_for_better, "scores|membership")]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0].__name__.strip("_") for m in MUTANTS])
def test_check_lists_raises_on_a_mutant(mutant):
    make, rule = mutant
    slab, ci, cv, k = _find(make)
    good_i, good_v = PC.canonical_lists(slab, k)
    PC.check_lists(slab, good_i, good_v, k, canonical=True)
    with pytest.raises(AssertionError, match=rule):
        PC.check_lists(slab, ci, cv, k)
    with pytest.raises(AssertionError):
        PC.check_lists(slab, ci, cv, k, tol=1e-6)


def test_check_lists_lets_any_member_of_a_kth_place_tie_pass_but_not_as_canonical():
    def other_tie(slab, raw, i, v, s, k):
        if i[k - 1] >= 0 and (k == 1 or v[k - 2] > v[k - 1]):
            spare = ((slab[:, s] == v[k - 1]) & ~torch.isin(torch.arange(slab.shape[0]), i)).nonzero()
            if len(spare):
                i[k - 1] = spare[-1, 0]
                return i, v
    slab, ci, cv, k = _find(other_tie)
    PC.check_lists(slab, ci, cv, k)
    with pytest.raises(AssertionError, match="canonical"):
        PC.check_lists(slab, ci, cv, k, canonical=True)


def test_tolerance_variant_keeps_the_exact_rules():
    """real-valued rows: the canonical list passes at tol = 0 and with a perturbation below tol; the structural mutants still raise"""
    case = PC.GAUSS[1]
    b = PC.built(case.name)
    row = next(r for r in b.rows if r[2])
    slab, k = PC.slab64(b, row), case.k32
    ci, cv = PC.canonical_lists(slab, k)
    PC.check_lists(slab, ci, cv, k, canonical=True)
    wob = torch.where(torch.isfinite(cv), cv.float().double(), cv)        # the scores rounded to f32: a perturbation of up to 6e-8
    PC.check_lists(slab, ci, torch.sort(wob, dim=1, descending=True).values, k, tol=1e-6)
    with pytest.raises(AssertionError, match="scores"):
        PC.check_lists(slab, ci, cv + 1e-3 * torch.isfinite(cv), k, tol=1e-6)
    s = int((ci[:, 1] >= 0).nonzero()[0])
    dup = ci.clone()
    dup[s, 1] = dup[s, 0]
    with pytest.raises(AssertionError, match="distinct"):
        PC.check_lists(slab, dup, cv, k, tol=1.0)


def test_big_rows_are_exact():
    qf, kf, slab = PC.big_rows(PC.BIG[0][0])
    assert torch.equal(kf[0].double() @ qf[0].double().t(), slab) and bool((slab * 256 == (slab * 256).round()).all())
    assert torch.equal((kf[0] @ qf[0].t()).double(), slab)
    e = PC.edge_counts(slab, PC.BIG_K)
    print("big rows:", e)
    assert e["tied_kth"] >= 64 and e["plus1"] >= 64
    for kg, blocks, _ in PC.BIG:
        assert -(-kg[0] // 4) * -(-kg[1] // 8) == blocks
    assert -(-PC.BIG_REFUSED[0] // 4) * -(-PC.BIG_REFUSED[1] // 8) == 4160


def test_pair_blocks_reached_against_brute_force():
    from fgvc_amd import ops
    masks = PC.sweep_masks()
    bad = [(m, ops.pair_blocks_reached(ops.MaskSpec(*m)), PC.blocks_reached_brute(*m)) for m in masks
           if ops.pair_blocks_reached(ops.MaskSpec(*m)) != PC.blocks_reached_brute(*m)]
    assert not bad, (len(bad), bad[:5])
    at, above = PC.limit_masks()
    print(f"{len(masks)} masks; at the limit {at}; just above {above}")
    assert len(at) >= 4 and len(above) >= 3
    for m in at:
        assert 60 <= PC.blocks_reached_brute(*m) <= 64 and ops.pair_f16f6_ok(256, 8, 16, 10, True, None, ops.MaskSpec(*m), True)
    assert sum(PC.blocks_reached_brute(*m) == 64 for m in at) >= 4
    for m in above:
        assert PC.blocks_reached_brute(*m) > 64 and not ops.pair_f16f6_ok(256, 8, 16, 10, True, None, ops.MaskSpec(*m), True)
        assert ops.split_path_ok(256, 8, 16, 10, True, None, ops.MaskSpec(*m), True)
    # the list capacity of fgvc_pair_topk_f16x3, as ops states it
    for kg, blocks, _ in PC.BIG:
        assert ops.pair_blocks_needed(*kg) == blocks and ops.split_path_ok(256, kg[0], kg[1], PC.BIG_K, True)
    assert not ops.split_path_ok(256, PC.BIG_REFUSED[0], PC.BIG_REFUSED[1], PC.BIG_K, True)
