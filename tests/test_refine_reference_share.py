"""CPU: what tests/test_gpu_refine_ops.py relies on, checked from the restatement and the oracle alone (tests/refine_cases.py).

* The restatement of refine.hip's rule yields, on every held query, the oracle's canonical top-k (O.topk_canonical) of the float64 slab
  of exact scores: the rule is right on lists whose approximate scores sit AT the bound the proof assumes, not a third of the way to it.
* Twins (one key frame in two slots) appear as the oracle has them: the lower slot first.
* Every case holds at least 95 % of its queries and reaches the path it is named for (the counts are printed: docs/LAB_NOTES.md).
* The builder's contract check is live: `delta` scaled by 1.5 trips it.
"""
import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import refine_cases as RC

ALL = RC.CASES + RC.CPU_ONLY


@pytest.mark.parametrize("case", ALL + [RC.OVERFLOW], ids=RC.case_id)
def test_restatement_is_the_canonical_topk_on_held_queries(case):
    b, r = RC.built(case.name), RC.restated(case.name)
    n_out, HWq, k = r["idx"].shape
    HWk = b.s32.shape[1]
    share = float(b.held.mean())
    equal = 0
    for f in range(n_out):
        slab = RC.slab64(b, f)
        kk = min(k, slab.shape[0])
        val, di = O.topk_canonical(slab, kk)
        want = torch.full((HWq, k), -1, dtype=torch.int64)
        want[:, :kk] = torch.where(torch.isfinite(val.t()), di.t(), torch.full_like(di.t(), -1))
        same = (torch.from_numpy(r["idx"][f]) == want).all(1).numpy()
        equal += int(same.sum())
        bad = np.nonzero(b.held[f] & ~same)[0]
        assert bad.size == 0, (case.name, f, bad[:5].tolist(), r["idx"][f][bad[:1]].tolist(), want[bad[:1]].tolist())
        # the scores the final entries carry: s32 of the entry where the rule re-scored, a where it did not -- never anything else
        gid = np.maximum(r["idx"][f], 0)
        pid = b.slot_pair[f][gid // HWk]
        qq = np.broadcast_to(np.arange(HWq)[:, None], gid.shape)
        live = r["idx"][f] >= 0
        src = np.where(r["exact"][f], b.s32[pid, gid % HWk, qq], b.a[pid, gid % HWk, qq])
        assert np.array_equal(r["score"][f][live], src[live])
    print(f"{case.name}: held {int(b.held.sum())}/{b.held.size} = {share:.4f}, equal to the canonical list {equal}/{b.held.size}, paths {r['counts']}, "
          f"words {r['words']}, max |a - s32| listed {r['err_listed']:.3e} re-scored {r['err_rescored']:.3e} sampled {r['err_sampled']:.3e} (eps {b.eps:.3e})")
    assert share >= RC.MIN_SHARE
    if case.kind in ("dyadic", "ladder"):
        assert bool(b.held.all())
    for path, floor in case.floors:
        assert r["counts"][path] >= floor, (case.name, path, r["counts"])
    assert r["err_listed"] <= b.eps and r["err_rescored"] <= b.eps


def test_twins_lower_slot_first():
    """A key frame in slots 0 and 1: every pixel of it that reaches the final list is followed by its twin, (pixel, slot 0) in front of
    (pixel, slot 1) with nothing but entries of exactly their score between them, on the re-scored and the from-scratch path alike
    (the restatement's lists ARE the oracle's canonical ones: the test above)."""
    for name in ("c03_twins_neartie_edge", "c12_eps_zero_twins", "c10_product_layout_two_rows"):
        b, r = RC.built(name), RC.restated(name)
        HWk = b.s32.shape[1]
        assert b.slot_pair[0, 0] == b.slot_pair[0, 1]
        seen, direct = set(), 0
        for q in range(r["idx"].shape[1]):
            ids, sc = r["idx"][0, q].tolist(), r["score"][0, q].tolist()
            for j, g in enumerate(ids):
                if 0 <= g < HWk:
                    # (only entries of exactly the twins' score may stand between them, or push the second one off the list's end)
                    j2 = ids.index(g + HWk) if g + HWk in ids else len(ids)
                    assert j2 > j and all(s == sc[j] for s in sc[j:min(j2 + 1, len(ids))]), (name, q, ids, sc)
                    direct += j2 == j + 1
                    seen.add(int(r["path"][0, q]))
        assert direct >= 100, (name, direct)
        if name == "c10_product_layout_two_rows":
            assert len(seen) >= 2, (name, seen)                                  # on more than one path


def test_dyadic_cases_have_the_ties_they_are_for():
    """Exact ties across the k-th place, exact ties across slots, and neighbours of the merged order exactly 2 eps apart in a."""
    for name in ("c11_dyadic_alt", "c11_dyadic_edge", "c11_dyadic_rand_k7"):
        b = RC.built(name)
        k, HWk = b.case.k, b.s32.shape[1]
        kth_tie = slot_tie = two_eps = 0
        for q in range(b.pair_idx.shape[1]):
            slab = RC.slab64(b, 0)[:, q].numpy()
            srt = np.sort(slab)[::-1]
            kth_tie += srt[k - 1] == srt[k]
            top = np.argsort(-slab, kind="stable")[:k]
            vals = {}
            for g in top:
                vals.setdefault(slab[g], set()).add(b.slot_pair[0, g // HWk])
            slot_tie += any(len(v) > 1 for v in vals.values())
            listed = sorted((float(s) for t, pid in enumerate(b.slot_pair[0]) for s, i in zip(b.pair_score[pid, q], b.pair_idx[pid, q]) if i >= 0), reverse=True)
            two_eps += any(x - y == 2 * b.eps for x, y in zip(listed[:RC.KX], listed[1:RC.KX]))
        print(f"{name}: ties across the k-th place {kth_tie}, across slots inside the top k {slot_tie}, neighbours exactly 2 eps apart {two_eps} (of {b.pair_idx.shape[1]} queries)")
        assert kth_tie >= 5 and slot_tie >= 5 and two_eps >= 5


def test_contract_check_is_live():
    """delta scaled by 1.5 leaves the bound: the builder's assertion must fail (and does not at scale 1)."""
    for name in ("c01_gauss_alt", "c04_wide_eps_over16_in_window", "c11_dyadic_edge"):
        RC.build(RC.BY_NAME[name])
        with pytest.raises(AssertionError):
            RC.build(RC.BY_NAME[name], delta_scale=1.5)


def test_midpoint_detector():
    x = np.float32(0.3)
    up = np.nextafter(x, np.float32(1))
    mid = (float(x) + float(up)) / 2
    assert RC.near_f32_midpoint(np.array([mid, -mid, mid + 5e-13]))[:3].all()
    assert not RC.near_f32_midpoint(np.array([float(x), float(up), mid + 1e-10, 0.0, 0.25])).any()
