"""CPU: what tests/test_gpu_window_ops.py relies on, checked with the reference alone.

* O.check_topk's `structural` argument: unchanged without it, strict with it.
* On every shape the GPU module uses, at least 95 % of the queries are held to the exact canonical list (the cap of that module:
  it may leave out at most 5 % of a case's queries).
* The test-side restatement of the c2f fine stage (tests/window_cases.py) reproduces the oracle's c2f_attention.
"""
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import window_cases as WC


def test_check_topk_structural_rule():
    # 4 candidates, 3 queries; candidates 1 and 2 are structural zeros
    dense = torch.tensor([[0.5, 0.5, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [-0.3, 0.0, -0.3]], dtype=torch.float64)
    st = torch.tensor([[False] * 3, [True] * 3, [True] * 3, [False] * 3])
    good = torch.tensor([[0, 1, 2]] * 3)
    score = torch.tensor([[0.5, 0.0, 0.0]] * 3)
    plain = O.check_topk(dense, good, score, 3)
    assert plain["clear"] == 0 and "checkable" not in plain                      # the default rule exempts every tie
    strict = O.check_topk(dense, good, score, 3, structural=st)
    assert strict["checkable"] == 2 and strict["checkable_mask"].tolist() == [True, False, True]    # query 1: a tie with a real candidate
    swapped = torch.tensor([[0, 2, 1], [0, 1, 2], [0, 1, 2]])
    O.check_topk(dense, swapped, score, 3)                                        # passes the default rule ...
    with pytest.raises(AssertionError):
        O.check_topk(dense, swapped, score, 3, structural=st)                     # ... and not the strict one
    cls = torch.tensor([[0] * 3, [5] * 3, [6] * 3, [0] * 3])                      # different classes do not tie by construction
    assert O.check_topk(dense, good, score, 3, structural=cls)["checkable"] == 0


@pytest.mark.parametrize("shape", WC.LOCAL_F32, ids=WC.case_id)
def test_local_share(shape):
    C, K, H, W, R, topk = shape
    q, keys, _ = WC.local_inputs(shape)
    dense, cls = WC.local_slab(q, keys, R)
    s = WC.share(dense, topk, cls)
    print(f"local {shape}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s
    if R >= 1:   # the border is where the structural rule matters: without it fewer queries (or none) are checkable
        assert WC.share(dense, topk, None) <= s


@pytest.mark.parametrize("shape", WC.LOCAL_ZERO_ROWS, ids=WC.case_id)
def test_local_zero_rows_share(shape):
    C, K, H, W, R, topk = shape
    q, keys, _ = WC.local_inputs(shape, zero_rows=True)
    dense, cls = WC.local_slab(q, keys, R)
    s = WC.share(dense, topk, cls)
    print(f"local zero rows {shape}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s
    # the case is what it is meant to be: nothing scores above 0, the canonical list is the padded taps 0..k-1 of slot 0, and slot 0
    # holds at least k in-image taps that score exactly 0 too (they fill the list before the padded taps arrive)
    val, idx = O.topk_canonical(dense, topk)
    assert float(dense.max()) == 0.0 and bool((idx.t() == torch.arange(topk)).all())
    LL = (2 * R + 1) ** 2
    inside_zero = ((dense[:LL] == 0) & ~WC.window_outside(H, W, R)).sum(0)
    assert int((inside_zero >= topk).sum()) >= 0.9 * H * W


@pytest.mark.parametrize("shape", WC.LOCAL_TIES, ids=WC.case_id)
def test_local_ties_share(shape):
    C, K, H, W, R, topk = shape
    q, keys, _ = WC.local_inputs(shape, twin=True)
    dense, cls = WC.local_slab(q, keys, R, frames=[0] * K)
    assert WC.share(dense, topk, None) == 0.0                                      # every score appears twice
    s = WC.share(dense, topk, cls)
    print(f"local ties {shape}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s


@pytest.mark.parametrize("topk", WC.PLAN_TOPK)
def test_plan_share(topk):
    C, K, H, W, R = WC.PLAN_SHAPE
    q, keys, _ = WC.local_inputs((C, K, H, W, R, topk))
    for row in WC.PLAN_ROWS:
        dense, cls = WC.local_slab(q, keys, R, frames=WC.plan_frames(row, K))
        s = WC.share(dense, topk, cls)
        print(f"plan row {row} topk {topk}: checkable share {s:.4f}")
        assert s >= WC.MIN_SHARE, (row, s)


@pytest.mark.parametrize("case", WC.COORD, ids=WC.case_id)
def test_coord_share(case):
    C, H, W, R, topk, scale = case
    q, keys, _ = WC.local_inputs((C, 1, H, W, R, topk))
    dense, cls = WC.local_slab(q, keys, R)
    s = WC.share(dense, min(topk, dense.shape[0]), cls)
    print(f"coord {case}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s
    # coord_of_lists on the oracle's own lists is get_coord
    val, idx = O.topk_canonical(dense, topk)
    got = WC.coord_of_lists(idx.t(), val.softmax(0).t(), H, W, R, scale)
    want = O.get_coord(q.double(), keys[0].double(), R, topk, WC.TEMP, scale).reshape(2, H * W).t()
    assert torch.allclose(got, want, atol=1e-9), float((got - want).abs().max())


@pytest.mark.parametrize("shape", WC.C2F_SWEEP, ids=WC.case_id)
def test_c2f_share_and_restatement(shape):
    Cf, T, H, W, scale, Rf, topk = shape
    c = WC.c2f_case(shape)
    s = WC.share(c["dense"], topk, c["cls"])
    print(f"c2f {shape}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s
    for mode in ("softmax", "cosine"):
        o_out, o_arg, o_idx, o_logit = O.c2f_attention(c["q"].double(), c["key"].double(), c["qfine"].double(), c["kfine"].double(),
                                                       c["v"].double(), topk, WC.TEMP, normalize=False, radius_fine=Rf, mode=mode)
        out, idx, logit = WC.c2f_out(c["dense"], c["pix"], c["v"], topk, mode)
        assert torch.equal(o_arg, c["arg"])
        assert torch.allclose(logit, o_logit, atol=1e-9)
        m = O.checkable_queries(c["dense"], topk, WC.GAP, c["cls"])
        assert torch.equal(idx[m], o_idx[m])
        assert torch.allclose(out[:, m], o_out.reshape(out.shape[0], -1)[:, m], atol=1e-9)


@pytest.mark.parametrize("name", list(WC.C2F_EXTRA))
def test_c2f_extra_share(name):
    shape, P, forced = WC.C2F_EXTRA[name]
    c = WC.c2f_case(shape, P=P, forced=forced)
    s = WC.share(c["dense"], shape[-1], c["cls"])
    print(f"c2f {name} {shape}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s
    if forced:   # most of the fine window of most queries lies outside the map
        assert float((c["cls"] == 1).float().mean()) > 0.5


@pytest.mark.parametrize("name", list(WC.C2F_TIES))
def test_c2f_ties_share(name):
    shape = WC.C2F_TIES[name]
    c = WC.c2f_case(shape, twin=True)
    assert WC.share(c["dense"], shape[-1], None) == 0.0
    s = WC.share(c["dense"], shape[-1], c["cls"])
    print(f"c2f ties {name} {shape}: checkable share {s:.4f}")
    assert s >= WC.MIN_SHARE, s
