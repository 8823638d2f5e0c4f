"""CPU: what tests/test_gpu_post_ops.py relies on, checked with the reference alone.

* On every read-out case the GPU module uses, at least 95 % of the maps are held to the coordinate check (clear gap, structural tie
  or zero map: tests/post_cases.py), and on those maps the float64 restatement agrees with the reference's own f32 pipeline
  (O.upsample_bilinear + O.img2coord) within the read-out tolerance.  That is what ties the tolerance to the reference.
* The exact-arithmetic cases are exact: the f32 field equals the float64 field bit for bit.
* The merge, propagate and Gaussian restatements reproduce O.topk_canonical, O.propagate_topk (and F.unfold's window) and
  O.gaussian_labels.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fgvc_oracle as O
from tests import post_cases as PC


def _oracle_coords(maps32):
    """O.img2coord of (T, P, h, w) f32 maps -> (T, P, 2)"""
    return np.transpose(O.img2coord(maps32.numpy()), (2, 1, 0))


@pytest.mark.parametrize("case", PC.READOUT, ids=PC.case_id)
def test_readout_share_and_oracle(case):
    name, T, Hf, Wf, P, h, w = case
    labels = PC.readout_labels(case)
    want = PC.readout_want(case, labels)
    share = float(want["checkable"].float().mean())
    plain = float(((want["gap"] > PC.CLEAR) | want["zero"]).float().mean())
    ref = _oracle_coords(PC.field(labels, Hf, Wf, h, w, torch.float32))
    ck = want["checkable"].numpy()
    err = np.abs(ref - want["coords"]).max(-1)
    tol = PC.readout_tol(h, w)
    print(f"read-out {name}: checkable share {share:.4f} (without the structural rule {plain:.4f}), reference f32 vs float64 restatement "
          f"{float(err[ck].max()):.3e} px (tol {tol:.3e})")
    assert share >= PC.MIN_SHARE, share
    assert plain <= share
    assert float(err[ck].max()) <= tol
    if name.startswith("special"):
        assert bool(want["zero"][:, 8].all()) and not bool(want["zero"][:, 9].any())
        assert np.array_equal(ref[:, 8], np.full((T, 2), -1.0))
        if name == "special_x4":        # the border bumps are what the structural rule is for
            assert bool(want["structural"][:, :8].any()) and plain < share


@pytest.mark.parametrize("name", ["base", "odd"])
def test_first_frame_share_and_oracle(name):
    case = next(c for c in PC.READOUT if c[0] == name)
    _, T, Hf, Wf, P, h, w = case
    pts, exact, far = PC.readout_points(h, w)
    want = PC.first_frame_want(pts, exact, h, w)
    share = float(want["checkable"].float().mean())
    ref = _oracle_coords(O.gaussian_labels(pts, h, w, 1)[0][None])
    err = np.abs(ref - want["coords"]).max(-1)
    ck = want["checkable"].numpy()
    print(f"first frame {name}: checkable share {share:.4f}, reference f32 vs float64 restatement {float(err[ck].max()):.3e} px")
    assert share >= PC.MIN_SHARE, share
    assert float(err[ck].max()) <= PC.readout_tol(h, w)
    assert bool((want["zero"][0] == far).all())
    assert bool(want["structural"][0].any())                # the half-integer centres tie exactly at rank 5


@pytest.mark.parametrize("case", PC.EXACT, ids=PC.case_id)
def test_exact_cases_are_exact(case):
    name, Hf, Wf, scale = case
    lab = PC.exact_labels(case)
    f32 = PC.field(lab, Hf, Wf, Hf * scale, Wf * scale, torch.float32)
    f64 = PC.field(lab, Hf, Wf, Hf * scale, Wf * scale)
    assert torch.equal(f32.double(), f64)


@pytest.mark.parametrize("topk", [1, 3, 5, 7, 12, 16])
def test_merge_restatement_is_topk_canonical(topk):
    T, HWq, HWk = 7, 33, PC.MERGE_HWK
    pi, ps = PC.merge_lists(T + 1, HWq, HWk, topk, seed=topk)
    sp = PC.merge_slot_pairs(3, T, T + 1, seed=topk)
    want = PC.merge_restated(pi, ps, sp, HWk, topk)
    for f in range(3):
        val, idx = O.topk_canonical(PC.merge_dense(pi, ps, sp[f], HWk), topk)                # (k, HWq)
        have = (val > O.NEG_INF).t()
        assert torch.equal(have, want["valid"][f])
        assert torch.equal(idx.t()[have], want["idx"][f][have])
        assert torch.equal((val / PC.TEMP).t()[have], want["logit"][f][have])
        full = have.all(1)
        assert torch.allclose(O.topk_weights((val / PC.TEMP).t()[full]), want["softmax"][f][full], atol=1e-14)
    assert bool((want["idx"][1][:, :1] < HWk).all()) or topk == 0         # row 1: one pair in every slot, the lowest slot's gid leads
    assert not bool(want["valid"][2].all())                              # row 2 has short rows


@pytest.mark.parametrize("window_L", [0, 3, 9])
def test_propagate_restatement_is_oracle(window_L):
    Hq, Wq, P, topk = 5, 33, 3, 5
    slots = PC.PROP_SLOTS[0]
    labels, idx, weight = PC.propagate_inputs(P, topk, Hq, Wq, Hq, Wq, slots, window_L, seed=1, empty=0.0)
    got, _ = PC.propagate_restated(labels, slots, idx, weight, Hq, Wq, Hq, Wq, window_L)
    value = labels.double()[slots]                                                          # (T, HW, P)
    if window_L == 0:
        want = O.propagate_topk(value.permute(2, 0, 1).reshape(P, -1), idx.long(), weight.double()).t()
    else:   # O.local_corr_topk's gather (vanilla_tracker.py:550-566)
        T, LL = len(slots), window_L * window_L
        unf = F.unfold(value.permute(0, 2, 1).reshape(T, P, Hq, Wq), kernel_size=window_L, padding=window_L // 2)
        unf = unf.reshape(T, P, LL, Hq * Wq).permute(1, 0, 2, 3).reshape(P, T * LL, Hq * Wq)
        g = unf.gather(1, idx.long().t().unsqueeze(0).expand(P, -1, -1))
        want = (g * weight.double().t().unsqueeze(0)).sum(1).t()
    assert torch.allclose(got, want, atol=1e-12), float((got - want).abs().max())


@pytest.mark.parametrize("case", PC.GAUSS, ids=PC.case_id)
def test_gauss_restatement_is_oracle(case):
    Hf, Wf, stride, P, sigma = case
    pts = PC.gauss_points(case)
    want, arg = PC.gauss_frame(pts, Hf, Wf, sigma, stride)
    ref = O.gaussian_labels(pts, (Hf - 1) * stride + 1, (Wf - 1) * stride + 1, stride, sigma)[1].double()
    bound = (4 + 4 * arg) * 2.0 ** -24 * want + PC.F32_MIN_NORMAL
    assert ref.shape == want.shape and bool(((ref - want).abs() <= bound).all())
    small = want[want > 0].min()
    print(f"gauss {case}: smallest positive label {float(small):.3e}, zeros {int((want.float() == 0).sum())}")
    if P >= 4:
        assert float(small) < PC.F32_MIN_NORMAL and bool((want.float() == 0).any())        # the case reaches subnormals and 0
