"""Record the fixtures of the flow-chaining point tracker (fgvc_amd/csrc/chain.hip) from the reference, executed read-only
in place.

    python tests/golden/gen_golden_chain.py          # writes tests/golden/chain_*.npz

`RAFT.forward_test` (mmpt/models/trackers/raft.py:222-289) and `bilinear_sample2d` (mmpt/datasets/flyingthingsplus/utils/samp.py:5-99) are
lifted out of their modules by AST at generation time and run unchanged on float32 CPU tensors; `forward_test_pair`, the only thing the
method asks of its network, is a stub that hands out prepared flows (every frame of `rgbs` holds its own number, which tells the stub the
pair).  Only data is stored: the flows, the queries, and the reference's `trajectories_pred` and `visibilities_pred`.

Flows: bicubic upsampling of a coarse normal field, as gen_golden_flow.py's `smooth`.  Queries: random times and positions, plus planted
ones -- t = 0 and t = T-1, integer positions, x = w-1, and points that start outside the frame on each side.  The generator asserts that
engine.chain_points_host and the loop restatement of tests/chain_cases.py both equal the reference on every entry, bit for bit, and that
each fixture's visible share lies in [0.2, 0.9].
"""
from __future__ import annotations

import ast
import os
import sys
import types
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from oracle.ref_import import REF_ROOT  # noqa: E402
from tests import chain_cases as CC  # noqa: E402
from fgvc_amd import engine  # noqa: E402

RAFT = "mmpt/models/trackers/raft.py"
SAMP = "mmpt/datasets/flyingthingsplus/utils/samp.py"
# name, T, h, w, amplitude (px), P, seed, margin of the random positions outside the frame (px)
CASES = (("chain_6x37x53", 6, 37, 53, 4.0, 64, 41, 3.0), ("chain_3x2x70", 3, 2, 70, 5.0, 65, 42, 0.3),
         ("chain_2x1x1", 2, 1, 1, 0.4, 4, 43, 0.0), ("chain_24x24x32", 24, 24, 32, 2.0, 48, 44, 2.0))


def lift():
    """-> (RAFT.forward_test as a plain function of (self, rgbs, ...), bilinear_sample2d)."""
    ns = {"torch": torch, "F": F}
    tree = ast.parse(open(os.path.join(REF_ROOT, SAMP)).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "bilinear_sample2d"]
    assert len(fn) == 1
    mod = ast.Module(fn, [])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "ref:" + SAMP, "exec"), ns)
    ns["samp"] = types.SimpleNamespace(bilinear_sample2d=ns["bilinear_sample2d"])
    tree = ast.parse(open(os.path.join(REF_ROOT, RAFT)).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "RAFT"]
    assert len(cls) == 1
    fn = [n for n in cls[0].body if isinstance(n, ast.FunctionDef) and n.name == "forward_test"]
    assert len(fn) == 1
    mod = ast.Module(fn, [])
    ast.fix_missing_locations(mod)
    exec(compile(mod, "ref:" + RAFT, "exec"), ns)
    return ns["forward_test"], ns["bilinear_sample2d"]


def smooth(N, C, H, W, amp, seed, coarse=(4, 6)):
    g = torch.Generator().manual_seed(seed)
    return F.interpolate(torch.randn(N, C, *coarse, generator=g) * amp, size=(H, W), mode="bicubic", align_corners=True).contiguous()


class Stub:
    """What RAFT.forward_test reads of `self`: forward_test_pair(imgs)[0][-1] = the pair's flow (1, 2, h, w)."""

    def __init__(self, fw, bw):
        self.fw, self.bw = fw, bw

    def forward_test_pair(self, imgs):
        a, b = int(imgs[0, 0, 0, 0, 0, 0]), int(imgs[0, 0, 0, 1, 0, 0])          # (B, 1, C, 2, H, W): the two frames' numbers
        assert abs(a - b) == 1
        return ([self.fw[a][None] if b == a + 1 else self.bw[b][None]],)


def make_queries(T, h, w, P, seed, margin):
    q = CC.queries(P, T, h, w, seed, margin)
    planted = [(0, w * 0.5, h * 0.5), (T - 1, w * 0.25, h * 0.5), (T // 2, w // 2, h // 2), (0, 0, 0), (T - 1, w - 1, h - 1),
               (T // 2, w - 1, h * 0.5), (1, -1.5, h * 0.5), (0, w + 0.75, h * 0.5), (T - 1, w * 0.5, -2.25), (1, w * 0.5, h + 1.5)]
    k = min(len(planted), P) if P >= 16 else 0
    q[:k] = np.asarray(planted[:k], np.float32)
    return q


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    forward_test, _ = lift()
    for name, T, h, w, amp, P, seed, margin in CASES:
        fw, bw = smooth(T - 1, 2, h, w, amp, seed), smooth(T - 1, 2, h, w, amp, seed + 100)
        if name == "chain_2x1x1":
            q = np.asarray([(0, 0.5, 0.5), (1, 0.25, 0.75), (0, -1.0, 0.5), (1, 0.5, 2.0)], np.float32)
        else:
            q = make_queries(T, h, w, P, seed + 200, margin)
        rgbs = torch.arange(T, dtype=torch.float32).view(1, T, 1, 1, 1).expand(1, T, 3, h, w)
        ref = forward_test(Stub(fw, bw), rgbs, torch.from_numpy(q)[None], None, None)
        traj, vis = ref[2][0].numpy(), ref[3][0].numpy()
        assert traj.dtype == np.float32 and traj.shape == (T, P, 2) and vis.dtype == np.bool_ and vis.shape == (T, P)
        for what, (t2, v2) in (("engine.chain_points_host", engine.chain_points_host(fw.numpy(), bw.numpy(), q)),
                               ("chain_cases.chain_ref", CC.chain_ref(fw.numpy(), bw.numpy(), q))):
            assert np.array_equal(t2, traj) and np.array_equal(CC.bits(t2), CC.bits(traj)), (name, what)
            assert np.array_equal(v2, vis.astype(np.uint8)), (name, what)
        share = float(vis.mean())
        moved = float(np.abs(traj - q[None, :, 1:]).max())
        print(f"{name}: P = {P}, visible share {share:.3f}, largest displacement from the query {moved:.2f} px; host and loop restatement equal "
              "the reference bit for bit")
        assert 0.2 <= share <= 0.9, (name, share)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, flow_fw=fw.numpy(), flow_bw=bw.numpy(), query=q, traj=traj, vis=vis.astype(np.uint8))
        print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
