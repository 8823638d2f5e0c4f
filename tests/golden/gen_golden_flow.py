"""Record the fixtures of the dense-flow operators (fgvc_amd/csrc/flow.hip) from the reference, executed read-only in place.

    python tests/golden/gen_golden_flow.py          # writes tests/golden/flow_*.npz

The reference's `coords_grid_warp` and `Warp` (mmpt/models/common/warp.py) and every function of occlusion_estimation.py are lifted out of
their modules by AST at generation time, the registry decorator of `Warp` dropped (the package itself needs mmcv, absent here), and run
unchanged on float32 CPU tensors.  Only data is stored: the input flows and feature maps, the reference's masks and warped maps, and the
share of each mask that the float64 restatement (tests/flow_cases.py) calls undecided.

Flows: bicubic upsampling of a coarse normal field (amplitude 3 to 6 px).  flow_bw is the inverse of flow_fw (a fixed-point iteration, so
that the pair is consistent to a few hundredths of a pixel), plus a smooth perturbation of a fraction of a pixel -- what makes every mask
mixed -- plus one rectangular block of gross inconsistency.  The generator asserts: every mask's mean lies in [0.2, 0.8]; the reference's
float32 masks equal the float64 restatement on every decided pixel; at most 1 % of a mask is undecided; the restated warp is within 1e-5
of the reference's.
"""
from __future__ import annotations

import ast
import os
import sys
import warnings
from typing import Dict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from oracle.ref_import import REF_ROOT  # noqa: E402
import flow_cases as FC  # noqa: E402

WARP = "mmpt/models/common/warp.py"
OCC = "mmpt/models/common/occlusion_estimation.py"
FLOWS = (("flow_2x37x53", 2, 37, 53, 3.0, 11), ("flow_2x64x96", 2, 64, 96, 6.0, 12))         # name, N, H, W, amplitude, seed
WARPS = ("flow_warp_2x3x37x53", 2, 3, 37, 53, 21)
MODES = (("consistency", {}), ("fb_abs", dict(diff=1.5)))
PERTURB = 0.7                                                                                  # px, per component


def lift():
    ns = {"torch": torch, "nn": nn, "F": F, "Tensor": torch.Tensor, "Dict": Dict}
    for rel in (WARP, OCC):
        body = []
        for n in ast.parse(open(os.path.join(REF_ROOT, rel)).read()).body:
            if isinstance(n, ast.ClassDef):
                n.decorator_list = []                                                          # @OPERATORS.register_module()
            if isinstance(n, (ast.ClassDef, ast.FunctionDef)):
                body.append(n)
        mod = ast.Module(body, [])
        ast.fix_missing_locations(mod)
        exec(compile(mod, "ref:" + rel, "exec"), ns)
    for name in ("coords_grid_warp", "Warp", "occlusion_estimation", "forward_backward_consistency", "forward_backward_absdiff", "flow_to_coords"):
        assert name in ns, name
    return ns


def smooth(N, C, H, W, amp, seed, coarse=(4, 6)):
    g = torch.Generator().manual_seed(seed)
    return F.interpolate(torch.randn(N, C, *coarse, generator=g) * amp, size=(H, W), mode="bicubic", align_corners=True).contiguous()


def sample_at(field, disp):
    """field(p + disp) at every pixel p, bilinear with the border clamped (the generator's own construction, not an operator under test)."""
    N, _, H, W = field.shape
    ys, xs = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    gx = (xs + disp[:, 0]) * 2 / max(W - 1, 1) - 1
    gy = (ys + disp[:, 1]) * 2 / max(H - 1, 1) - 1
    return F.grid_sample(field, torch.stack([gx, gy], -1), mode="bilinear", padding_mode="border", align_corners=True)


def flows(N, H, W, amp, seed):
    fw = smooth(N, 2, H, W, amp, seed)
    bw = -fw
    for _ in range(8):                                                                         # bw(y) = -fw(y + bw(y))
        bw = -sample_at(fw, bw)
    bw = bw + smooth(N, 2, H, W, PERTURB, seed + 100, coarse=(5, 7))
    y0, x0 = H // 5, W // 2
    bw[:, :, y0:y0 + H // 4, x0:x0 + W // 4] += 9.0                                            # gross inconsistency
    return fw.contiguous(), bw.contiguous()


def main():
    warnings.simplefilter("ignore")
    torch.set_num_threads(1)
    ns = lift()
    for name, N, H, W, amp, seed in FLOWS:
        fw, bw = flows(N, H, W, amp, seed)
        out = dict(flow_fw=fw.numpy(), flow_bw=bw.numpy())
        for mode, kw in MODES:
            ref = ns["occlusion_estimation"](fw, bw, mode, **kw)
            want = FC.consistency_both_ref(fw.numpy(), bw.numpy(), mode, kw.get("diff", 1.5))
            for key, occ64, decided in (("occ_fw", want[0], want[2]), ("occ_bw", want[1], want[3])):
                occ = ref[key].numpy()
                assert occ.dtype == np.float32 and occ.shape == (N, 1, H, W) and set(np.unique(occ)) <= {0.0, 1.0}
                mean, undecided = float(occ.mean()), float(1.0 - decided.mean())
                wrong = int(((occ != occ64) & decided).sum())
                print(f"{name} {mode} {key}: mean {mean:.3f}, undecided share {undecided:.2e}, {wrong} decided pixels differ from float64")
                assert 0.2 <= mean <= 0.8, (name, mode, key, mean)
                assert wrong == 0 and undecided <= 0.01
                out[f"{mode}_{key}"] = occ.astype(np.uint8)
                out[f"{mode}_{key}_undecided"] = np.float64(undecided)
        out["diff"] = np.float64(1.5)
        path = os.path.join(HERE, name + ".npz")
        np.savez_compressed(path, **out)
        print(name, os.path.getsize(path), "bytes")
    name, N, C, H, W, seed = WARPS
    feat = smooth(N, C, H, W, 1.0, seed, coarse=(6, 8))
    flow = smooth(N, 2, H, W, 4.0, seed + 1)
    out = dict(feat=feat.numpy(), flow=flow.numpy())
    for ac in (False, True):
        for um in (False, True):
            got = ns["Warp"](align_corners=ac, use_mask=um)(feat, flow).numpy()
            want, ones, _ = FC.warp_ref(feat.numpy(), flow.numpy(), ac, um)
            decided = np.broadcast_to((np.abs(ones - 0.9999) >= FC.MASK_MARGIN)[:, None], got.shape) if um else np.ones(got.shape, bool)
            undecided = float(1.0 - decided.mean())
            err = float(np.abs(got - want)[decided].max())
            print(f"{name} align_corners={ac} use_mask={um}: max |reference - float64| = {err:.2e}, undecided share {undecided:.2e}, "
                  f"{float((got != 0).mean()):.3f} of the output non-zero")
            assert err <= 1e-5 and undecided <= 0.01
            out[f"out_ac{int(ac)}_m{int(um)}"] = got
            out[f"undecided_ac{int(ac)}_m{int(um)}"] = np.float64(undecided)
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **out)
    print(name, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
