"""Host tests of the J&F counts path (fgvc_jf_counts_u8, metrics' backend='hip', test_cfg.masks): the symbol and its
argument validation, the counts formulation against the host scorer (==) and against the reference's golden values, the keywords'
refusals, and that the shared cases reach every branch of the boundary measure.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import jf_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(JC.cases())


def test_symbol_is_declared_exported_and_validates():
    from fgvc_amd import _lib, build, ops
    assert "jf.hip" in build.SOURCES and "fgvc_jf_counts_u8" in _lib.SIGNATURES
    with open(os.path.join(ROOT, "include", "fgvc_hip.h")) as f:
        assert "int fgvc_jf_counts_u8(const uint8_t* gt, const uint8_t* pred, int T, int h, int w, int n_objects, int radius" in f.read()
    lib = _lib.load()
    assert lib.fgvc_jf_tile_rows() == ops.JF_TILE == JC.JF_TILE
    a, b, out = (C.create_string_buffer(64), C.create_string_buffer(64), C.create_string_buffer(6 * 8 * 4))       # never reached
    pa, pb, po = (C.cast(x, C.c_void_p) for x in (a, b, out))

    def call(gt=pa, pred=pb, T=1, h=4, w=4, n=1, r=2, counts=po):
        return lib.fgvc_jf_counts_u8(gt, pred, T, h, w, n, r, counts, None)
    for kw in (dict(gt=None), dict(pred=None), dict(counts=None)):
        assert call(**kw) == _lib.ERR_INVALID_ARG and b"null" in lib.fgvc_last_error()
    assert call(r=0) == _lib.ERR_INVALID_ARG and b"radius" in lib.fgvc_last_error()
    assert call(r=65) == _lib.ERR_UNSUPPORTED and b"radius" in lib.fgvc_last_error()
    assert call(n=256) == _lib.ERR_INVALID_ARG and b"n_objects" in lib.fgvc_last_error()
    assert call(n=-1) == _lib.ERR_INVALID_ARG
    for kw in (dict(T=-1), dict(h=-1), dict(w=-1)):
        assert call(**kw) == _lib.ERR_INVALID_ARG and b"negative" in lib.fgvc_last_error()
    assert call(h=1 << 16, w=1 << 15) == _lib.ERR_INVALID_ARG
    assert call(T=0) == _lib.FGVC_OK and call(n=0) == _lib.FGVC_OK                       # nothing to write, nothing launched


def test_wrapper_refusals_without_a_gpu():
    from fgvc_amd import _lib, ops
    m = torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.jf_counts(m, m, 1, 2)


def test_radius_rule():
    from fgvc_amd import metrics
    assert metrics.jf_radius((480, 854)) == 8 and metrics.jf_radius((2160, 3840)) == 36
    assert metrics.jf_radius((5, 6), 8) == 8 and metrics.jf_radius((40, 40), 1) == 1
    assert isinstance(metrics.jf_radius((60, 84)), int)


@pytest.mark.parametrize("name", NAMES)
def test_counts_give_the_host_scores_bit_for_bit(name):
    from fgvc_amd import metrics
    gt, pred, n, r = JC.cases()[name]
    J, F = metrics.jf_from_counts(JC.expected(name))
    Jh, Fh = JC.jf_host(gt, pred, n, r)
    assert J.dtype == F.dtype == np.float64 and J.shape == F.shape == (gt.shape[0], n)
    assert np.array_equal(J, Jh) and np.array_equal(F, Fh)
    if name.startswith("disk_edge"):
        assert tuple(F[:, 0]) == JC.DISK_EDGE_F


def test_known_boundaries():
    """metrics._seg2bmap's consequences, through the counts: a frame-filling object has no boundary, one pixel gives a 2 x 2 block, a
    1 x N image marks x0 - 1 and x1, a 1 x 1 image nothing."""
    c = JC.expected("borders_and_empties_4x24x40")
    assert tuple(c[0, 0]) == (24 * 40, 24 * 40, 0, 0, 0, 0)
    assert tuple(JC.expected("disk_edge_4x40x40")[0, 0, 2:4]) == (4, 4)
    assert tuple(JC.expected("one_row_1x1x130")[0, 0, 2:4]) == (2, 2)          # pred 12..63 -> 11 and 63; gt 10..64 -> 9 and 64
    assert tuple(JC.expected("one_row_1x1x130")[0, 1, 2:4]) == (2, 1)          # gt 100..129 reaches the row's end: 99 only
    assert tuple(JC.expected("one_pixel_1x1x1")[0, 0]) == (1, 1, 0, 0, 0, 0)


def test_cases_reach_every_branch():
    """The equalities above and on the GPU cannot pass by avoiding the hard branches."""
    seen = set()
    for name in NAMES:
        for inter, union, n_fg, n_gt, hit_fg, hit_gt in JC.expected(name).reshape(-1, 6):
            seen.add("both empty" if n_fg == 0 and n_gt == 0 else "no fg" if n_fg == 0 else "no gt" if n_gt == 0 else "both")
            if n_fg and n_gt:
                if hit_fg == 0 and hit_gt == 0:
                    seen.add("p + r == 0")
                if 0 < hit_fg < n_fg:
                    seen.add("partial precision")
                if 0 < hit_gt < n_gt:
                    seen.add("partial recall")
            if union == 0:
                seen.add("empty union")
            if 0 < inter < union:
                seen.add("partial J")
    assert seen == {"both empty", "no fg", "no gt", "both", "p + r == 0", "partial precision", "partial recall", "empty union", "partial J"}


def test_counts_route_reproduces_the_reference_golden():
    """tests/golden/vos_jf.npz (the reference's db_eval_iou / db_eval_boundary / JFM) through counts_host -> jf_from_counts."""
    from fgvc_amd import metrics
    g = np.load(os.path.join(ROOT, "tests", "golden", "vos_jf.npz"))
    gt, pr = g["gt"], g["pred"]
    r = metrics.jf_radius(gt.shape[-2:])
    stats = {k: [] for k in ("JM", "JR", "JD", "FM", "FR", "FD")}
    for o in range(gt.shape[0]):
        J, F = metrics.jf_from_counts(JC.counts_host(gt[o].astype(np.uint8), pr[o].astype(np.uint8), 1, r))
        np.testing.assert_allclose(J[:, 0], g[f"iou_{o}"], rtol=0, atol=1e-12)
        np.testing.assert_allclose(F[:, 0], g[f"f_{o}"], rtol=0, atol=1e-12)
        for key, vals in (("J", J[:, 0]), ("F", F[:, 0])):
            for s, v in zip("MRD", metrics.db_statistics(vals)):
                stats[key + s].append(v)
    for k, v in stats.items():
        np.testing.assert_allclose(np.asarray(v), g["JFM_" + k], rtol=0, atol=1e-12)


def test_backend_keyword(monkeypatch):
    from fgvc_amd import metrics
    s = JC.davis_sequences()
    assert metrics.davis_jf(s) == metrics.davis_jf(s, backend="host")
    gt, pred = s["six"]
    G, S = metrics.davis_masks_to_objects(gt, 3), metrics.davis_masks_to_objects(pred, 3)
    assert metrics.JFM(G, S) == metrics.JFM(G, S, backend="host")
    assert np.array_equal(metrics.db_eval_boundary(G[0], S[0]), metrics.db_eval_boundary(G[0], S[0], backend="host"))
    for call in (lambda b: metrics.davis_jf(s, backend=b), lambda b: metrics.JFM(G, S, backend=b),
                 lambda b: metrics.db_eval_boundary(G[0], S[0], backend=b)):
        with pytest.raises(ValueError, match="backend"):
            call("cuda")
    with pytest.raises(NotImplementedError, match="void_pixels"):
        metrics.db_eval_boundary(G[0], S[0], void_pixels=np.zeros_like(G[0]), backend="hip")
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)                     # (this test is the same on a GPU box)
    for call in (lambda: metrics.davis_jf(s, backend="hip"), lambda: metrics.JFM(G, S, backend="hip"),
                 lambda: metrics.db_eval_boundary(G[0], S[0], backend="hip")):
        with pytest.raises(RuntimeError, match="GPU"):
            call()
    from fgvc_amd.datasets import davis_evaluate
    with pytest.raises(RuntimeError, match="GPU"):
        davis_evaluate(None, [], backend="hip")
    with pytest.raises(ValueError, match="backend"):
        davis_evaluate(None, [], backend="device")


@pytest.mark.parametrize("typ", ["VanillaTracker", "HRVanillaTracker"])
def test_masks_key_is_parsed_at_construction(typ):
    import fgvc_amd.mmpt_api as api
    from fgvc_amd import engine
    bb = dict(type="ResNet", depth=18, strides=(1, 1, 1, 4), out_indices=(2,), pool_type="none")
    assert api.build_model(dict(type=typ, backbone=bb), test_cfg=dict()).masks_form == "numpy"
    assert api.build_model(dict(type=typ, backbone=bb), test_cfg=dict(masks="numpy")).masks_form == "numpy"
    assert api.build_model(dict(type=typ, backbone=bb), test_cfg=dict(masks="device")).masks_form == "device"
    with pytest.raises(ValueError, match="masks"):
        api.build_model(dict(type=typ, backbone=bb), test_cfg=dict(masks="cuda"))
    assert engine.parse_masks(None) == "numpy"
