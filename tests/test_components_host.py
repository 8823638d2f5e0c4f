"""CPU tests of connected components of id maps: metrics.components_host against scipy.ndimage.label on every case
of tests/components_cases.py, metrics.clean_masks_host against maps and statistics written out by hand, deliberately wrong restatements
that the case set has to tell from the contract, engine.parse_clean, and the C surface.  Every comparison is `==`."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import components_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location("fgvc_" + name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- the contract against an independent implementation -------------------------------------------------------------------------------------
def _scipy_components(ids, connectivity, background):
    """scipy.ndimage.label per frame and id with the 4- / 8-structure (id 0: always 4), every label mapped to its component's minimum index"""
    ndimage = pytest.importorskip("scipy.ndimage")
    four, eight = ndimage.generate_binary_structure(2, 1), ndimage.generate_binary_structure(2, 2)
    T, h, w = ids.shape
    out = np.full((T, h, w), -1, np.int32)
    index = np.arange(h * w, dtype=np.int64).reshape(h, w)
    for t in range(T):
        for o in np.unique(ids[t]).tolist():
            if o == 0 and not background:
                continue
            lab, n = ndimage.label(ids[t] == o, structure=four if o == 0 or connectivity == 4 else eight)
            if n:
                roots = ndimage.minimum(index, lab, np.arange(1, n + 1))
                sel = lab > 0
                out[t][sel] = np.asarray(roots, np.int64)[lab[sel] - 1]
    return out


@pytest.mark.parametrize("name", list(CC.cases()))
def test_components_host_equals_scipy_on_the_named_cases(name):
    pytest.importorskip("scipy.ndimage")
    for conn, bg in CC.VARIANTS:
        got = CC.expected(name, conn, bg)
        assert got.dtype == np.int32 and got.shape == CC.cases()[name].shape
        assert np.array_equal(got, _scipy_components(CC.cases()[name], conn, bg)), (name, conn, bg)


@pytest.mark.parametrize("h", CC.HEIGHTS)
@pytest.mark.parametrize("w", CC.WIDTHS)
def test_components_host_equals_scipy_at_every_size(w, h):
    pytest.importorskip("scipy.ndimage")
    for conn, bg in CC.VARIANTS:
        assert np.array_equal(CC.expected_sized(w, h, conn, bg), _scipy_components(CC.sized(w, h), conn, bg)), (w, h, conn, bg)


def test_components_host_by_hand():
    from fgvc_amd import metrics
    m = CC.art("1.1",
               ".1.",
               "2.2")[None]
    assert metrics.components_host(m, 8)[0].tolist() == [[0, -1, 0], [-1, 0, -1], [6, -1, 8]]
    assert metrics.components_host(m, 4)[0].tolist() == [[0, -1, 2], [-1, 4, -1], [6, -1, 8]]
    assert metrics.components_host(m, 8, background=True)[0].tolist() == [[0, 1, 0], [3, 0, 5], [6, 7, 8]]      # id 0: 4-neighbours only
    assert metrics.components_host(np.zeros((2, 0, 3), np.uint8)).shape == (2, 0, 3)
    with pytest.raises(ValueError, match="connectivity"):
        metrics.components_host(m, 6)
    with pytest.raises(ValueError, match="3 dimensions"):
        metrics.components_host(m[0])


def test_the_named_cases_are_what_their_names_say():
    """the component counts that make the cases worth running"""
    def count(name, conn, t=0, bg=False):
        lab = CC.expected(name, conn, bg)[t]
        return len(np.unique(lab[lab >= 0]))
    assert count("serpentine", 4) == 1 and count("spiral", 4) == 1 and count("comb_u", 4) == 1 and count("comb_u_mirrored", 4) == 1
    assert int(CC.cases()["serpentine"][0].sum()) > 30 * CC.TC and int(CC.cases()["spiral"][0].sum()) > 15 * CC.TC        # long paths
    assert count("checkerboard", 8) == 2 and count("checkerboard", 4) == CC.H * CC.W
    for t in (0, 1):
        assert count("diagonal_through_tile_corners", 8, t) == 1 and count("diagonal_through_tile_corners", 4, t) > 30
        assert count("blocks_touching_at_a_tile_corner", 8, t) == 1 and count("blocks_touching_at_a_tile_corner", 4, t) == 2
    zeros = int((CC.cases()["diagonal_through_tile_corners"][2] == 0).sum())          # each its own component: id 0 is 4-connected
    assert count("diagonal_through_tile_corners", 8, 2, bg=True) == 1 + zeros and count("diagonal_through_tile_corners", 4, 2, bg=True) == 2 + zeros
    assert count("blocks_touching_at_a_tile_corner", 8, 2) == 1
    assert len(np.unique(CC.cases()["all_256_ids"][0])) == 256
    lab = CC.expected("last_row_equals_next_first_row", 8, False)
    assert lab[0, CC.H - 1, 0] == (CC.H - 1) * CC.W and lab[1, 0, 5] == 0 and lab[2, 0, 5] == 3


# ---- the cleaning rule against answers written out by hand ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CC.clean_cases()))
def test_clean_masks_host_gives_the_written_answer(name):
    from fgvc_amd import metrics
    c = CC.clean_cases()[name]
    out, stats = metrics.clean_masks_host(c["ids"], c["n_ids"], **CC.clean_kwargs(c["kw"]))
    assert out.dtype == np.uint8 and stats.dtype == np.int64
    assert np.array_equal(out, c["want"]), (name, out)
    assert np.array_equal(stats, c["stats"]), (name, stats.tolist())
    assert not stats[:, 0].any()


def test_clean_masks_host_refusals():
    from fgvc_amd import metrics
    m = np.zeros((1, 3, 3), np.uint8)
    for kw, word in ((dict(n_ids=0), "n_ids"), (dict(n_ids=257), "n_ids"), (dict(connectivity=6), "connectivity"), (dict(keep="biggest"), "keep"),
                     (dict(frames=[True, False]), "frames")):
        with pytest.raises(ValueError, match=word):
            metrics.clean_masks_host(m, **{"n_ids": 2, **kw})


# ---- deliberately wrong restatements: each must differ from the contract on the case named beside it ---------------------------------------
def _four_for_eight(ids, connectivity=8, background=False):
    from fgvc_amd import metrics
    return metrics.components_host(ids, 4 if connectivity == 8 else 8, background)


def _one_forward_pass(ids, connectivity=8, background=False):
    """a single raster pass: a pixel takes the smallest label among its already-labelled neighbours, and no equivalence is ever resolved"""
    ids = np.asarray(ids)
    T, h, w = ids.shape
    out = np.full((T, h, w), -1, np.int32)
    for t in range(T):
        for y in range(h):
            for x in range(w):
                v = ids[t, y, x]
                if v == 0 and not background:
                    continue
                near = [(y, x - 1), (y - 1, x)] + ([(y - 1, x - 1), (y - 1, x + 1)] if connectivity == 8 and v != 0 else [])
                seen = [out[t, j, i] for j, i in near if 0 <= j and 0 <= i < w and ids[t, j, i] == v]
                out[t, y, x] = min(seen) if seen else y * w + x
    return out


def _ignoring_ids(ids, connectivity=8, background=False):
    from fgvc_amd import metrics
    return metrics.components_host((np.asarray(ids) != 0).astype(np.uint8), connectivity, background)


def _frames_joined(ids, connectivity=8, background=False):
    """the clip labelled as one tall frame: the flat index runs from a frame's last row into the next frame's first"""
    from fgvc_amd import metrics
    ids = np.asarray(ids)
    T, h, w = ids.shape
    lab = metrics.components_host(ids.reshape(1, T * h, w), connectivity, background).reshape(T, h, w).astype(np.int64)
    return np.where(lab >= 0, lab - np.arange(T)[:, None, None] * h * w, -1).astype(np.int32)


def _ties_to_the_larger_root(ids, n_ids, **kw):
    """keep='largest' with equal areas decided for the LARGER root: the contract on the map turned by 180 degrees"""
    from fgvc_amd import metrics
    out, stats = metrics.clean_masks_host(np.asarray(ids)[:, ::-1, ::-1], n_ids, **kw)
    return out[:, ::-1, ::-1], stats


def _fill_before_drop(ids, n_ids, min_area=0, keep="all", fill_holes=False, **kw):
    from fgvc_amd import metrics
    filled, _ = metrics.clean_masks_host(ids, n_ids, fill_holes=fill_holes, **kw)
    return metrics.clean_masks_host(filled, n_ids, min_area=min_area, keep=keep, **{k: v for k, v in kw.items() if k in ("connectivity", "frames")})


COMPONENT_MUTANTS = ((_four_for_eight, "diagonal_through_tile_corners", 8), (_four_for_eight, "blocks_touching_at_a_tile_corner", 4),
                     (_one_forward_pass, "comb_u", 8), (_one_forward_pass, "serpentine", 4), (_ignoring_ids, "checkerboard", 8),
                     (_frames_joined, "last_row_equals_next_first_row", 8))
CLEAN_MUTANTS = ((_ties_to_the_larger_root, "equal_areas_the_smaller_root_stays"), (_fill_before_drop, "speck_inside_is_dropped_then_filled"))


@pytest.mark.parametrize("mutant,name,conn", COMPONENT_MUTANTS, ids=[f"{m.__name__}-{n}-{c}" for m, n, c in COMPONENT_MUTANTS])
def test_the_component_cases_tell_a_wrong_restatement_from_the_contract(mutant, name, conn):
    wrong = mutant(CC.cases()[name], conn, False)
    assert wrong.shape == CC.expected(name, conn, False).shape and not np.array_equal(wrong, CC.expected(name, conn, False))


@pytest.mark.parametrize("mutant,name", CLEAN_MUTANTS, ids=[f"{m.__name__}-{n}" for m, n in CLEAN_MUTANTS])
def test_the_clean_cases_tell_a_wrong_restatement_from_the_contract(mutant, name):
    c = CC.clean_cases()[name]
    out, _ = mutant(c["ids"], c["n_ids"], **CC.clean_kwargs(c["kw"]))
    assert out.shape == c["want"].shape and not np.array_equal(out, c["want"])


# ---- test_cfg.clean --------------------------------------------------------------------------------------------------------------------------
def test_parse_clean():
    from fgvc_amd import engine
    assert engine.parse_clean(None) is None
    cfg = engine.parse_clean(dict(min_area=16, keep="largest", connectivity=4, fill_holes=True, max_hole_area=9))
    assert cfg == engine.CleanConfig(16, "largest", 4, True, 9) and cfg.active
    assert cfg.kwargs() == dict(min_area=16, keep="largest", connectivity=4, fill_holes=True, max_hole_area=9)
    for spec in ({}, dict(min_area=0), dict(min_area=1, keep="all", fill_holes=False)):
        cfg = engine.parse_clean(spec)
        assert isinstance(cfg, engine.CleanConfig) and not cfg.active                # accepted; the call launches nothing for it
    assert engine.parse_clean(dict(min_area=2)).active and engine.parse_clean(dict(fill_holes=True)).active
    for spec, word in ((dict(area=3), "area"), (True, "test_cfg.clean"), (dict(min_area=-1), "min_area"), (dict(min_area=2.5), "min_area"),
                       (dict(min_area=True), "min_area"), (dict(keep="biggest"), "keep"), (dict(connectivity=6), "connectivity"),
                       (dict(fill_holes=1), "fill_holes"), (dict(max_hole_area=-2), "max_hole_area"), (dict(max_hole_area="3"), "max_hole_area")):
        with pytest.raises(ValueError, match=word):
            engine.parse_clean(spec)


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------
ENTRIES = ("fgvc_seg_components_i32", "fgvc_seg_clean_u8", "fgvc_seg_clean_workspace_bytes", "fgvc_seg_ccl_tile_rows", "fgvc_seg_ccl_tile_cols")


def test_entries_are_declared_exported_and_validate():
    import re
    from fgvc_amd import _lib, build, ops
    assert "components.hip" in build.SOURCES
    with open(os.path.join(ROOT, "include", "fgvc_hip.h")) as f:
        text = f.read()
    lib = _lib.load()
    for name in ENTRIES:
        decl = re.search(r"(?:int|size_t) " + name + r"\(([^;]*)\);", text)
        assert decl and name in _lib.SIGNATURES and hasattr(lib, name), name
        params = [p for p in decl.group(1).split(",") if p.strip() != "void"]
        assert len(params) == len(_lib.SIGNATURES[name][1]), name                                  # one ctypes argument per declared parameter
    assert (lib.fgvc_seg_ccl_tile_rows(), lib.fgvc_seg_ccl_tile_cols()) == (CC.TR, CC.TC) == ops.CCL_TILE
    assert lib.fgvc_seg_clean_workspace_bytes(2, 5, 7, 3) == 2 * 3 * 8 + 2 * 5 * 7 * 12
    assert lib.fgvc_seg_clean_workspace_bytes(0, 5, 7, 3) == 0 and lib.fgvc_seg_clean_workspace_bytes(2, 5, 7, 257) == 0
    buf = C.create_string_buffer(4096)                                                              # never reached
    p = C.cast(buf, C.c_void_p)

    def comps(ids=p, st=16, sy=4, T=1, h=4, w=4, conn=8, bg=0, out=p):
        return lib.fgvc_seg_components_i32(ids, st, sy, T, h, w, conn, bg, out, None)
    for kw, word in ((dict(ids=None), b"ids"), (dict(out=None), b"labels"), (dict(T=0), b"T="), (dict(h=0), b"h="), (dict(w=-3), b"w="),
                     (dict(conn=6), b"connectivity"), (dict(bg=2), b"background"), (dict(sy=3), b"ids_stride_y"),
                     (dict(T=2, st=-16), b"ids_stride_y"), (dict(h=1 << 16, w=1 << 15, sy=1 << 15), b"2^31")):
        assert comps(**kw) == _lib.ERR_INVALID_ARG and lib.fgvc_last_error().startswith(b"fgvc_seg_components_i32: ") \
            and word in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())

    def clean(ids=p, st=16, sy=4, T=1, h=4, w=4, n=3, conn=8, min_area=0, largest=0, fill=0, hole=-1, flags=None, out=p, ost=16, osy=4, stats=p,
              ws=p, ws_bytes=4096):
        return lib.fgvc_seg_clean_u8(ids, st, sy, T, h, w, n, conn, min_area, largest, fill, hole, flags, out, ost, osy, stats, ws, ws_bytes, None)
    need = lib.fgvc_seg_clean_workspace_bytes(1, 4, 4, 3)
    other = C.cast(C.addressof(buf) + 2048, C.c_void_p)
    for kw, word in ((dict(ids=None), b"ids"), (dict(out=None), b"out"), (dict(stats=None), b"stats"), (dict(ws=None), b"workspace"),
                     (dict(ws=C.cast(C.addressof(buf) + 4, C.c_void_p)), b"workspace"), (dict(ws_bytes=need - 1), b"workspace_bytes"),
                     (dict(n=0), b"n_ids"), (dict(n=257), b"n_ids"), (dict(T=0), b"T="), (dict(h=0), b"h="), (dict(w=0), b"w="),
                     (dict(conn=5), b"connectivity"), (dict(min_area=-1), b"min_area"), (dict(largest=2), b"keep_largest"),
                     (dict(fill=-1), b"fill_holes"), (dict(sy=3), b"ids_stride_y"), (dict(osy=3), b"out_stride_y"),
                     (dict(out=other, T=2, ost=8), b"out_stride_t"), (dict(osy=8, ost=32), b"in place"),
                     (dict(h=1 << 16, w=1 << 15, sy=1 << 15, osy=1 << 15), b"2^31")):
        assert clean(**kw) == _lib.ERR_INVALID_ARG and lib.fgvc_last_error().startswith(b"fgvc_seg_clean_u8: ") \
            and word in lib.fgvc_last_error(), (kw, lib.fgvc_last_error())


def test_wrapper_refusals_without_a_gpu():
    from fgvc_amd import _lib, ops
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.seg_components(torch.zeros(1, 4, 4, dtype=torch.uint8))
    with pytest.raises(_lib.FgvcHipError, match="GPU"):
        ops.seg_clean(torch.zeros(1, 4, 4, dtype=torch.uint8), 2)


def test_kernels_use_no_scratch():
    """The code-object notes of the built library: none of the component kernels uses scratch memory or spills a register, vector or scalar;
    the tile kernel's LDS is a label word and an id halfword per pixel of the tile, and 1024 threads a workgroup leave at most 128 VGPRs."""
    notes = _tool("kernel_notes").kernel_notes()
    ours = {k: v for k, v in notes.items() if "ccl_" in k}
    assert len(ours) == 6, sorted(ours)
    for k, v in ours.items():
        assert v["private_segment_fixed_size"] == 0 and v["vgpr_spill_count"] == 0 and v["sgpr_spill_count"] == 0 and v["vgpr_count"] <= 128, (k, v)
        assert v["group_segment_fixed_size"] == (CC.TR * CC.TC * 6 if "ccl_tile_kernel" in k else 0), (k, v)
