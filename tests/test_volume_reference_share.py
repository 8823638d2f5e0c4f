"""CPU: what tests/test_gpu_volume_ops.py relies on, checked from the restatements alone (tests/volume_cases.py).

* volume64 is the oracle's corr_volume; split_bf16_model is torch's own bfloat16 rounding (round to nearest even on the CPU).
* The FORMAT halves of the two-part bounds, on the very rows the GPU module uses: bf16x3 within 2.0001 * 2^-16 A0 / tau and plain bf16
  within 2 * 2^-9 A0 / tau of volume64 on every entry (derived in volume_cases' docstring); the f16f8 / f16f6 formats, stated on the
  host, within the project bar 1e-3 on unit-norm rows at tau 0.07.  These are properties of the number formats and are not derived
  tighter here; the GPU module asserts the other half (the kernel against its own model) on every entry.
* By plain arithmetic on the shapes -- written out from the comments of the .hip files, without a call into the library -- every case
  id reaches what it names.
"""
import numpy as np
import pytest
import torch

from oracle import fgvc_oracle as O
from tests import volume_cases as VC


# ----------------------------------------------------------------------------------------------------------------------
# the restatements
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 256])
def test_volume64_is_the_oracle(C):
    g = torch.Generator().manual_seed(C)
    (Hq, Wq), (Hk, Wk) = (5, 7), (4, 9)
    q, k = torch.randn(C, Hq, Wq, generator=g) * 3, torch.randn(C, Hk, Wk, generator=g) * 3
    rows = lambda x: x.flatten(1).t().contiguous()
    want = O.corr_volume(q.double(), k.double(), 0.07, normalize=False)
    got = VC.volume64(rows(q), rows(k), 0.07)
    assert got.shape == want.shape == (Hk * Wk, Hq * Wq)
    assert torch.allclose(got, want, rtol=1e-13, atol=1e-12)
    qn, kn = O.l2_normalize(q.double(), 0), O.l2_normalize(k.double(), 0)            # normalised rows: the default call
    assert torch.allclose(VC.volume64(rows(qn), rows(kn), 0.07), O.corr_volume(q.double(), k.double(), 0.07), rtol=1e-12, atol=1e-12)
    val, A = VC.f32_model64(rows(q), rows(k), 0.07)
    assert torch.equal(val, got) and bool((A >= (got * 0.07).abs() - 1e-9).all())


@pytest.mark.parametrize("shape", [(67, 64, 3), (1, 4, 8), (300, 256, 9)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_split_bf16_model_is_torch_bfloat16(shape):
    n, C, seed = shape
    rows = VC.split_rows(n, C, seed)
    assert np.isfinite(rows).all()
    mag = np.abs(rows[rows != 0])
    assert mag.min() >= 2.0 ** -61 and mag.max() <= 2.0 ** 61                        # far inside the normal range
    x = torch.from_numpy(rows)
    hi = x.bfloat16()
    res = x - hi.float()
    assert float(res[res != 0].abs().min()) >= 2.0 ** -100                           # every non-zero residual is a normal f32 too
    lo = res.bfloat16()
    want = torch.stack([hi.view(torch.int16), lo.view(torch.int16)], dim=-2)
    got = torch.from_numpy(VC.split_bf16_model(rows))
    assert got.shape == (n, 2, C) and torch.equal(got, want)
    if C >= 8:   # the row classes are what they say
        bits = rows.view(np.uint32)
        cls = np.arange(C) % 8
        assert ((bits[:, cls == 1] & 0x1FFFF) == 0x08000).all() and ((bits[:, cls == 2] & 0x1FFFF) == 0x18000).all()     # ties: even / odd above
        assert (res[:, torch.from_numpy(cls == 3)] == 0).all() and (rows[:, cls == 7] == 0).all()
        assert np.signbit(rows[1::2, cls == 7]).all() and not np.signbit(rows[0::2, cls == 7]).any()
        # a tie rounds to even: down above an even bf16, up above an odd one
        h = got[:, 0].numpy().view(np.uint16).astype(np.uint32)
        assert (h[:, cls == 1] == bits[:, cls == 1] >> 16).all() and (h[:, cls == 2] == (bits[:, cls == 2] >> 16) + 1).all()
        r6 = res[:, torch.from_numpy(cls == 6)].numpy().view(np.uint32)
        assert ((r6 & 0xFFFF) == 0x8000).all() and (r6 != 0).all()                   # the residual is a tie of its own


def test_bf16_parts_round_trip():
    rows = VC.split_rows()
    hi, lo = VC.bf16_parts(VC.split_bf16_model(rows))
    x = torch.from_numpy(rows).double()
    nz = x != 0
    assert bool(((x - hi).abs()[nz] <= 2.0 ** -8 * x.abs()[nz]).all()) and bool((lo.abs()[nz] <= 2.0 ** -8 * x.abs()[nz]).all())
    assert bool(((x - hi - lo).abs()[nz] <= 2.0 ** -17 * x.abs()[nz]).all())
    assert float(((x - hi - lo).abs()[nz] / x.abs()[nz]).max()) > 2.0 ** -19                      # and the rows come close to it
    assert float((lo == 0).double().mean()) >= 0.2 and float((lo != 0).double().mean()) >= 0.5    # both kinds of residual are there


# ----------------------------------------------------------------------------------------------------------------------
# part 2 of the bounds: the formats, from the models alone
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", VC.bf16_cases(), ids=lambda c: c[-1])
def test_bf16_format_bounds(case):
    C, HWq, HWk, tau, kind, name = case
    q, k = VC.pair_rows(kind, HWq, HWk, C)
    qs, ks = VC.split_bf16_model(q), VC.split_bf16_model(k)
    ref, A0 = VC.volume64(q, k, tau), VC.abs64(q, k)
    for what, model64, fmt in (("bf16x3", VC.bf16x3_model64, VC.BF16X3_FORMAT), ("bf16", VC.bf16_model64, VC.BF16_FORMAT)):
        val, A = model64(qs, ks, tau)
        err, bound = (val - ref).abs(), fmt * A0 / tau
        live = bound > 0
        ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
        print(f"{what} {name} {kind}: max |model - volume64| {float(err.max()):.3e}, largest err / format bound {ratio:.3f}")
        assert bool((err <= bound).all()), (what, ratio)
        assert bool((A <= A0 * (1 + 2.0 ** -5)).all())
    if kind != "raw30":      # unit-norm rows: both parts of bf16x3 together stay far inside the project bar
        assert (VC.BF16X3_FORMAT + VC.accum_n("bf16x3", C) * VC.U24) * 1.0001 / VC.TEMP < VC.TOL


@pytest.mark.parametrize("case", VC.f8_cases(), ids=lambda c: c[-1])
def test_narrow_format_bar(case):
    """f16f8 and f16f6 as the .hip files document them, stated on the host: the three sums stay within 1e-3 of volume64"""
    HWq, HWk, kind, name = case
    q, k = VC.pair_rows(kind, HWq, HWk, 256, False)
    ref = VC.volume64(q, k, VC.TEMP)
    for what, split, model64 in (("f16f8", VC.split_f16f8_host, VC.f16f8_model64), ("f16f6", VC.split_f16f6_host, VC.f16f6_model64)):
        val, A = model64(split(q), split(k), VC.TEMP)
        err = float((val - ref).abs().max())
        print(f"{what} {name} {kind}: max |model - volume64| {err:.3e}")
        assert err < VC.TOL, (what, err)
        assert VC.accum_n(what, 256) * VC.U24 * float(A.max()) / VC.TEMP < VC.TOL / 4           # the accumulation half is small beside it


def test_narrow_host_formats_are_the_documented_ones():
    q, _ = VC.pair_rows("heavy", 200, 5, 256, False)
    h, h8, l8 = VC.split_f16f8_host(q)
    _, l = VC.f16_parts_host(q)
    assert (np.abs(h8 - h) <= np.maximum(np.abs(h) / 16, 2.0 ** -10)).all() and (np.abs(l8 - l) <= np.maximum(np.abs(l) / 16, 2.0 ** -10)).all()
    assert np.isin(np.abs(h8), VC.E4M3[:127]).all() and np.isin(np.abs(l8), VC.E4M3[:127]).all()
    h, h6, l6 = VC.split_f16f6_host(q)
    for got, ref in ((h6 * 16, h), (l6 * 16, l)):        # test_split_f16f6_format's statement of the GPU rows
        bm = np.abs(ref).reshape(-1, 8, 32).max(-1, keepdims=True).repeat(32, -1).reshape(ref.shape)
        assert (np.abs(got - ref) <= np.maximum(np.abs(ref) / 16, bm / 7.5 / 8) * 1.0001 + 1e-30).all()
    assert float(VC.E4M3[0x7E]) == 448.0 and float(VC.E4M3[0x38]) == 1.0 and float(VC.E4M3[1]) == 2.0 ** -9 and np.isnan(VC.E4M3[0x7F])


# ----------------------------------------------------------------------------------------------------------------------
# every case id reaches what it names
# ----------------------------------------------------------------------------------------------------------------------
def test_f32_and_bf16_cases_reach_their_chunks():
    KCHUNK = 16                                            # key blocks of 32 per workgroup (corr_volume.hip)
    shapes = {what: (HWq, HWk) for HWq, HWk, what in VC.F32_SHAPES}
    for HWq, HWk, what in VC.F32_SHAPES:                   # the f32 launch and the C = 64 / 128 bf16 launch keep KCHUNK at these sizes
        n_q, n_kb = VC.cdiv(HWq, 128), VC.cdiv(HWk, 32)
        assert max(KCHUNK, VC.cdiv(n_kb, max(1, 2048 // n_q))) == KCHUNK
    HWq, HWk = shapes["17blocks_chunk2_one_live_row"]
    assert VC.cdiv(HWk, 32) == 17 > KCHUNK and HWk - 16 * 32 == 1 and HWq % 128 == 1
    HWq, HWk = shapes["35blocks_16_16_3"]
    assert VC.cdiv(HWk, 32) == 35 == 16 + 16 + 3 and HWk % 32 != 0 and HWq % 32 != 0
    assert shapes["exact_tiles"] == (128, 32) and shapes["one_over"] == (129, 33) and shapes["smallest"] == (1, 1)
    assert all(c in (32, 64, 128, 256) for c in VC.F32_C) and set(VC.F32_TAU_SMALL) == set(VC.F32_C)
    # every C meets every kind of row, and a multi-chunk shape with each of at least two kinds
    for C in VC.F32_C:
        mine = [c for c in VC.f32_cases() if c[0] == C]
        assert {c[4] for c in mine} == set(VC.KINDS3)
        assert len({c[4] for c in mine if VC.cdiv(c[2], 32) > KCHUNK}) >= 2
    # C = 256, bf16: 8 waves = 256 queries, stages of two key blocks, kchunk = max(16, ...) rounded up to even
    s256 = {what: (HWq, HWk) for HWq, HWk, what in VC.BF16_256_SHAPES}
    for HWq, HWk, what in VC.BF16_256_SHAPES:
        n_q, n_kb = VC.cdiv(HWq, 256), VC.cdiv(HWk, 32)
        k = max(16, VC.cdiv(n_kb, max(1, 1024 // n_q)))
        assert k + (k & 1) == 16
    HWq, HWk = s256["33blocks_16_16_1_half_stage"]
    assert VC.cdiv(HWk, 32) == 33 and (33 - 32) % 2 == 1 and HWk % 32 == 0 and HWq == 2 * 256 + 1      # the last chunk: one block = half a stage
    HWq, HWk = s256["35blocks_16_16_3_stage_then_half"]
    assert VC.cdiv(HWk, 32) == 35 and (35 - 32) == 3                                                   # a full stage, then half a stage
    HWq, HWk = s256["all_full_two_chunks_counted_wait_only"]
    assert HWq % 256 == 0 and HWk % 64 == 0 and VC.cdiv(HWk, 32) == 32                                 # every wave, block and stage full; two chunks
    assert s256["under_one_tile"] == (255, 63) and s256["one_full_tile"] == (256, 64) and s256["over_one_tile"] == (257, 65)
    assert {c[4] for c in VC.bf16_cases() if c[0] == 256 and VC.cdiv(c[2], 32) > 16} == set(VC.KINDS3)


def test_narrow_cases_reach_every_row_class():
    want = {256: (0, 1), 240: (16, 2), 48: (16, 2), 232: (8, 4), 248: (24, 4), 40: (8, 4), 255: (31, 1), 33: (1, 1)}
    for HWq, (m, p) in want.items():
        assert HWq & 31 == m and VC.row_class_period(HWq)[0] == p
    assert sorted(want) == sorted(VC.F8_HWQ)
    # both sides of the +31 in n_q = cdiv(HWq + 31, 256) for each shifted period
    nq = {HWq: VC.f8_geometry(HWq, 64)["n_q"] for HWq in VC.F8_HWQ}
    assert nq[240] == 2 and nq[48] == 1 and nq[232] == 2 and nq[248] == 2 and nq[40] == 1 and nq[256] == 1 and nq[255] == 1
    for HWq in (240, 232, 248):
        assert VC.cdiv(HWq, 256) == 1                      # the second query tile exists only because of the shift
    # classes without a row: HWk below the period
    for HWq, HWk, kind, name in VC.f8_cases():
        geo = VC.f8_geometry(HWq, HWk)
        assert sum(geo["n_v"]) == HWk and ("nv0" in name) == (HWk < geo["period"]) == (min(geo["n_v"]) == 0)
    ids = [c[-1] for c in VC.f8_cases()]
    assert sum("p2" in i and "nv0" in i for i in ids) == 2 and sum("p4" in i and "nv0" in i for i in ids) == 9      # HWk 1 | HWk 1, 2, 3
    assert VC.f8_geometry(256, 200)["n_vb"] == 7                                       # 7 virtual blocks at p = 1
    assert {k for _, _, k, _ in VC.f8_cases()} == set(VC.KINDS4)
    # 609 at p = 1: s_tile = 10 admits c_half = 5 (2 s_tile / c >= 4); 576 does not yet
    assert VC.f6_geometry(256, 609)["s_tile"] == 10 and VC.f6_geometry(256, 609, 5)["admitted"] and not VC.f6_geometry(256, 576, 5)["admitted"]


def test_forced_chunkings_reach_what_they_name():
    for HWq, HWk, kc in VC.F8_KC_CASES:
        assert kc % 2 == 0 and kc > 0                      # the stage loop walks two key blocks at a time
        geo = VC.f8_geometry(HWq, HWk, kc)
        assert geo["kchunk"] == kc and geo["chunks"] == VC.cdiv(geo["n_vb"], kc)
    assert VC.f8_geometry(256, 609, 2)["chunks"] == 10 and VC.f8_geometry(256, 200, 2)["last_chunk_blocks"] == 1       # an odd tail: the break inside a stage
    assert VC.f8_geometry(256, 609, 4)["chunks"] == 5 and VC.f8_geometry(256, 200, 4)["last_chunk_blocks"] == 3
    assert any(VC.f8_geometry(HWq, HWk, kc)["chunks"] > 1 and VC.f8_geometry(HWq, HWk, kc)["period"] == 4 for HWq, HWk, kc in VC.F8_KC_CASES)
    assert any(min(VC.f8_geometry(HWq, HWk, kc)["n_v"]) == 0 for HWq, HWk, kc in VC.F8_KC_CASES)
    # classes of unequal length under a forced chunk: class 1's second workgroup starts behind the class's last block (kb0 = 2 >= kb1 = 2)
    # although the class has rows; in every other case only the classes without rows have kb0 >= kb1
    geo = VC.f8_geometry(240, 129, 2)
    assert geo["period"] == 2 and geo["n_v"] == [65, 64] and geo["n_vb"] == 3 and geo["chunks"] == 2
    assert VC.cdiv(geo["n_v"][1], 32) == 2 <= (geo["chunks"] - 1) * geo["kchunk"] < VC.cdiv(geo["n_v"][0], 32)
    seen_c, crossing_two_real_tiles, lone_second = set(), False, False
    for HWq, HWk, c in VC.F6_C_CASES:
        geo = VC.f6_geometry(HWq, HWk, c)
        assert geo["admitted"], (HWq, HWk, c)              # 2 s_tile / c >= 4: the launch's own search could have picked it
        assert geo["c_half"] == c and geo["cuts"][0] == 0 and geo["cuts"][-1] == 2 * geo["s_tile"]
        assert all(a < b for a, b in zip(geo["cuts"][:-1], geo["cuts"][1:]))            # no empty piece
        assert geo["crossing"] == bool(c & 1)                # an odd c: one piece runs from one tile into the next
        seen_c.add(c)
        crossing_two_real_tiles |= geo["crossing"] and geo["n_tiles"] >= 2
        lone_second |= geo["n_tiles"] % 2 == 1             # n_q * period odd: the last pair has no second tile
    assert seen_c == {1, 2, 3, 4, 5} and crossing_two_real_tiles and lone_second
    assert VC.f6_geometry(513, 609)["n_tiles"] == 3 and VC.f6_geometry(48, 1100)["period"] == 2 and VC.f6_geometry(48, 1100)["n_tiles"] == 2
    for HWq in (256, 255, 33):                             # HWq <= 256 at p = 1: one tile, the pair's second tile does not exist
        assert VC.f6_geometry(HWq, 609)["n_tiles"] == 1
    for HWq, HWk in VC.F6_SDMA_CASES:
        assert (HWq, HWk) in [(c[0], c[1]) for c in VC.f8_cases()]
    # c = 1: the single piece covers both tiles of the pair, i.e. it crosses too
    assert VC.f6_geometry(48, 609, 1)["cuts"] == [0, 2 * VC.f6_geometry(48, 609)["s_tile"]]
    HWq, HWk, kind = VC.BASE_SHAPE
    assert VC.row_class_period(HWq) == (2, True) and HWk % 32 != 0


def test_accumulation_constants():
    assert [VC.accum_n("f32", C) for C in (32, 64, 128, 256)] == [19, 35, 67, 131]
    assert VC.accum_n("bf16x3", 64) == 68 and VC.accum_n("f16f6", 256) == 260
    assert VC.GUARD % 4 == 0
