"""Shared cases of the edge-aware read-out tests (test_guided_host.py on the CPU, test_gpu_guided.py on the GPU): geometries, inputs, the
error bound of the kernel's f32 arithmetic, and the disc prototype.

THE BOUND (value_bound).  The kernel (fgvc_amd/csrc/guided.hip) evaluates, per output pixel and channel, v = sum_i w_i L_i / sum_i w_i over
N = (2 radius + 1)^2 taps with w_i = exp(-a_i), a_i = e_i - e_min >= 0, in f32 (unit roundoff u = 2^-24); engine.guided_readout_host
evaluates the same in float64 from the same f32 inputs.  What follows bounds |v_f32 - v_f64| to first order in u.

  geometry   The centre cell and the guide's bilinear taps come from integer divisions: exact.  A spatial offset (i - fy) is
             (float)di - t with t = (float)rem / (float)D - 0.5: rem and D are integers below 2^24 (exact), so the offset carries at most
             2 relative roundings, its square 5, the sum of two squares 6, and the product with 1 / (2 sigma_space^2) (itself rounded once
             from double) 8:   |d e_space| <= 8 u e_space.
  colours    I: three fused multiply-adds on differences of guide values, |dI| <= 10 u gmax (gmax = max |guide|).  A cell colour is a
             sum of sy values, a sum of sx such sums and one division, all in order: |dGc| <= (sy + sx - 1) u gmax.  d = I - Gc adds one
             rounding of a value <= 2 gmax.  So each colour difference is off by at most Kd u gmax with Kd = 12 + sy + sx -- an ABSOLUTE
             error: the subtraction cancels, so it is not small relative to d.
             e_range = |d|^2 / (2 sigma_range^2) then moves by at most sqrt(3) |d| Kd u gmax / sigma_range^2
             = sqrt(6 e_range) Kd u G with G = gmax / sigma_range, plus 8 u e_range from its own six roundings and the rounded constant.
  exponent   |d e_i| <= 8 u e_i + sqrt(6 e_i) Kd u G (+ 1 u e_i for the sum of the two parts).  The f32 minimum is within the same
             bound, taken at e_min, of the float64 one (min is 1-Lipschitz).  With e_i = a_i + e_min, e_min <= E (E = the largest e_min
             of the case, from the float64 rule) and one more rounding for the subtraction:
               |d a_i| <= u (10 a_i + 18 E) + sqrt(6) Kd u G (sqrt(a_i) + 2 sqrt(E)).
  weight     expf is accurate to 1 ulp here and its argument is rounded once more by the negation-free subtraction above:
               |d w_i| <= exp(-a_i) |d a_i| + 2 u w_i.
             The exponent's rounding error times a exp(-a) <= 1 / e, and sqrt(a) exp(-a) <= sqrt(1/2) exp(-1/2) < 0.43, give
               |d w_i| <= dw := u (10 / e + 18 E + 2) + sqrt(6) Kd u G (0.43 + 2 sqrt(E)).
  value      Labels (normalised or not) lie in [0, 1]; the normalisation (x - mn) / ((mx - mn) + 1e-12) costs 4 u relative to a value
             <= 1 whatever the spread (two subtractions, the rounded constant's sum, one division; the cases keep every spread either 0 or
             far above the denormal range).  Numerator and denominator are each off by at most N dw plus N u from
             their running sums, the denominator is >= 1 (the tap with e = e_min has weight 1) and v <= 1, the reciprocal and the
             product add 2 u:
               |d v| <= 2 N dw + (2 N + 6) u =: B.
The ids must agree wherever the float64 margin best - second exceeds 2 B, the confidence bytes within 1 there.  (A margin error of 2 B
moves 255 * margin by 510 B, which is below one level only where B < 1 / 510; the assertion stays at one level as specified.)
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
CHUNK = 16            # fgvc_guided_channel_chunk(): the GPU test checks that the library agrees
TILE = (8, 32)        # fgvc_guided_tile_rows() x fgvc_guided_tile_cols()
EXCLUDED_MAX = 0.005


def value_bound(case, E: float, gmax: float) -> float:
    sy, sx = case["hp"] // case["Hf"], case["wp"] // case["Wf"]
    N = (2 * case["radius"] + 1) ** 2
    Kd, G = 12 + sy + sx, gmax / case["sigma_range"]
    dw = U * (10 / math.e + 18 * E + 2) + math.sqrt(6) * Kd * U * G * (0.43 + 2 * math.sqrt(E))
    return 2 * N * dw + (2 * N + 6) * U


def _case(name, Hf, Wf, s, pad, out, n, C, radius, norm=True, sigma_range=0.1, sigma_space=1.0, guide="smooth", labels="blobs", seed=0):
    hp, wp = Hf * s, Wf * s
    return dict(name=name, Hf=Hf, Wf=Wf, hp=hp, wp=wp, pad=pad, out=out, n=n, C=C, radius=radius, norm=norm, sigma_range=sigma_range,
                sigma_space=sigma_space, guide=guide, labels=labels, seed=seed)


# pad = (left, right, top, bottom).  No output is larger than 64 x 96, and none is a multiple of the 8 x 32 tile except where it equals the frame.
CASES = [
    _case("g5x7-equal-C2-r1", 5, 7, 4, (0, 0, 0, 0), (20, 28), 1, 2, 1, seed=1),
    _case("g5x7-left-larger-C5-r2-n3", 5, 7, 4, (3, 0, 0, 0), (23, 33), 3, 5, 2, seed=2),
    _case("g5x7-right-smaller-C1-r3", 5, 7, 4, (0, 2, 0, 0), (13, 19), 1, 1, 3, seed=3),
    _case("g16x24-top-larger-C17-r2", 16, 24, 4, (0, 0, 3, 0), (64, 96), 1, CHUNK + 1, 2, seed=4),
    _case("g16x24-bottom-smaller-C5-r3-nonorm-n3", 16, 24, 4, (0, 0, 0, 2), (45, 70), 3, 5, 3, norm=False, seed=5),
    _case("g16x24-equal-C256-r2-nonorm", 16, 24, 4, (0, 0, 0, 0), (64, 96), 1, 256, 2, norm=False, seed=26),
    _case("g8x12s8-equal-C5-r2", 8, 12, 8, (0, 0, 0, 0), (64, 96), 1, 5, 2, seed=7),
    _case("g8x12s8-allsides-larger-C2-r1-n3", 8, 12, 8, (3, 2, 1, 4), (61, 93), 3, 2, 1, seed=8),
    _case("g8x12s8-smaller-C17-r3-nonorm", 8, 12, 8, (0, 0, 0, 0), (40, 50), 1, CHUNK + 1, 3, norm=False, seed=9),
    _case("g16x24-sr1e-3-palette-C5-r2", 16, 24, 4, (0, 0, 0, 0), (64, 96), 1, 5, 2, sigma_range=1e-3, guide="palette", labels="regions", seed=10),
    _case("g16x24-sr1e3-smaller-C5-r3", 16, 24, 4, (0, 0, 0, 0), (50, 75), 1, 5, 3, sigma_range=1e3, seed=11),
    _case("g16x24-left-ties-C4-r2", 16, 24, 4, (5, 0, 0, 0), (64, 91), 1, 4, 2, labels="ties", seed=12),
]


def geometry(case):
    """(Hf, Wf, pad_shape, pad, out_shape) as ops.seg_readout_guided takes them."""
    return case["Hf"], case["Wf"], (case["hp"], case["wp"]), case["pad"], case["out"]


def _fields(n, C, H, W, rng, waves=3, k=1.5):
    """(n, C, H, W) smooth random fields in about [-1, 1]: a few low-frequency cosines each."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = np.zeros((n, C, H, W))
    for f in range(n):
        for c in range(C):
            for _ in range(waves):
                ky, kx = rng.uniform(-k, k, 2) * np.pi / max(H, 1), rng.uniform(-k, k, 2) * np.pi / max(W, 1)
                out[f, c] += np.cos(ky[0] * y + kx[0] * x + rng.uniform(0, 2 * np.pi)) * np.cos(ky[1] * y + kx[1] * x + rng.uniform(0, 2 * np.pi))
    return out / waves


def _regions(case, rng):
    """(n, Hf, Wf) region ids in 0..C-1: 3 x 3-cell blocks, neighbours differ."""
    n, Hf, Wf, C = case["n"], case["Hf"], case["Wf"], case["C"]
    by, bx = (Hf + 2) // 3, (Wf + 2) // 3
    blocks = (np.add.outer(np.arange(by), 2 * np.arange(bx))[None] + rng.integers(0, C, (n, 1, 1))) % C
    return np.repeat(np.repeat(blocks, 3, 1), 3, 2)[:, :Hf, :Wf]


def make_inputs(case):
    """labels (n, Hf*Wf, C) f32 with rows in [0, 1], guide (n, 3, hp, wp) f32; deterministic per case."""
    rng = np.random.default_rng(1000 + case["seed"])
    n, Hf, Wf, C, hp, wp = (case[k] for k in ("n", "Hf", "Wf", "C", "hp", "wp"))
    if case["guide"] == "palette":
        # one colour per 3 x 3-cell region, multiples of 1/8 up to 1/2: cell means and bilinear samples are exact, colours differ by >= 1/8
        reg = _regions(case, rng)
        pal = (np.stack([reg % 5, (reg // 5 + 2 * reg) % 5, (3 * reg) % 5], 1) - 2) / 8.0           # (n, 3, Hf, Wf), in [-1/4, 1/4]
        guide = np.repeat(np.repeat(pal, hp // Hf, 2), wp // Wf, 3)
    else:
        guide = 0.5 * _fields(n, 3, hp, wp, rng) + 0.01 * rng.standard_normal((n, 3, hp, wp))
    if case["labels"] == "regions":
        logits = 7.0 * np.eye(C)[reg]                                                                 # (n, Hf, Wf, C): the region's own channel
        logits = logits + 0.05 * rng.standard_normal(logits.shape)
    else:
        amp = np.full(C, 40.0)
        if C > 8:                                                                                     # many channels: five strong ones, the last among them
            amp[:] = 8.0
            amp[[0, 2, 3, C // 2, C - 1]] = 40.0, 40.0, 40.0, 40.0, 70.0
        logits = amp * _fields(n, C, Hf, Wf, rng, waves=2, k=0.8).transpose(0, 2, 3, 1)
        if C >= 3 and case["labels"] == "blobs":
            logits[..., 1] = -np.inf                                                                  # (zeroed below: the rows still sum to 1)
    e = np.exp(logits - logits.max(-1, keepdims=True))
    lab = e / e.sum(-1, keepdims=True)
    if case["labels"] == "ties":
        # a propagated one-hot: the argmax's one-hot blurred by a 3 x 3 box; channel 2 is a copy of channel 1 (identical inputs: exact ties)
        hot = np.eye(C)[lab.argmax(-1)]
        padded = np.pad(hot, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
        lab = sum(padded[:, a:a + Hf, b:b + Wf] for a in range(3) for b in range(3)) / 9.0
        lab[..., 2] = lab[..., 1]
    elif C >= 3 and case["labels"] == "blobs":
        lab[..., 1] = 0.0                                                                             # a channel whose maximum is <= 0
    return torch.from_numpy(lab.reshape(n, Hf * Wf, C).astype(np.float32)), torch.from_numpy(guide.astype(np.float32))


_REF = {}


def reference(case):
    """(labels, guide, the float64 rule's GuidedReadout, B): computed once per case and shared; never modified."""
    key = case["name"]
    if key not in _REF:
        from fgvc_amd import engine
        lab, guide = make_inputs(case)
        Hf, Wf, pad_shape, pad, out = geometry(case)
        ref = engine.guided_readout_host(lab, guide, Hf, Wf, pad_shape, pad, out, case["norm"], case["radius"], case["sigma_space"],
                                         case["sigma_range"])
        B = value_bound(case, float(ref.e_min.max()), float(guide.abs().max()))
        _REF[key] = (lab, guide, ref, B)
    return _REF[key]


def decided(case, ref, B):
    """The pixels whose id the bound decides: margin > 2 B.  In the ties case channels 1 and 2 hold identical inputs, so their float64
    values are equal bit for bit and the margin there is exactly 0; a pixel whose best is that pair is decided (the first of the two
    must win) where the pair leads the other channels by more than 2 B."""
    if case["labels"] != "ties":
        return ref.margin > 2 * B
    v = ref.values
    others = v[..., [0, 3]].max(-1).values
    pair = v[..., 1]
    assert torch.equal(v[..., 1], v[..., 2])
    return (pair - others).abs() > 2 * B


# ---- the disc prototype ---------------------------------------------------------------------------------------------------------------------
DISC_H, DISC_W, DISC_R, DISC_C = 64, 96, 17.4, (30.3, 45.7)


def disc_inputs(stride, blur, noise=0.02, seed=0):
    """A disc of radius 17.4 px at a non-grid-aligned centre on a textured 64 x 96 frame.  Returns (truth (H, W) bool, labels (1, HfWf, 2)
    f32 = per-cell coverage blurred `blur` times by a 3 x 3 box, guide (1, 3, H, W) f32 = two textured colours + noise)."""
    rng = np.random.default_rng(seed)
    H, W = DISC_H, DISC_W
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    truth = (y - DISC_C[0]) ** 2 + (x - DISC_C[1]) ** 2 <= DISC_R ** 2
    Hf, Wf = H // stride, W // stride
    cov = truth.reshape(Hf, stride, Wf, stride).mean((1, 3))
    for _ in range(blur):
        p = np.pad(cov, 1, mode="edge")
        cov = sum(p[a:a + Hf, b:b + Wf] for a in range(3) for b in range(3)) / 9.0
    lab = np.stack([1 - cov, cov], -1).reshape(1, Hf * Wf, 2)
    tex = 0.03 * np.sin(0.9 * x) * np.cos(0.7 * y)
    fg, bg = np.array([0.6, 0.2, -0.3]), np.array([-0.2, -0.1, 0.4])
    guide = np.where(truth[None], fg[:, None, None], bg[:, None, None]) + tex[None] + noise * rng.standard_normal((3, H, W))
    return truth, torch.from_numpy(lab.astype(np.float32)), torch.from_numpy(guide[None].astype(np.float32))


def jaccard(a, b) -> float:
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / float((a | b).sum())


def bilinear_readout(lab, Hf, Wf, H, W):
    """The plain read-out of a frame that needs no padding: bilinear to (H, W), per-channel min-max over the map, argmax (seg_readout's rule)."""
    L = lab.double().reshape(1, Hf, Wf, -1).permute(0, 3, 1, 2)
    up = torch.nn.functional.interpolate(L, size=(H, W), mode="bilinear", align_corners=False)
    mn, mx = up.amin((2, 3), keepdim=True), up.amax((2, 3), keepdim=True)
    up = torch.where(mx > 0, (up - mn) / (mx - mn + 1e-12), up)
    return up.argmax(1)[0]
