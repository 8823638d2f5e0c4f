"""Cases and restatements for the flow-chaining point tracker (fgvc_amd/csrc/chain.hip), shared by the CPU and the GPU
tests and by tests/golden/gen_golden_chain.py.  `chain_ref` restates the whole rule -- the reference's chain (raft.py:247-289 on
bilinear_sample2d, samp.py:5-99), the 'consistency' visibility and the fail-closed rule -- in plain Python loops over one point at a time,
written from the rule's text, not from fgvc_amd.engine: it records every hop of a walk first and decides visibility afterwards."""
import math

import numpy as np

from tests import flow_cases as FC

F32 = np.float32
LIMIT = 2.0 ** 23
FIXTURES = ("chain_6x37x53", "chain_3x2x70", "chain_2x1x1", "chain_24x24x32")


def _usable(x, y):
    return math.isfinite(x) and math.isfinite(y) and abs(x) < LIMIT and abs(y) < LIMIT


def _in_frame(x, y, h, w):
    return 0 <= x < w and 0 <= y < h           # (a NaN fails)


def _sample(plane, x, y):
    """bilinear_sample2d of one plane at the float32 position (x, y)."""
    h, w = plane.shape
    fx, fy = F32(math.floor(x)), F32(math.floor(y))
    gx, gy = F32(fx + F32(1)), F32(fy + F32(1))
    cols = [min(max(int(fx) + d, 0), w - 1) for d in (0, 1)]
    rows = [min(max(int(fy) + d, 0), h - 1) for d in (0, 1)]
    wx, wy = [F32(gx - x), F32(x - fx)], [F32(gy - y), F32(y - fy)]
    acc = None
    for j in (0, 1):
        for i in (0, 1):
            term = F32(F32(wx[i] * wy[j]) * plane[rows[j], cols[i]])
            acc = term if acc is None else F32(acc + term)
    return acc


def _walk(fields, oks, steps, x, y):
    """One side of a track: `steps` = [(frame written, field index)].  Returns [(frame, x, y, hop_good)] up to the first unusable position."""
    out = []
    for t, g in steps:
        if not _usable(x, y):
            break
        h, w = fields[g][0].shape
        good = True
        if oks is not None:
            xn, yn = min(max(math.floor(F32(x + F32(0.5))), 0), w - 1), min(max(math.floor(F32(y + F32(0.5))), 0), h - 1)
            good = _in_frame(x, y, h, w) and oks[g][yn, xn] != 0
        with np.errstate(all="ignore"):
            x, y = F32(x + _sample(fields[g][0], x, y)), F32(y + _sample(fields[g][1], x, y))
        if not _usable(x, y):
            break
        out.append((t, x, y, good))
    return out


def chain_ref(flow_fw, flow_bw, query, ok_fw=None, ok_bw=None, visibility="frame"):
    """traj (T, P, 2) float32, vis (T, P) uint8."""
    flow_fw, flow_bw, query = np.asarray(flow_fw, F32), np.asarray(flow_bw, F32), np.asarray(query, F32)
    n, _, h, w = flow_fw.shape
    T, P = n + 1, len(query)
    sticky = visibility == "consistency"
    assert visibility in ("frame", "consistency") and (not sticky or (ok_fw is not None and ok_bw is not None))
    traj, vis = np.full((T, P, 2), np.nan, F32), np.zeros((T, P), np.uint8)
    for p in range(P):
        qt, qx, qy = query[p]
        if not (math.isfinite(qt) and qt == math.floor(qt) and 0 <= qt < T):
            continue
        tq = int(qt)
        traj[tq, p], vis[tq, p] = (qx, qy), _in_frame(qx, qy, h, w)
        sides = (_walk(flow_fw, ok_fw if sticky else None, [(t, t - 1) for t in range(tq + 1, T)], qx, qy),
                 _walk(flow_bw, ok_bw if sticky else None, [(t, t) for t in range(tq - 1, -1, -1)], qx, qy))
        for hops in sides:
            for i, (t, x, y, _) in enumerate(hops):
                traj[t, p] = (x, y)
                vis[t, p] = _in_frame(x, y, h, w) and all(g for _, _, _, g in hops[:i + 1])
    return traj, vis


def bits(a):
    """The bit patterns of a float32 array (so that == places NaNs and tells -0 from +0)."""
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- case builders --------------------------------------------------------------------------------------------------------------------
def flows(T, h, w, amp, seed):
    """flow_fw, flow_bw (T-1, 2, h, w) float32: two independent smooth fields of amplitude `amp` px."""
    return FC.smooth_field((T - 1, 2, h, w), seed, amp), FC.smooth_field((T - 1, 2, h, w), seed + 1, amp)


def queries(P, T, h, w, seed, margin=2.0):
    """(P, 3) float32 = (t, x, y): random integer times of [0, T), positions up to `margin` px outside the frame on every side."""
    rng = np.random.default_rng(seed)
    q = np.empty((P, 3), F32)
    q[:, 0] = rng.integers(0, T, P)
    q[:, 1] = rng.uniform(-margin, w + margin, P)
    q[:, 2] = rng.uniform(-margin, h + margin, P)
    return q


def masks(T, h, w, seed, keep=0.8):
    """ok_fw, ok_bw (T-1, h, w) uint8: about `keep` of the pixels set."""
    rng = np.random.default_rng(seed)
    return tuple((rng.random((T - 1, h, w)) < keep).astype(np.uint8) for _ in range(2))


def poisoned(T, h, w, seed):
    """A case whose point 0 (query time 1, at a pixel centre) reads a NaN planted in flow_fw[1] and whose point 1 reads an inf planted in
    flow_bw[0]: flows, query (P = 6), and the two points' numbers."""
    assert T >= 3 and h >= 8 and w >= 8
    fw, bw = flows(T, h, w, 1.5, seed)
    q = queries(6, T, h, w, seed + 2, margin=0.0)
    q[0], q[1] = (1, 3, 4), (1, 5, 2)
    fw[1, 0, 4, 3] = np.nan                    # the forward hop 1 -> 2 of point 0 has weight 1 on this tap
    bw[0, 1, 2, 5] = np.inf                    # the backward hop 1 -> 0 of point 1
    return fw, bw, q
