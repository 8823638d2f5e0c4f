"""Shared cases of the J&F counts kernel (fgvc_jf_counts_u8) and its numpy restatement.

counts_host is built from the pieces metrics.f_measure itself uses (metrics._seg2bmap, metrics._disk, scipy's binary_dilation), so the
kernel is held to the host scorer with `==`.  A case is (gt, pred, n_objects, radius): two (T, h, w) uint8 id maps; the radius reaches
f_measure as bound_th >= 1, i.e. in pixels, whatever the image size.  The shapes are the smallest at which the kernel can go wrong: it
packs 64 pixels of a row into a word, a workgroup owns ops.JF_TILE rows, and the disk reads a halo of `radius` rows and one word."""
import functools

import numpy as np

from fgvc_amd import metrics

JF_TILE = 32            # = ops.JF_TILE = fgvc_jf_tile_rows(): tests/test_jf_host.py checks all three agree


def counts_host(gt: np.ndarray, pred: np.ndarray, n: int, r: int) -> np.ndarray:
    """(T, n, 6) int64: |G & S|, |G | S|, |b(S)|, |b(G)|, |b(S) & dil b(G)|, |b(G) & dil b(S)| per frame and object 1 .. n."""
    from scipy.ndimage import binary_dilation
    fp = metrics._disk(int(r))
    out = np.zeros((gt.shape[0], n, 6), np.int64)
    for t in range(gt.shape[0]):
        for o in range(1, n + 1):
            G, S = gt[t] == o, pred[t] == o
            bS, bG = metrics._seg2bmap(S), metrics._seg2bmap(G)
            dS = binary_dilation(bS, structure=fp) if bS.any() else bS
            dG = binary_dilation(bG, structure=fp) if bG.any() else bG
            out[t, o - 1] = [(G & S).sum(), (G | S).sum(), bS.sum(), bG.sum(), (bS & dG).sum(), (bG & dS).sum()]
    return out


def jf_host(gt: np.ndarray, pred: np.ndarray, n: int, r: int):
    """(J, F), each (T, n) float64, from metrics.db_eval_iou and metrics.f_measure themselves."""
    J, F = np.zeros((gt.shape[0], n)), np.zeros((gt.shape[0], n))
    for t in range(gt.shape[0]):
        for o in range(1, n + 1):
            G, S = gt[t] == o, pred[t] == o
            J[t, o - 1] = metrics.db_eval_iou(G, S)
            F[t, o - 1] = metrics.f_measure(S, G, bound_th=r)
    return J, F


def _blobs(rng, T, h, w, n, cell=8, noise=0.35):
    """Smooth random fields, one per id: their argmax is a map of blobs with ragged edges."""
    coarse = rng.random((T, n + 1, -(-h // cell) + 1, -(-w // cell) + 1))
    f = np.kron(coarse, np.ones((cell, cell)))[:, :, cell // 2:cell // 2 + h, cell // 2:cell // 2 + w]
    return f, lambda: (f + noise * rng.random(f.shape)).argmax(1).astype(np.uint8)


def _rect(m, t, y0, y1, x0, x1, o):
    m[t, y0:y1 + 1, x0:x1 + 1] = o          # edges INCLUDED: y0 .. y1, x0 .. x1


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20260)
    c = {}
    # ragged: the width crosses one 64-pixel word, the height one tile
    _, draw = _blobs(rng, 2, 37, 70, 3)
    c["ragged_2x37x70"] = (draw(), draw(), 3, 3)
    # two words plus one pixel; rectangle edges at x in {0, 63, 64, 127, 128}, y in {0, h - 1} and on the tile seam (rows 31 | 32)
    h, w = JF_TILE + 1, 129
    g, p = np.zeros((3, h, w), np.uint8), np.zeros((3, h, w), np.uint8)
    _rect(g, 0, 0, 20, 0, 63, 1); _rect(p, 0, 0, 22, 0, 64, 1)
    _rect(g, 0, 25, h - 1, 64, 128, 2); _rect(p, 0, 24, h - 1, 60, 127, 2)
    _rect(g, 1, JF_TILE - 2, h - 1, 120, 128, 1); _rect(p, 1, JF_TILE - 1, h - 1, 127, 128, 1)
    _rect(g, 1, 5, JF_TILE - 1, 62, 65, 2); _rect(p, 1, 6, JF_TILE, 63, 64, 2)
    _rect(g, 2, JF_TILE, JF_TILE, 0, 128, 1); _rect(p, 2, JF_TILE - 1, JF_TILE - 1, 1, 127, 1)      # one-row objects either side of the seam
    _rect(g, 2, 3, 12, 128, 128, 2); _rect(p, 2, 0, 9, 127, 127, 2)                                  # one-column objects at the right border
    c["two_words_plus_one_3x33x129"] = (g, p, 2, 8)
    # the disk is larger than the image
    c["disk_over_image_1x5x6"] = (rng.integers(0, 3, (1, 5, 6)).astype(np.uint8), rng.integers(0, 3, (1, 5, 6)).astype(np.uint8), 2, 8)
    # degenerate images
    g, p = np.zeros((1, 1, 130), np.uint8), np.zeros((1, 1, 130), np.uint8)
    g[0, 0, 10:65], p[0, 0, 12:64], g[0, 0, 100:130], p[0, 0, 127:129] = 1, 1, 2, 2
    c["one_row_1x1x130"] = (g, p, 2, 3)
    c["one_column_1x130x1"] = (g.reshape(1, 130, 1).copy(), p.reshape(1, 130, 1).copy(), 2, 3)
    c["one_pixel_1x1x1"] = (np.ones((1, 1, 1), np.uint8), np.ones((1, 1, 1), np.uint8), 1, 2)
    # the disk's edge: one ground-truth pixel, one predicted pixel at (dy, dx); host F = 1, 1, 0.75, 0.75 (tests/test_jf_host.py)
    g, p = np.zeros((4, 40, 40), np.uint8), np.zeros((4, 40, 40), np.uint8)
    g[:, 20, 20] = 1
    for t, (dy, dx) in enumerate(DISK_EDGE_OFFSETS):
        p[t, 20 + dy, 20 + dx] = 1
    c["disk_edge_4x40x40"] = (g, p, 1, 5)
    # borders and empties (n = 3, an id of 7 in pred)
    h, w = 24, 40
    g, p = np.zeros((4, h, w), np.uint8), np.zeros((4, h, w), np.uint8)
    g[0], p[0] = 1, 1                                              # frame-filling in both: no boundary at all; objects 2, 3 in neither
    g[1, 10], g[1, :, 15], p[1, 11], p[1, :, 17] = 1, 1, 1, 1      # a cross touching all four borders
    _rect(g, 1, 2, 6, 20, 30, 2)                                   # object 2 in gt only
    _rect(p, 1, 14, 20, 22, 35, 3)                                 # object 3 in pred only
    _rect(p, 1, 0, 3, 0, 5, 7)                                     # id 7 > n: no object
    g[2] = 1; _rect(p, 2, 4, 15, 6, 30, 1)                         # gt fills the frame (no boundary), pred does not
    _rect(g, 2, 0, 2, 0, 2, 2); _rect(p, 2, h - 3, h - 1, w - 3, w - 1, 2)       # far apart: boundaries on both sides, no hit
    p[3] = 1; _rect(g, 3, 4, 15, 6, 30, 1)                         # pred fills the frame, gt does not
    c["borders_and_empties_4x24x40"] = (g, p, 3, 2)
    # many objects
    c["many_objects_1x16x16"] = (rng.integers(0, 256, (1, 16, 16)).astype(np.uint8), rng.integers(0, 256, (1, 16, 16)).astype(np.uint8), 255, 2)
    # the radius limit
    _, draw = _blobs(rng, 1, 40, 50, 2)
    c["radius_64_1x40x50"] = (draw(), draw(), 2, 64)
    # seeded random blobs
    _, draw = _blobs(rng, 2, 48, 64, 3)
    c["blobs_2x48x64"] = (draw(), draw(), 3, 4)
    return c


DISK_EDGE_OFFSETS = ((3, 4), (5, 0), (5, 1), (4, 4))
DISK_EDGE_F = (1.0, 1.0, 0.75, 0.75)


@functools.lru_cache(maxsize=None)
def expected(name: str) -> np.ndarray:
    """counts_host of a case, computed once per session and shared (treat as read-only)."""
    gt, pred, n, r = cases()[name]
    out = counts_host(gt, pred, n, r)
    out.setflags(write=False)
    return out


def davis_sequences():
    """Two synthetic sequences of 6 x 48 x 64 ids (one cut to T = 2: both frames are then scored), predictions as float64."""
    rng = np.random.default_rng(7)
    seqs = {}
    for name, T, n in (("six", 6, 3), ("two", 2, 2)):
        _, draw = _blobs(rng, T, 48, 64, n, noise=0.25)
        gt, pred = draw(), draw()
        pred[0] = gt[0]
        seqs[name] = (gt, pred.astype(np.float64))
    return seqs
