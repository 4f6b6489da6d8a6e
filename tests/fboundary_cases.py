"""The seeded cases of the boundary F-score tests (tests/test_fboundary_cpu.py, tests/test_fboundary_gpu.py and, under
the CPU emulation, tests/test_fboundary_emu_cpu.py) and of tests/golden/make_golden_fboundary.py.  Every case is a few
thousand pixels: the smallest shapes at which each rule of the specification can break.

  seam_r2/r3/r20  19 classes, 2 x 70 x 131 in 8 x 8 blocks: 5 x 3 tiles of the match kernel (16 rows x 64 columns) with
                  ragged last tiles (70 = 4 * 16 + 6, 131 = 2 * 64 + 3); the prediction is the ground truth rolled by
                  (2, -3) with 3 % noise; 2 % scattered ignore pixels and one ignore rectangle; radius 20 is larger than
                  the tile height, so a halo crosses two neighbouring tile rows
  disk_out/in     radius 5, the ground truth one pixel of class 0: the prediction is class 0 at every offset with
                  25 < d^2 <= 36 (just outside the disk) / 16 < d^2 <= 25 (just inside): the disk against a square and
                  against radius 4 and 6 -- the offsets (3,4), (4,4) and (5,1) decide
  edge_*          1 x 1, 1 x 9, 9 x 1 and 2 x 2 images (last row, last column, corner), and 5 x 7 with bound_th = 8
  branches        all four branches of precision / recall, and 0 < match < n in both directions for class 0
  labels65        65 classes with ignore = 65, ground-truth labels that are neither a class nor the ignore label (70, 255,
                  -1: int64 only), prediction bytes >= C
  checker         every pixel a boundary: a checkerboard prediction, radius 4
  c254_r0, r32    the limits: 254 classes at radius 0; radius 32 on a small image
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "fboundary_golden.npz")
TILE_H, TILE_W = 16, 64          # csrc/fboundary.hip


def _blocks(rs, C, B, H, W, bs):
    g = rs.randint(0, C, (B, (H + bs - 1) // bs, (W + bs - 1) // bs))
    return np.repeat(np.repeat(g, bs, 1), bs, 2)[:, :H, :W].astype(np.int64)


def _seam():
    rs = np.random.RandomState(8101)
    B, H, W, C = 2, 70, 131, 19
    gt = _blocks(rs, C, B, H, W, 8)
    pred = np.roll(gt, (2, -3), (1, 2)).copy()
    noise = rs.rand(B, H, W) < 0.03
    pred[noise] = rs.randint(0, C, int(noise.sum()))
    gt = gt.copy()
    gt[rs.rand(B, H, W) < 0.02] = 255
    gt[0, 20:37, 50:80] = 255          # across the seam of tile columns 0 | 1 and of tile rows 1 | 2
    gt[1, 60:70, 120:131] = 255        # the ragged bottom-right tile
    return pred.astype(np.uint8), gt


def _disk(lo, hi):
    n, c = 17, 8
    gt = np.ones((1, n, n), np.int64)
    pred = np.ones((1, n, n), np.uint8)
    gt[0, c, c] = 0
    for dy in range(-6, 7):
        for dx in range(-6, 7):
            if lo < dx * dx + dy * dy <= hi:
                pred[0, c + dy, c + dx] = 0
    return pred, gt


def _edge(seed, H, W):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 3, (2, H, W)).astype(np.uint8), rs.randint(0, 3, (2, H, W)).astype(np.int64)


def _branches():
    gt = np.full((1, 24, 40), 4, np.int64)
    pred = np.full((1, 24, 40), 4, np.uint8)
    gt[0, 2:10, 2:12] = 0
    pred[0, 2:10, 2:18] = 0            # class 0: three sides match, the right side is 6 > r away
    gt[0, 14:20, 2:8] = 1              # class 1: ground truth only
    pred[0, 14:20, 12:18] = 3          # class 3: prediction only
    gt[0, 2:6, 24:28] = 2              # class 2: both, nowhere within r
    pred[0, 16:20, 32:36] = 2
    return pred, gt                    # classes 5, 6, 7: neither


def _labels65():
    rs = np.random.RandomState(8102)
    B, H, W, C = 1, 20, 30, 65
    gt = _blocks(rs, C, B, H, W, 4)
    pred = np.roll(gt, (1, 1), (1, 2)).astype(np.uint8)
    gt[rs.rand(B, H, W) < 0.05] = 65   # the ignore label
    gt[0, 3:8, 4:9] = 70               # neither a class nor the ignore label
    gt[0, 12:15, 20:26] = 255
    gt[0, 16:19, 2:7] = -1
    pred[0, 5:9, 14:19] = 65           # prediction bytes >= C
    pred[0, 10:13, 1:4] = 200
    pred[0, 0:2, 25:30] = 255
    return pred, gt


def _checker():
    rs = np.random.RandomState(8103)
    H, W = 18, 70
    gt = _blocks(rs, 3, 1, H, W, 6)
    yy, xx = np.mgrid[0:H, 0:W]
    pred = ((yy + xx) % 2).astype(np.uint8)[None]
    gt[0, 4:7, 60:66] = 255
    return pred, gt


def _c254():
    rs = np.random.RandomState(8104)
    gt = rs.randint(0, 254, (1, 12, 20)).astype(np.int64)
    pred = gt.astype(np.uint8).copy()
    m = rs.rand(1, 12, 20) < 0.5
    pred[m] = rs.randint(0, 254, int(m.sum()))
    return pred, gt


def _r32():
    rs = np.random.RandomState(8105)
    gt = _blocks(rs, 5, 1, 12, 40, 4)
    pred = np.roll(gt, 17, 2).astype(np.uint8)
    return pred, gt


INPUTS = {
    "seam": _seam, "disk_out": lambda: _disk(25, 36), "disk_in": lambda: _disk(16, 25),
    "e1x1": lambda: _edge(1, 1, 1), "e1x9": lambda: _edge(2, 1, 9), "e9x1": lambda: _edge(3, 9, 1),
    "e2x2": lambda: _edge(4, 2, 2), "e5x7": lambda: _edge(5, 5, 7), "branches": _branches, "labels65": _labels65,
    "checker": _checker, "c254": _c254, "r32": _r32,
}

# name: inputs, classes, ignore label, bound_th (an integer radius, or a fraction of the diagonal)
CASES = {
    "seam_r2": dict(inp="seam", C=19, ignore=255, bound_th=2),
    "seam_r3": dict(inp="seam", C=19, ignore=255, bound_th=0.02),      # ceil(0.02 * 148.52) = 3
    "seam_r20": dict(inp="seam", C=19, ignore=255, bound_th=20),
    "disk_out": dict(inp="disk_out", C=2, ignore=255, bound_th=5),
    "disk_in": dict(inp="disk_in", C=2, ignore=255, bound_th=5),
    "edge_1x1": dict(inp="e1x1", C=3, ignore=255, bound_th=1),
    "edge_1x9": dict(inp="e1x9", C=3, ignore=255, bound_th=1),
    "edge_9x1": dict(inp="e9x1", C=3, ignore=255, bound_th=1),
    "edge_2x2": dict(inp="e2x2", C=3, ignore=255, bound_th=1),
    "edge_5x7_r8": dict(inp="e5x7", C=3, ignore=255, bound_th=8),
    "branches": dict(inp="branches", C=8, ignore=255, bound_th=2),
    "labels65": dict(inp="labels65", C=65, ignore=65, bound_th=2),
    "checker": dict(inp="checker", C=3, ignore=255, bound_th=4),
    "c254_r0": dict(inp="c254", C=254, ignore=255, bound_th=0),
    "r32": dict(inp="r32", C=5, ignore=255, bound_th=32),
}
ALL = tuple(CASES)

_INP = {}


def inputs(name):
    """(pred uint8 [B,H,W], gt int64 [B,H,W]) of a case, from its seed; read-only"""
    key = CASES[name]["inp"]
    if key not in _INP:
        pred, gt = INPUTS[key]()
        pred.setflags(write=False)
        gt.setflags(write=False)
        _INP[key] = (pred, gt)
    return _INP[key]


def fits_u8(name):
    gt = inputs(name)[1]
    return bool(gt.min() >= 0 and gt.max() <= 255)


_GOLDEN = None


def golden():
    global _GOLDEN
    if _GOLDEN is None:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _GOLDEN = {k: z[k] for k in z.files}
    return _GOLDEN


_REF = {}


def reference(name):
    """The restatement's answer for a case, computed once: dict(r, counts int64 [B,C,4], F, P float64 [B,C], Fpc, Fc)."""
    if name not in _REF:
        import fboundary_ref as R
        k = CASES[name]
        pred, gt = inputs(name)
        r = int(R.radius(pred.shape[1:], k["bound_th"]))
        cnt = R.counts(pred, gt, k["C"], k["ignore"], r)
        F, P = R.scores(cnt)
        Fpc, Fc = R.fpc_fc(F)
        for a in (cnt, F, P, Fpc, Fc):
            a.setflags(write=False)
        _REF[name] = dict(r=r, counts=cnt, F=F, P=P, Fpc=Fpc, Fc=Fc)
    return _REF[name]
