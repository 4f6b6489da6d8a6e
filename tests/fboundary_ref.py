"""Restatement of the reference's boundary F-score (utils/f_boundary.py) in NumPy + scipy.ndimage, independent of the
library: per (image, class) the two dense boolean maps, seg2bmap's three shifted XORs with its last-row, last-column
and corner rules, binary_dilation with the dx^2 + dy^2 <= r^2 footprint (what skimage.morphology.disk and
binary_dilation are), the four integer sums, then precision, recall and F with the reference's four branches in Python
scalars.  tests/test_fboundary_cpu.py holds it to the golden data of the real reference with ==."""
import numpy as np
import scipy.ndimage as ndi


def radius(shape, bound_th):
    """f_boundary.py:127-128"""
    return bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm(shape))


def disk(r):
    r = int(r)
    y, x = np.mgrid[-r:r + 1, -r:r + 1]
    return x * x + y * y <= r * r


def seg2bmap(seg):
    """f_boundary.py:193-223 for width = height = None"""
    seg = seg.astype(bool)
    e = np.zeros_like(seg)
    s = np.zeros_like(seg)
    se = np.zeros_like(seg)
    e[:, :-1] = seg[:, 1:]
    s[:-1, :] = seg[1:, :]
    se[:-1, :-1] = seg[1:, 1:]
    b = seg ^ e | seg ^ s | seg ^ se
    b[-1, :] = seg[-1, :] ^ e[-1, :]
    b[:, -1] = seg[:, -1] ^ s[:, -1]
    b[-1, -1] = 0
    return b


def dilate(b, r):
    if not b.any():
        return b
    return ndi.binary_dilation(b, structure=disk(r))


def counts(pred, gt, num_classes, ignore_label, r):
    """int64 [B,C,4] = {n_fg, n_gt, fg_match, gt_match}; pred, gt: integer arrays [B,H,W]"""
    pred, gt = np.asarray(pred).astype(np.int64), np.asarray(gt).astype(np.int64)
    B = pred.shape[0]
    out = np.zeros((B, num_classes, 4), dtype=np.int64)
    for i in range(B):
        ign = gt[i] == ignore_label
        for c in np.union1d(np.unique(pred[i]), np.unique(gt[i])):
            if not 0 <= c < num_classes:
                continue
            fg_b = seg2bmap((pred[i] == c) & ~ign)
            gt_b = seg2bmap((gt[i] == c) & ~ign)
            out[i, c] = (fg_b.sum(), gt_b.sum(), (fg_b & dilate(gt_b, r)).sum(), (gt_b & dilate(fg_b, r)).sum())
    return out


def scores(cnt):
    """(F, precision) float64 [B,C], entry by entry in Python scalars as f_boundary.py:154-171 takes them"""
    cnt = np.asarray(cnt)
    F = np.zeros(cnt.shape[:2])
    P = np.zeros(cnt.shape[:2])
    for i in range(cnt.shape[0]):
        for c in range(cnt.shape[1]):
            n_fg, n_gt, fg_match, gt_match = (np.int64(v) for v in cnt[i, c])
            if n_fg == 0 and n_gt > 0:
                precision, recall = 1, 0
            elif n_fg > 0 and n_gt == 0:
                precision, recall = 0, 1
            elif n_fg == 0 and n_gt == 0:
                precision, recall = 1, 1
            else:
                precision, recall = fg_match / float(n_fg), gt_match / float(n_gt)
            F[i, c] = 0 if precision + recall == 0 else 2 * precision * recall / (precision + recall)
            P[i, c] = precision
    return F, P


def fpc_fc(F):
    """what eval_mask_boundary returns from the per-image F of a batch (:87-92)"""
    Fpc = np.zeros(F.shape[1])
    Fc = np.zeros(F.shape[1])
    for c in range(F.shape[1]):
        Fc[c] = F.shape[0]
        Fpc[c] = sum(F[:, c])
    return Fpc, Fc


def branch(cnt):
    """which of the four branches an entry takes: 'gt', 'pred', 'none', 'both'"""
    n_fg, n_gt = int(cnt[0]), int(cnt[1])
    return "gt" if n_fg == 0 and n_gt > 0 else "pred" if n_fg > 0 and n_gt == 0 else "none" if n_fg == 0 else "both"
