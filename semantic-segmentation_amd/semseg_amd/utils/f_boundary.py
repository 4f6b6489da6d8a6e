"""Boundary F-score on the device (utils/f_boundary.py of the reference: eval_mask_boundary, db_eval_boundary, seg2bmap).

  boundary_radius     the reference's `bound_pix` (f_boundary.py:127-128) as an integer
  boundary_counts     int64 [B,C,4] = {n_fg, n_gt, fg_match, gt_match} per (image, class) in two launches
                      (ssa_fboundary_counts, csrc/fboundary.hip), device tensors in, device tensor out, no synchronisation
  f_scores            precision, recall and F from the counts, float64 on the host, the reference's four branches (:154-171)
  eval_mask_boundary  the reference's function of that name: (Fpc, Fc) as NumPy float64
  BoundaryMeter       accumulates the counts of a validation run on the device; `.avg` is what the reference's
                      `eval_metrics` (utils/misc.py) reads from its `mf_score` argument

`dropin.install(device_f_boundary=True)` puts this module under `utils.f_boundary`.  The per-class boolean maps, the
1,257-tap dilation and the 10-process pool of the reference do not exist here; nothing falls back to the host.
"""
import ctypes
import sys

import numpy as np
import torch

from .._lib import lib, check

MAX_CLASSES = 254
MAX_RADIUS = 32

_SYNC_CFG = [False]       # dropin.install(device_f_boundary=True): refresh our cfg from the reference's on every call


def _cfg():
    from ..config import cfg
    if _SYNC_CFG[0] and "config" in sys.modules and hasattr(sys.modules["config"], "assert_and_infer_cfg"):
        from ..dropin import sync_config
        sync_config()
    return cfg


def boundary_radius(shape, bound_th=0.008):
    """f_boundary.py:127-128: bound_th itself from 1 on, else ceil(bound_th * ||(H, W)||) in NumPy's float64.  A bound_th
    >= 1 that is no integer (the reference would build an even-sized footprint) and a radius outside 0..32 raise."""
    H, W = int(shape[0]), int(shape[1])
    if H <= 0 or W <= 0:
        raise ValueError("boundary_radius: the image is %d x %d" % (H, W))
    bound_pix = bound_th if bound_th >= 1 else np.ceil(bound_th * np.linalg.norm((H, W)))
    r = int(bound_pix)
    if r != bound_pix:
        raise ValueError("bound_th = %r is neither below 1 nor an integer" % (bound_th,))
    if not 0 <= r <= MAX_RADIUS:
        raise ValueError("boundary radius %d for bound_th = %r at %d x %d: 0..%d are supported" % (r, bound_th, H, W, MAX_RADIUS))
    return r


def _refuse_capture(t):
    """The metric is not offered inside a graph capture (torch.cuda.graph): a captured boundary_counts in one process
    with the captured training step ended in a crash of that step's replay, cause unknown.  It runs eagerly."""
    if t.is_cuda and torch.cuda.is_current_stream_capturing():
        raise RuntimeError("boundary_counts is not supported inside a graph capture: call it eagerly")


def boundary_counts(pred, gts, num_classes, ignore_label, bound_th=0.008):
    """pred: uint8 [B,H,W] on the device (what eval_tail returns as `pred`); gts: uint8 or int64 [B,H,W] on the same
    device.  Returns int64 [B,C,4] = {n_fg, n_gt, fg_match, gt_match} on the device; nothing waits for it."""
    from .. import hip_backend as hb
    if not (torch.is_tensor(pred) and torch.is_tensor(gts)):
        raise ValueError("boundary_counts takes device tensors")
    if pred.dtype != torch.uint8 or pred.dim() != 3:
        raise ValueError("boundary_counts: pred must be uint8 [B, H, W]")
    if gts.dtype not in (torch.uint8, torch.int64) or tuple(gts.shape) != tuple(pred.shape):
        raise ValueError("boundary_counts: gts must be uint8 or int64 of pred's shape")
    if gts.device != pred.device:
        raise ValueError("boundary_counts: pred and gts are on different devices")
    C = int(num_classes)
    if not 1 <= C <= MAX_CLASSES:
        raise ValueError("boundary_counts: 1..%d classes are supported, not %d" % (MAX_CLASSES, C))
    B, H, W = pred.shape
    if not 1 <= B <= 65535 or H < 1 or W < 1:
        raise ValueError("boundary_counts: shape %s" % (tuple(pred.shape),))
    r = boundary_radius((H, W), bound_th)
    _refuse_capture(pred)
    pred, gts = pred.contiguous(), gts.contiguous()
    counts = torch.empty((B, C, 4), dtype=torch.int64, device=pred.device)
    work = torch.empty((2, B, H, W), dtype=torch.int32, device=pred.device)
    check(lib().ssa_fboundary_counts(hb._p(pred), hb._p(gts), int(gts.dtype == torch.uint8), B, H, W, C, int(ignore_label),
                                     r, hb._p(counts), hb._p(work), ctypes.c_size_t(work.numel() * 4), hb._s()),
          "ssa_fboundary_counts")
    return counts


def f_scores(counts):
    """(F, precision) as float64 [B,C] NumPy arrays from counts [B,C,4] (tensor on any device, or array):
    f_boundary.py:154-171 -- only the ground truth present: P = 1, R = 0; only the prediction: P = 0, R = 1; neither:
    P = R = 1; else fg_match / n_fg and gt_match / n_gt; F = 0 where P + R == 0, else 2 P R / (P + R)."""
    c = counts.detach().cpu().numpy() if torch.is_tensor(counts) else np.asarray(counts)
    if c.ndim != 3 or c.shape[2] != 4:
        raise ValueError("f_scores: counts must be [B, C, 4]")
    c = c.astype(np.int64)
    n_fg, n_gt, fg_m, gt_m = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
    has_fg, has_gt = n_fg > 0, n_gt > 0
    both = has_fg & has_gt
    with np.errstate(divide="ignore", invalid="ignore"):
        P = np.where(both, fg_m / n_fg.astype(np.float64), np.where(has_fg, 0.0, 1.0))
        R = np.where(both, gt_m / n_gt.astype(np.float64), np.where(has_gt, 0.0, 1.0))
        F = np.where(P + R == 0, 0.0, 2 * P * R / (P + R))
    return F, P


def _sum_over_batch(F):
    """Fpc as the reference's `sum(Fs)` takes it: image by image from 0."""
    Fpc = np.zeros(F.shape[1])
    for i in range(F.shape[0]):
        Fpc = Fpc + F[i]
    return Fpc


def _as_pred_u8(t):
    """class ids of any integer type as the kernel's bytes: what is outside 0..254 becomes 255 (no class)"""
    if t.dtype == torch.uint8:
        return t
    t = t.long()
    return torch.where((t < 0) | (t > 254), torch.full_like(t, 255), t).to(torch.uint8)


def eval_mask_boundary(seg_mask, gt_mask, num_classes, num_proc=10, bound_th=0.008, *, device=None):
    """utils/f_boundary.py:61-92: returns (Fpc, Fc), per class the sum of F over the batch and the number of images (no
    F is NaN here, so that is the batch size).  seg_mask, gt_mask: [B,H,W] NumPy arrays or tensors on any device, moved
    to `device` (default: where a tensor argument already is on a GPU, else the current GPU) once and left unchanged;
    num_proc is accepted and ignored; cfg.DATASET.IGNORE_LABEL is read at call time."""
    ignore = int(_cfg().DATASET.IGNORE_LABEL)
    seg = seg_mask if torch.is_tensor(seg_mask) else torch.from_numpy(np.ascontiguousarray(seg_mask))
    gt = gt_mask if torch.is_tensor(gt_mask) else torch.from_numpy(np.ascontiguousarray(gt_mask))
    if device is None:
        device = next((t.device for t in (seg, gt) if t.is_cuda), torch.device("cuda"))
    seg, gt = seg.to(device), gt.to(device)
    if gt.dtype not in (torch.uint8, torch.int64):
        gt = gt.long()
    counts = boundary_counts(_as_pred_u8(seg), gt, num_classes, ignore, bound_th)
    F, _ = f_scores(counts)
    return _sum_over_batch(F), np.full(int(num_classes), float(F.shape[0]))


class BoundaryMeter:
    """The boundary F-score of a validation run.  update() launches the kernels and keeps the [B,C,4] counts on the
    device; Fpc, Fc and avg copy them to the host once, when read.  `avg` = mean over classes of Fpc / Fc is what the
    reference's eval_metrics records as `mask_f1_score` (utils/misc.py reads `mf_score.avg`)."""

    def __init__(self, num_classes=None, ignore_label=None, bound_th=0.008):
        self.num_classes, self.ignore_label, self.bound_th = num_classes, ignore_label, bound_th
        self.reset()

    def reset(self):
        self._counts = []
        self._host = None

    def update(self, pred, gts):
        cfg = _cfg()
        C = int(cfg.DATASET.NUM_CLASSES if self.num_classes is None else self.num_classes)
        ignore = int(cfg.DATASET.IGNORE_LABEL if self.ignore_label is None else self.ignore_label)
        if self._counts and self._counts[0].shape[1] != C:
            raise ValueError("BoundaryMeter: %d classes after %d" % (C, self._counts[0].shape[1]))
        gts = gts.to(pred.device)
        if gts.dtype not in (torch.uint8, torch.int64):
            gts = gts.long()
        self._counts.append(boundary_counts(_as_pred_u8(pred), gts, C, ignore, self.bound_th))
        self._host = None

    def add_counts(self, counts):
        """counts [B,C,4] taken elsewhere (boundary_counts), tensor or array"""
        self._counts.append(counts if torch.is_tensor(counts) else torch.as_tensor(np.asarray(counts), dtype=torch.int64))
        self._host = None

    def counts(self):
        """int64 [N,C,4] on the host, N = images so far: one device-to-host copy after the last update"""
        if self._host is None:
            if not self._counts:
                raise ValueError("BoundaryMeter: nothing accumulated")
            self._host = torch.cat([c.reshape(-1, c.shape[1], 4) for c in self._counts]).cpu().numpy()
        return self._host

    @property
    def Fpc(self):
        return _sum_over_batch(f_scores(self.counts())[0])

    @property
    def Fc(self):
        c = self.counts()
        return np.full(c.shape[1], float(c.shape[0]))

    @property
    def avg(self):
        return float(np.mean(self.Fpc / self.Fc))
