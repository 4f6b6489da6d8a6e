"""The label half of the auto-labelled coarse data path (scripts/train_cityscapes_sota.yml: the `train_extra` images
with `coarse_boost_classes`, `custom_coarse_dropout_classes`, `mask_out_cityscapes` and `custom_coarse_prob`), on the
device (csrc/autolabel.hip, ssa_autolabel_u8).

The reference does this work in two places, with one whole-image NumPy pass per label id:
  * BaseLoader.read_images and the thresholding of __getitem__ (datasets/base_loader.py:152-229), once per item and
    epoch: the drop mask, the id -> trainId loop against the mask as rewritten so far with the gtCoarse merge of the
    boosted classes, and `prob / 255.0 < CUSTOM_COARSE_PROB -> IGNORE_LABEL`.  Here: read_labels (mode "current").
  * class_centroids_image (datasets/uniform.py:104-121), once per image when the centroid cache is built: the same loop
    with the hit taken against an untouched copy.  Here: datasets/uniform.py calls prepare_labels(mode="original").

Both are four launches per batch of same-sized maps, whatever the number of ids: see include/semseg_hip.h."""
import os

import numpy as np
import torch

from ..config import cfg

DEVICE = "cuda"                       # where read_labels sends the decoded maps
DROP_MASK_SIZE = (1024, 2048)         # base_loader.py:59: the drop mask is an array of this size, (H, W) ...
DROP_MASK_WINDOW = (14, 15, 2030, 840)   # ... that is 1 on rows 15..839 and columns 14..2029: (x0, y0, x1, y1)
MODES = {"original": 0, "current": 1}


def label_steps(id_to_trainid, boost=None):
    """The steps of the id -> trainId loop as bytes, n x (key, value, boosted), in the dict's own order
    (base_loader.py:177-183, uniform.py:114-121).  A key outside 0..255 matches no pixel of an 8-bit map and drops out
    (Cityscapes' -1), as in id2trainid_table.  boost: cfg.DROPOUT_COARSE_BOOST_CLASSES where the item's path turns the
    merge on, else None; a step is boosted when its VALUE, the train id, is in it."""
    out = bytearray()
    boost = None if boost is None else set(int(b) for b in boost)
    for k, v in (id_to_trainid or {}).items():
        k, v = int(k), int(v)
        if not 0 <= k <= 255:
            continue
        if not 0 <= v <= 255:
            raise ValueError("id_to_trainid maps %r to %r, which a uint8 label map cannot hold" % (k, v))
        out += bytes((k, v, 1 if boost is not None and v in boost else 0))
    return bytes(out)


def prob_cut(prob):
    """How many of the bytes 0..255 satisfy `b / 255.0 < prob` in float64 (base_loader.py:221-222): the compare is
    monotone in the byte, so the kernel tests `p < cut`.  0 .. 256."""
    if prob is None:
        raise ValueError("cfg.DATASET.CUSTOM_COARSE_PROB is None: an auto-labelled ('refinement') item needs the threshold")
    return int(np.count_nonzero(np.arange(256, dtype=np.uint8) / 255.0 < prob))


def coarse_path(label_fn):
    """The gtCoarse labelIds file of an auto-labelled item (base_loader.py:164-165, uniform.py:105-106)."""
    path = label_fn.replace(cfg.DATASET.CITYSCAPES_CUSTOMCOARSE, os.path.join(cfg.DATASET.CITYSCAPES_DIR, 'gtCoarse/gtCoarse'))
    return path.replace('leftImg8bit', 'gtCoarse_labelIds')


def decode_u8(path):
    from PIL import Image
    mask = np.array(Image.open(path))
    if mask.dtype != np.uint8 or mask.ndim != 2:
        raise ValueError("%s: a label map is one 8-bit channel, not %s %r" % (path, mask.dtype, mask.shape))
    return mask


def _rows(m, N, H, W):
    """(tensor, row stride) of a uint8 [N,H,W] tensor, read in place where its rows are dense and evenly spaced."""
    if H > 1 and W > 0 and m.stride(2) == 1 and m.stride(1) >= W and (N == 1 or m.stride(0) == H * m.stride(1)):
        return m, int(m.stride(1))
    return m.contiguous(), W


def prepare_labels(labels, coarse, prob, steps, mode, window=None, prob_cut=0, ignore_label=255):
    """labels, coarse, prob: uint8 device tensors [H,W] or [N,H,W] of one shape (rows may be strided); coarse may be None
    when no step is boosted, prob when prob_cut == 0.  steps: label_steps(...).  mode: "current" (the loader: every step
    compares against the map as rewritten so far) or "original" (the centroid pass: against the untouched map).  window:
    (x0, y0, x1, y1) of the drop mask -- labels outside it read as 0 -- or None.  Returns the uint8 label map of the same
    shape, dense.  Enqueues four launches on the current stream; nothing waits."""
    from .. import hip_backend as hb
    from .._lib import lib, check
    if mode not in MODES:
        raise ValueError("mode is 'current' or 'original', not %r" % (mode,))
    m = labels
    if m.dtype != torch.uint8 or m.dim() not in (2, 3):
        raise ValueError("label maps are uint8 tensors [H,W] or [N,H,W]")
    squeeze = m.dim() == 2
    N, H, W = (int(v) for v in ((1,) + tuple(m.shape) if squeeze else m.shape))
    steps = bytes(steps)
    if len(steps) % 3 or len(steps) > 3 * 256:
        raise ValueError("steps are up to 256 (key, value, boosted) byte triples")
    if coarse is None and any(steps[2::3]):
        raise ValueError("a boosted step needs the gtCoarse map")
    if prob is None and prob_cut:
        raise ValueError("a threshold needs the probability map")
    tensors, lds = [], []
    for t in (m, coarse, prob):
        if t is None:
            tensors.append(None)
            lds.append(0)
            continue
        if t.dtype != torch.uint8 or tuple(t.shape) != tuple(labels.shape) or t.device != labels.device:
            raise ValueError("labels, coarse and prob are uint8 tensors of one shape on one device")
        t, ld = _rows(t.unsqueeze(0) if squeeze else t, N, H, W)
        tensors.append(t)
        lds.append(ld)
    x0, y0, x1, y1 = (int(v) for v in window) if window is not None else (0, 0, 0, 0)
    out = torch.empty((N, H, W), dtype=torch.uint8, device=m.device)
    if out.numel():
        pairs = torch.empty((N, 2048), dtype=torch.int32, device=m.device)
        table = torch.empty((N, 65536), dtype=torch.uint8, device=m.device)
        check(lib().ssa_autolabel_u8(hb._p(tensors[0]), hb._p(tensors[1]), hb._p(tensors[2]), N, H, W, lds[0], lds[1], lds[2],
                                     steps, len(steps) // 3, MODES[mode], x0, y0, x1, y1, int(prob_cut), int(ignore_label),
                                     hb._p(pairs), hb._p(table), hb._p(out), W, hb._s()), "ssa_autolabel_u8")
    return out[0] if squeeze else out


class LabelPlan:
    """What the reference's loader does with the label of one item, decided from its path and cfg alone."""
    __slots__ = ("refinement", "boost", "coarse_fn", "prob_fn", "window", "prob_cut")

    def __repr__(self):
        return "LabelPlan(%s)" % ", ".join("%s=%r" % (k, getattr(self, k)) for k in self.__slots__)


def label_plan(mask_path):
    """The decisions of base_loader.py:162-183 and 206-223 for mask_path:
      refinement  'refinement' in the path: an auto-labelled item, thresholded by its `_prob.png`
      boost       cfg.DROPOUT_COARSE_BOOST_CLASSES where the merge with gtCoarse is on ('refinement' in the path, the set
                  is not None, 'vidseq' is not in the path), else None
      coarse_fn   the gtCoarse file when cfg.DATASET.CITYSCAPES_CUSTOMCOARSE is in the path, else None
      prob_fn, prob_cut   the probability map and the byte threshold of a refinement item, else (None, 0)
      window      the drop mask (MASK_OUT_CITYSCAPES, CUSTOM_COARSE_PROB not None, a refinement item), else None"""
    if not mask_path:
        raise ValueError("an item without a label file has no label to prepare")
    d = cfg.DATASET
    p = LabelPlan()
    p.refinement = 'refinement' in mask_path
    on = p.refinement and cfg.DROPOUT_COARSE_BOOST_CLASSES is not None and 'vidseq' not in mask_path
    p.boost = list(cfg.DROPOUT_COARSE_BOOST_CLASSES) if on else None
    p.coarse_fn = coarse_path(mask_path) if d.CITYSCAPES_CUSTOMCOARSE in mask_path else None
    p.window = DROP_MASK_WINDOW if (d.MASK_OUT_CITYSCAPES and d.CUSTOM_COARSE_PROB is not None and p.refinement) else None
    p.prob_fn = mask_path.replace('.png', '_prob.png') if p.refinement else None
    p.prob_cut = prob_cut(d.CUSTOM_COARSE_PROB) if p.refinement else 0
    return p


def read_labels(mask_path, id_to_trainid):
    """The label map of BaseLoader.__getitem__ before the joint transforms (read_images' id -> trainId loop, drop mask and
    gtCoarse merge, then the probability threshold), as the uint8 device tensor [H,W] RandomSizeAndCrop.apply takes.
    The one to three PNGs are decoded on the host; a label that is not auto-labelled goes through the same call with
    no boosted step.  Where the reference fails with a NameError (a boosted class without a gtCoarse file to merge)
    or a TypeError (a refinement item without CUSTOM_COARSE_PROB), or multiplies by its 1024 x 2048 drop mask an image
    of another size, this raises ValueError."""
    plan = label_plan(mask_path)
    steps = label_steps(id_to_trainid, plan.boost)
    boosted = any(steps[2::3])
    if boosted and plan.coarse_fn is None:
        raise ValueError("%s: a boosted class of an auto-labelled item needs its gtCoarse map, and the path does not contain "
                         "cfg.DATASET.CITYSCAPES_CUSTOMCOARSE (%s)" % (mask_path, cfg.DATASET.CITYSCAPES_CUSTOMCOARSE))
    mask = decode_u8(mask_path)
    if plan.window is not None and mask.shape != DROP_MASK_SIZE:
        raise ValueError("%s: the drop mask of MASK_OUT_CITYSCAPES is %d x %d, the label map %d x %d"
                         % ((mask_path,) + DROP_MASK_SIZE + mask.shape))
    maps = [mask, decode_u8(plan.coarse_fn) if boosted else None, decode_u8(plan.prob_fn) if plan.refinement else None]
    for fn, other in zip((plan.coarse_fn, plan.prob_fn), maps[1:]):
        if other is not None and other.shape != mask.shape:
            raise ValueError("%s is %r, the label map %r" % (fn, other.shape, mask.shape))
    dev = [None if a is None else torch.from_numpy(a).to(DEVICE) for a in maps]
    return prepare_labels(dev[0], dev[1], dev[2], steps, "current", window=plan.window, prob_cut=plan.prob_cut,
                          ignore_label=cfg.DATASET.IGNORE_LABEL)
