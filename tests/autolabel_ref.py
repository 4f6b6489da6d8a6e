"""NumPy restatement of the label half of the auto-labelled coarse data path (TEST REFERENCE; imports nothing of the
product): the sequential whole-array assignments of BaseLoader.read_images / __getitem__ (datasets/base_loader.py:152-229)
and of class_centroids_image (datasets/uniform.py:104-121), one pass per step -- NOT the pair table csrc/autolabel.hip
builds.  tests/test_autolabel_cpu.py pins it to the real reference's output (tests/golden/autolabel_golden.json); the
kernels are then held to it bit for bit."""
import numpy as np

DROP_WINDOW = (14, 15, 2030, 840)           # base_loader.py:59-60: drop_mask[15:840, 14:2030] = 1, as (x0, y0, x1, y1)
DROP_SIZE = (1024, 2048)


def merge(o, g, p, steps, mode, window=None, cut=0, ignore=255):
    """What ssa_autolabel_u8 is specified to compute for ONE image.  o, g, p: uint8 [H, W] (g, p may be None);
    steps: [(key, value, boosted), ...]; mode "current" | "original"; window (x0, y0, x1, y1) or None; cut 0..256."""
    mask = np.array(o, dtype=np.uint8)
    if window is not None and window[2] > window[0] and window[3] > window[1]:
        keep = np.zeros(mask.shape, dtype=bool)
        keep[window[1]:window[3], window[0]:window[2]] = True
        mask[~keep] = 0
    untouched = mask.copy()
    for k, v, boosted in steps:
        hit = (mask == k) if mode == "current" else (untouched == k)
        if boosted and hit.sum() > 0:
            hit = hit | (g == k)
        mask[hit] = v
    if cut:
        mask[p.astype(np.int64) < cut] = ignore
    return mask


def merge_batch(o, g, p, steps, mode, window=None, cut=0, ignore=255):
    return np.stack([merge(o[i], None if g is None else g[i], None if p is None else p[i], steps, mode, window, cut, ignore)
                     for i in range(len(o))])


def loader_labels(mask_path, o, g, p, id_to_trainid, customcoarse, boost, mask_out_cityscapes, prob, ignore=255):
    """The label BaseLoader.__getitem__ hands to the transforms, statement by statement (float64 compare of the
    probability included).  g is read only where `customcoarse in mask_path`, p only for a refinement item."""
    refinement = 'refinement' in mask_path
    mask = np.array(o)
    if mask_out_cityscapes and prob is not None and refinement:
        drop = np.zeros(DROP_SIZE)
        drop[DROP_WINDOW[1]:DROP_WINDOW[3], DROP_WINDOW[0]:DROP_WINDOW[2]] = 1.0
        mask = drop * mask
    mask = mask.copy()
    have_coarse = customcoarse in mask_path
    for k, v in id_to_trainid.items():
        hit = (mask == k)
        if refinement and boost is not None and v in boost and hit.sum() > 0 and 'vidseq' not in mask_path:
            assert have_coarse, "the reference has no gtCoarse here (NameError)"
            hit = hit | (g == k)
        mask[hit] = v
    mask = mask.astype(np.uint8)
    if refinement:
        mask[(p / 255.0) < prob] = ignore
    return mask


def centroid_labels(label_fn, o, g, id2trainid, customcoarse, boost):
    """The map class_centroids_image takes its centroids from (uniform.py:112-121): hits against the untouched copy."""
    mask = np.array(o)
    untouched = mask.copy()
    if id2trainid:
        for k, v in id2trainid.items():
            hit = (untouched == k)
            if 'refinement' in label_fn and boost is not None and v in boost and hit.sum() > 0:
                assert customcoarse in label_fn, "the reference has no gtCoarse here (NameError)"
                hit = hit | (g == k)
            mask[hit] = v
    return mask


def plain_table(o, id_to_trainid):
    """What a plain id -> trainId table makes of the map: what the tests must be able to tell from the real thing."""
    lut = np.arange(256, dtype=np.uint8)
    for k, v in id_to_trainid.items():
        if 0 <= k <= 255:
            lut[k] = v
    return lut[o]
