"""NumPy restatement of the class-uniform centroid pass and of the constant padding (TEST REFERENCE; imports nothing of
the product).  Integer sums and floor division, what csrc/centroids.hip computes; tests/test_uniform_cpu.py pins it to
the golden data of the real reference (datasets/uniform.py:84-135) and to live scipy.ndimage.center_of_mass."""
from collections import defaultdict

import numpy as np


def lut_of(id2trainid):
    """uniform.py:112-121 as a table: the step compares against an untouched copy of the mask."""
    lut = np.arange(256, dtype=np.uint8)
    for k, v in (id2trainid or {}).items():
        if 0 <= k <= 255:
            lut[k] = v
    return lut


def tile_locations(tile, H, W):
    return [(x * tile, y * tile) for y in range(H // tile) for x in range(W // tile)]


def centroid_table(mask, tile, C, id2trainid=None):
    """mask uint8 [H, W] -> (sums uint64 [tiles, C, 3] = (n, sum x, sum y) tile-local, centroids int32 [tiles, C, 2])."""
    H, W = mask.shape
    m = lut_of(id2trainid)[mask]
    locs = tile_locations(tile, H, W)
    sums = np.zeros((len(locs), C, 3), dtype=np.uint64)
    cent = np.full((len(locs), C, 2), -1, dtype=np.int32)
    ar = np.arange(tile, dtype=np.int64)
    for t, (x_offs, y_offs) in enumerate(locs):
        patch = m[y_offs:y_offs + tile, x_offs:x_offs + tile]
        for c in np.unique(patch).tolist():
            if c >= C:
                continue
            hit = patch == c
            n = int(hit.sum())
            sx = int((hit.sum(0).astype(np.int64) * ar).sum())
            sy = int((hit.sum(1).astype(np.int64) * ar).sum())
            sums[t, c] = (n, sx, sy)
            cent[t, c] = (sx // n + x_offs, sy // n + y_offs)
    return sums, cent


def as_dict(item, cent):
    """The reference's per-image dict from a centroid table: tiles outside, classes inside (uniform.py:123-133)."""
    image_fn, label_fn = item
    out = defaultdict(list)
    for t in range(cent.shape[0]):
        for c in range(cent.shape[1]):
            if cent[t, c, 0] >= 0:
                out[c].append((image_fn, label_fn, (int(cent[t, c, 0]), int(cent[t, c, 1])), c))
    return out


def merged(dicts):
    """uniform.py:160-164: the per-image dicts merged in item order."""
    out = defaultdict(list)
    for d in dicts:
        for c in d:
            out[c].extend(d[c])
    return out


def pad(src, lrtb, fill):
    """ImageOps.expand / add_margin for uint8 [H, W] or [H, W, 3]; lrtb = (left, top, right, bottom)."""
    left, top, right, bottom = lrtb
    H, W = src.shape[:2]
    out = np.empty((H + top + bottom, W + left + right) + src.shape[2:], dtype=np.uint8)
    out[...] = np.asarray(fill, dtype=np.uint8)
    out[top:top + H, left:left + W] = src
    return out
