"""Cases of the class-uniform sampling tests (tests/test_uniform_*.py) and of tests/golden/make_golden_uniform.py: label
maps regenerated from seeds (the golden file stores results, not pixels), the inputs of build_epoch, the draws of
RandomSizeAndCrop and the small pairs whose padded and cropped bytes the golden holds.  Nothing here imports the product.

The centroid cases are the smallest shapes at which the kernel of csrc/centroids.hip can go wrong: a thread reads 16
labels at a time from 16-byte aligned addresses, so widths that are no multiple of 16 and a row stride of W + 5 give
partial chunks at both ends of a row; 2 x 3 tiles plus a remainder in both directions exercise the tile walk."""
import hashlib
import zlib

import numpy as np

CITY_LIKE = {-1: 255, 0: 255, 1: 255, 2: 255, 3: 255, 4: 255, 5: 255, 6: 255, 7: 0, 8: 1, 9: 255, 10: 255, 11: 2, 12: 3,
             13: 4, 14: 255, 15: 255, 16: 255, 17: 5, 18: 255, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13,
             27: 14, 28: 15, 29: 255, 30: 255, 31: 16, 32: 17, 33: 18}
TWO_ONTO_ONE = {0: 255, 1: 4, 2: 4, 3: 0, 4: 1, 5: 2, 6: 3, 7: 18, 8: 18, 9: 19, 200: 5, -1: 255, 300: 7}


def _blocky(rng, H, W, values, block):
    """Random rectangles of `block` pixels, every one of a value of `values`: long runs, as a label map has."""
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    grid = np.asarray(values, dtype=np.uint8)[rng.randint(0, len(values), (by, bx))]
    return np.ascontiguousarray(np.repeat(np.repeat(grid, block, 0), block, 1)[:H, :W])


def _single_pixels(H, W, tile):
    """Class 1 only at every tile's (0, 0), class 2 only at every tile's (T-1, T-1); the rest is ignore."""
    m = np.full((H, W), 255, dtype=np.uint8)
    m[0:(H // tile) * tile:tile, 0:(W // tile) * tile:tile] = 1
    m[tile - 1:(H // tile) * tile:tile, tile - 1:(W // tile) * tile:tile] = 2
    return m


def _straddle(H, W, tile):
    """A rectangle of class 3 across the corner shared by four tiles, one of class 5 across a vertical edge only."""
    m = np.full((H, W), 255, dtype=np.uint8)
    m[tile - 3:tile + 5, tile - 7:tile + 2] = 3
    m[2:6, 2 * tile - 1:2 * tile + 1] = 5
    return m


def _alternating(H, W):
    return np.ascontiguousarray(np.broadcast_to((np.arange(W) % 2 * 3 + 1).astype(np.uint8), (H, W)))     # 1, 4, 1, 4


def _bands(H, W):
    return np.ascontiguousarray(np.broadcast_to(((np.arange(H) // 3) % 5).astype(np.uint8)[:, None], (H, W)))


def _checker(H, W):
    return (((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2) * 7).astype(np.uint8)                  # 0 and 7


# name -> (N, H, W, tile, C, id2trainid or None, extra row stride, content)
CASES = {
    "t8_blocky": (1, 19, 29, 8, 19, None, 0, "blocky19"),
    "t16_lut_n3": (3, 37, 53, 16, 19, TWO_ONTO_ONE, 0, "blocky_raw"),
    "t64_c65": (1, 135, 203, 64, 65, None, 0, "blocky65"),
    "t16_ld": (3, 37, 53, 16, 19, None, 5, "blocky19"),
    "no_tiles": (1, 10, 53, 16, 19, None, 0, "blocky19"),
    "pixels": (1, 37, 53, 16, 19, None, 0, "pixels"),
    "straddle": (1, 37, 53, 16, 19, None, 0, "straddle"),
    "alternating": (1, 37, 53, 16, 19, None, 0, "alternating"),
    "alternating_t64": (1, 70, 150, 64, 19, None, 3, "alternating"),
    "bands": (1, 37, 53, 16, 19, None, 0, "bands"),
    "checker": (1, 19, 29, 8, 19, None, 0, "checker"),
    "c1": (1, 37, 53, 16, 1, None, 0, "blocky_small"),
    "c256": (1, 37, 53, 16, 256, None, 0, "blocky_bytes"),
    "c256_lut": (1, 19, 29, 8, 256, TWO_ONTO_ONE, 0, "blocky_bytes"),
    "full2048": (1, 2048, 2048, 2048, 19, None, 0, "full"),            # sum_x = 2048 * (2047 * 2048 / 2) = 2^32 - 2^21
    "full4096": (1, 4096, 4096, 4096, 19, None, 0, "full"),            # sum_x = 4096 * (4095 * 4096 / 2) > 2^35
    "workload": (1, 1024, 2048, 1024, 19, CITY_LIKE, 0, "city"),       # the workload's own shape, Cityscapes ids
}
SMALL = tuple(k for k in CASES if k not in ("full2048", "full4096", "workload"))

_MAPS = {}


def label_maps(name):
    """uint8 [N, H, W] of a case (cached; treat as read-only)."""
    if name not in _MAPS:
        N, H, W, tile, C, _, _, content = CASES[name]
        rng = np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)
        maps = []
        for _ in range(N):
            if content == "blocky19":
                m = _blocky(rng, H, W, list(range(19)) + [255, 19, 40], 5)
            elif content == "blocky_raw":
                m = _blocky(rng, H, W, list(range(12)) + [200, 255], 4)
            elif content == "blocky65":
                m = _blocky(rng, H, W, list(range(65)) + [65, 66, 255], 9)
            elif content == "blocky_small":
                m = _blocky(rng, H, W, [0, 0, 1, 2, 255], 6)
            elif content == "blocky_bytes":
                m = _blocky(rng, H, W, list(range(256)), 3)
            elif content == "city":
                m = _blocky(rng, H, W, list(range(34)), 37)
                m[rng.randint(0, H, 200), rng.randint(0, W, 200)] = 26      # specks: classes of a few pixels
            elif content == "pixels":
                m = _single_pixels(H, W, tile)
            elif content == "straddle":
                m = _straddle(H, W, tile)
            elif content == "alternating":
                m = _alternating(H, W)
            elif content == "bands":
                m = _bands(H, W)
            elif content == "checker":
                m = _checker(H, W)
            elif content == "full":
                m = np.full((H, W), 5, dtype=np.uint8)
            else:
                raise KeyError(content)
            maps.append(m)
        _MAPS[name] = np.stack(maps)
        _MAPS[name].setflags(write=False)
    return _MAPS[name]


def file_names(name, i):
    """The fixed relative names under which image i of a case is known to the reference and to the tests."""
    return ("%s_%d_leftImg8bit.png" % (name, i), "%s_%d_labelIds.png" % (name, i))


# the maps whose centroid dicts and build_centroids JSON the golden holds as text (written as PNGs, in this order)
JSON_SET = ("t16_lut_n3", "t8_blocky", "pixels")
JSON_CLASSES, JSON_TILE = 19, 1024          # build_centroids always runs at tile 1024: these small maps have no tile ...
JSON_BIG = ("json_big", 1030, 1100)         # ... so one map a little larger than a tile joins them


def json_big_map():
    rng = np.random.RandomState(77)
    m = _blocky(rng, JSON_BIG[1], JSON_BIG[2], list(range(12)) + [200, 255], 97)
    m.setflags(write=False)
    return m


# ---- build_epoch: (seed, number of items, class_uniform_pct, bias or None, train)
EPOCHS = [(0, 40, 0.5, None, True), (1, 57, 0.5, None, True), (2, 23, 0.3, None, True), (3, 40, 1.0, None, True),
          (4, 64, 0.5, [1.0, 2.5, 0.0, 1.5, 0.49, 3.0, 1.0], True), (5, 40, 0.5, None, False), (6, 40, 0, None, True)]
EPOCH_CLASSES = 7


def epoch_inputs(n_items):
    """imgs and a centroid table over EPOCH_CLASSES classes: class 2 has no centroid, class 5 a single one."""
    imgs = [("img_%03d.png" % i, "lab_%03d.png" % i) for i in range(n_items)]
    lens = [5, 11, 0, 3, 8, 1, 30]
    centroids = {c: [("img_%03d.png" % ((7 * k + c) % n_items), "lab_%03d.png" % ((7 * k + c) % n_items),
                      (13 * k + c, 5 * k + 2 * c), c) for k in range(lens[c])] for c in range(EPOCH_CLASSES)}
    return imgs, centroids


def np_state_digest():
    st = np.random.get_state()
    return hashlib.sha256(st[1].tobytes() + repr(st[2:]).encode()).hexdigest()[:16]


def py_state_digest():
    import random
    return hashlib.sha256(repr(random.getstate()).encode()).hexdigest()[:16]


# ---- RandomSizeAndCrop plans: (seed, crop_size, nopad, scale_min, scale_max, full_size, pre_size, translate_aug_fix,
#                                (w, h), centroid)
PLANS = [
    (0, (32, 48), False, 0.5, 2.0, False, None, False, (80, 60), None),          # pads at small scales, crops at large
    (1, (32, 48), False, 0.5, 2.0, False, None, False, (80, 60), None),
    (2, (32, 48), False, 0.5, 2.0, False, None, False, (80, 60), (70, 11)),      # centroid
    (3, (32, 48), False, 0.5, 2.0, False, None, False, (80, 60), (3, 55)),
    (4, (32, 48), False, 0.3, 0.5, False, None, False, (80, 60), (40, 30)),      # always padded, with a centroid
    (5, (32, 48), False, 0.3, 0.5, False, None, False, (80, 60), None),
    (6, (32, 48), True, 0.3, 0.5, False, None, False, (80, 60), None),           # nopad: the crop shrinks
    (7, (32, 48), True, 0.3, 0.5, False, None, False, (80, 60), (10, 50)),
    (8, 40, True, 0.5, 2.0, False, None, False, (80, 60), None),
    (9, (30, 40), False, 1.0, 1.0, False, None, False, (40, 30), None),          # resized == crop: no draw after the scale
    (10, (30, 40), False, 1.0, 1.0, False, None, False, (40, 30), (5, 5)),
    (11, (30, 64), False, 1.0, 1.0, False, None, False, (40, 30), None),         # one axis fits: no draw on it, pad on x
    (12, (64, 40), False, 1.0, 1.0, False, None, False, (40, 30), None),
    (13, (32, 48), False, 0.5, 2.0, True, None, False, (80, 60), None),          # full_size: the crop is the input size
    (14, (32, 48), False, 0.5, 2.0, True, None, False, (80, 60), (22, 33)),
    (15, (32, 48), False, 0.5, 2.0, False, 50, False, (80, 60), None),           # pre_size, wide
    (16, (32, 48), False, 0.5, 2.0, False, 50, False, (60, 80), (30, 70)),       # pre_size, tall
    (17, (32, 48), False, 0.3, 0.5, False, None, True, (80, 60), None),          # TRANSLATE_AUG_FIX: image slides in crop
    (18, (32, 48), False, 0.3, 0.5, False, None, True, (80, 60), (40, 30)),
    (19, (32, 48), False, 1.0, 2.0, False, None, True, (80, 60), None),          # TRANSLATE_AUG_FIX, image >= crop
    (20, (32, 48), False, 1.0, 2.0, False, None, True, (80, 60), (79, 59)),
    (21, (32, 48), True, 0.5, 2.0, False, None, False, (80, 60), (0, 0)),
]
PLAN_REPEATS = 6        # draws per entry from one seeded generator: the later ones start from the state the earlier left


# ---- pairs whose bytes the golden holds: (seed, crop_size, scale range, translate_aug_fix, (w, h), centroid)
PAIRS = [(0, (24, 32), (0.4, 0.6), False, (40, 30), None),           # padded by a border
         (1, (24, 32), (1.2, 1.6), False, (40, 30), (35, 4)),        # not padded
         (2, (24, 32), (0.4, 0.6), True, (40, 30), None),            # padded by margins
         (3, (24, 32), (0.4, 0.6), False, (40, 30), (20, 15))]       # padded, with a centroid


def pair(seed, size):
    """A small RGB image and its label map, uint8."""
    rng = np.random.RandomState(1000 + seed)
    w, h = size
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    lab = _blocky(rng, h, w, list(range(19)) + [255], 4)
    return img, lab
