"""Cases of the auto-labelled coarse data path tests (tests/test_autolabel_*.py) and of
tests/golden/make_golden_autolabel.py: maps regenerated from seeds (the golden file stores results, not pixels).  Nothing
here imports the product.

Two kinds of cases:
  KERNEL   inputs of ssa_autolabel_u8 / prepare_labels: the smallest shapes at which the kernels of csrc/autolabel.hip can
           go wrong.  A thread reads 16 labels at a time, so widths that are no multiple of 16 and a row stride of W + 5,
           on each array on its own, give partial chunks at both row ends and every load width; the presence bits are per
           image and per step; the window and the threshold have their own edges.  No launch caps its grid, so there is
           no case past a cap.
  ITEMS    items of the loader and of the centroid pass as files on disk, with the cfg state they are read under: what the
           golden holds the REAL reference's output for."""
import zlib

import numpy as np

# Cityscapes' id -> trainId (datasets/cityscapes_labels.py) without the key -1, in the dict's order; the golden records
# the one the reference used and tests/test_autolabel_cpu.py compares
CITY = {0: 255, 1: 255, 2: 255, 3: 255, 4: 255, 5: 255, 6: 255, 7: 0, 8: 1, 9: 255, 10: 255, 11: 2, 12: 3, 13: 4, 14: 255,
        15: 255, 16: 255, 17: 5, 18: 255, 19: 6, 20: 7, 21: 8, 22: 9, 23: 10, 24: 11, 25: 12, 26: 13, 27: 14, 28: 15, 29: 255,
        30: 255, 31: 16, 32: 17, 33: 18}
CITY_BOOST = [14, 15, 16]
CITY_IDS = [0, 7, 8, 11, 24, 26, 27, 28, 31, 33, 40]
# values that are later keys: in mode "current" a pixel walks the chain, in mode "original" it takes one step
CHAIN = {1: 2, 2: 3, 3: 1, 9: 2}
CHAIN_PERM = {3: 1, 9: 2, 2: 3, 1: 2}
CHAIN_BOOST = [3]                        # the step 2 -> 3, in the middle of both orders
CHAIN_IDS = [0, 1, 2, 3, 9, 5]
# 5 becomes 6 at the first step: in mode "current" the boosted id 6 is present at its own step only through that
VIA_EARLIER = {5: 6, 6: 7}
VIA_BOOST = [7]
# all 256 keys, a permutation of the order, values that collide with later keys, every 5th step boosted
ALL256 = {int(k): int((7 * k + 3) % 256) for k in np.random.RandomState(256).permutation(256)}
ALL256_BOOST = sorted({v for i, v in enumerate(ALL256.values()) if i % 5 == 0})


def steps_of(id_to_trainid, boost=None):
    """[(key, value, boosted), ...] in the dict's order, keys outside 0..255 dropped (the rule of label_steps)."""
    return [(int(k), int(v), int(boost is not None and v in boost)) for k, v in id_to_trainid.items() if 0 <= int(k) <= 255]


def blocky(rng, H, W, values, block):
    """Random rectangles of `block` pixels, every one of a value of `values`: long runs, as a label map has."""
    by, bx = (H + block - 1) // block, (W + block - 1) // block
    grid = np.asarray(values, dtype=np.uint8)[rng.randint(0, len(values), (by, bx))]
    return np.ascontiguousarray(np.repeat(np.repeat(grid, block, 0), block, 1)[:H, :W])


def _rng(name):
    return np.random.RandomState(zlib.crc32(name.encode()) & 0x7fffffff)


def prob_bytes(rng, H, W, cut):
    """Probability bytes around a threshold: cut - 1 and cut themselves, the ends of the range, and others."""
    values = sorted({max(cut - 1, 0), min(cut, 255), 0, 255, 77, 200})
    return blocky(rng, H, W, values, 3)


# name -> dict(N, H, W, ids, block, steps, mode, window, cut, ignore, extra, coarse, special)
#   extra: additional row stride of (labels, coarse, prob, out); coarse: whether the gtCoarse map is given; special: what
#   inputs() arranges in the maps for a presence-gate case
def _case(N, H, W, ids, block, steps, mode, window=None, cut=0, ignore=255, extra=(0, 0, 0, 0), coarse=True, special=None):
    return dict(N=N, H=H, W=W, ids=ids, block=block, steps=steps, mode=mode, window=window, cut=cut, ignore=ignore, extra=extra,
                coarse=coarse, special=special)


KERNEL = {}
_CHAIN_STEPS = steps_of(CHAIN, CHAIN_BOOST)
_CITY_STEPS = steps_of(CITY, CITY_BOOST)
# unaligned 16-byte chunks at both row ends, each array on its own and all together; a window off the 16-grid; a threshold
for _tag, _extra in (("l", (5, 0, 0, 0)), ("c", (0, 5, 0, 0)), ("p", (0, 0, 5, 0)), ("o", (0, 0, 0, 5)), ("all", (5, 5, 5, 5))):
    KERNEL["3x37_ld_" + _tag] = _case(2, 3, 37, CHAIN_IDS, 2, _CHAIN_STEPS, "current", (3, 1, 30, 3), 128, 250, _extra)
    KERNEL["64x80_ld_" + _tag] = _case(1, 64, 80, CITY_IDS, 5, _CITY_STEPS, "current", (17, 9, 71, 50), 128, 255, _extra)
KERNEL["h1"] = _case(1, 1, 53, CHAIN_IDS, 3, _CHAIN_STEPS, "current", None, 128)
KERNEL["h1_ld"] = _case(2, 1, 53, CHAIN_IDS, 3, _CHAIN_STEPS, "original", None, 0, 255, (5, 5, 0, 5))
for _mode in ("current", "original"):
    KERNEL["city_" + _mode] = _case(2, 37, 53, CITY_IDS, 4, _CITY_STEPS, _mode)
    KERNEL["chain_" + _mode] = _case(1, 37, 53, CHAIN_IDS, 4, _CHAIN_STEPS, _mode)
    KERNEL["chain_perm_" + _mode] = _case(1, 37, 53, CHAIN_IDS, 4, steps_of(CHAIN_PERM, CHAIN_BOOST), _mode)
    # presence gates
    KERNEL["only_in_g_" + _mode] = _case(1, 19, 29, CITY_IDS, 3, _CITY_STEPS, _mode, special="only_in_g")
    KERNEL["via_earlier_" + _mode] = _case(1, 19, 29, [0, 5, 9], 3, steps_of(VIA_EARLIER, VIA_BOOST), _mode, special="via_earlier")
    KERNEL["n3_one_image_" + _mode] = _case(3, 19, 29, CITY_IDS, 3, _CITY_STEPS, _mode, special="one_image")
    KERNEL["all256_" + _mode] = _case(1, 64, 80, list(range(256)), 2, steps_of(ALL256, ALL256_BOOST), _mode)
    KERNEL["no_steps_" + _mode] = _case(1, 19, 29, list(range(256)), 2, [], _mode, (2, 2, 20, 11), 77, 9, coarse=False)
KERNEL["in_dropped"] = _case(1, 37, 53, CITY_IDS, 4, _CITY_STEPS, "current", (5, 6, 40, 30), special="in_dropped")
KERNEL["window_1px"] = _case(1, 19, 29, CITY_IDS, 3, _CITY_STEPS, "current", (13, 7, 14, 8))
KERNEL["window_1px_corner"] = _case(1, 19, 29, CITY_IDS, 3, _CITY_STEPS, "current", (28, 18, 29, 19))
KERNEL["window_whole"] = _case(1, 19, 29, CITY_IDS, 3, _CITY_STEPS, "current", (0, 0, 29, 19))
KERNEL["no_coarse"] = _case(1, 19, 29, CITY_IDS, 3, steps_of(CITY), "current", coarse=False)
for _cut in (0, 1, 128, 255, 256):
    KERNEL["cut_%d" % _cut] = _case(1, 19, 45, CITY_IDS, 3, _CITY_STEPS, "current", None, _cut, 255)
# more than one band of rows per image and more than one workgroup of chunks: 300 rows of 96
KERNEL["bands"] = _case(2, 300, 96, CITY_IDS, 11, _CITY_STEPS, "current", (14, 15, 90, 250), 128)

_INPUTS = {}


def inputs(name):
    """(labels, coarse, prob) uint8 [N, H, W] of a kernel case (cached; treat as read-only)."""
    if name not in _INPUTS:
        c = KERNEL[name]
        rng = _rng(name)
        N, H, W = c["N"], c["H"], c["W"]
        o = np.stack([blocky(rng, H, W, c["ids"], c["block"]) for _ in range(N)])
        g = np.stack([blocky(rng, H, W, c["ids"], c["block"] + 1) for _ in range(N)])
        p = np.stack([prob_bytes(rng, H, W, c["cut"]) for _ in range(N)])
        sp = c["special"]
        if sp == "only_in_g":                       # the boosted id 27 is in g alone: nothing of g may arrive
            o[o == 27] = 26
            g[:, 2:9, 3:17] = 27
        elif sp == "via_earlier":                   # no 6 in o; 5 becomes 6 at the first step; g has 6 where o has 0 and 9
            g[:] = 0
            g[:, 4:15, 6:20] = 6
            assert (o == 5).any() and not (o == 6).any()
        elif sp == "one_image":                     # image 1 alone has the boosted id 28; g has it everywhere
            o[o == 28] = 26
            o[1, 5:9, 5:9] = 28
            g[:, 10:16, 2:25] = 28
        elif sp == "in_dropped":                    # the boosted id 31 only outside the window: absent after the drop mask
            o[o == 31] = 26
            o[0, 0:5, :] = 31
            o[0, :, 45:] = 31
            g[0, 10:20, 10:30] = 31
        for a in (o, g, p):
            a.setflags(write=False)
        _INPUTS[name] = (o, g, p)
    return _INPUTS[name]


# ---- items on disk.  The tree: <CUSTOMCOARSE>/... holds the auto labels and their _prob.png, <CITYSCAPES_DIR>/gtCoarse/
# gtCoarse/... the gtCoarse maps, plain/ ordinary labels.  Relative names: the tests and the golden maker chdir.
CUSTOMCOARSE, CITYSCAPES_DIR = "ccroot", "csroot"
# name -> (label path, (H, W), id map name, settings: boost set, mask_out, prob)
ITEMS = {
    "refine": ("ccroot/refinement/aachen/a_leftImg8bit.png", (37, 53), "CITY", dict(boost=CITY_BOOST, mask_out=False, prob=0.5)),
    "refine_vidseq": ("ccroot/refinement/vidseq/b_leftImg8bit.png", (37, 53), "CITY", dict(boost=CITY_BOOST, mask_out=False, prob=0.5)),
    "refine_no_boost": ("ccroot/refinement/aachen/c_leftImg8bit.png", (37, 53), "CITY", dict(boost=None, mask_out=False, prob=0.5)),
    "plain": ("plain/d_labelIds.png", (37, 53), "CITY", dict(boost=CITY_BOOST, mask_out=True, prob=0.5)),
    "coarse_not_refined": ("ccroot/other/e_leftImg8bit.png", (19, 29), "CITY", dict(boost=CITY_BOOST, mask_out=True, prob=0.5)),
    "refine_small": ("ccroot/refinement/bonn/f_leftImg8bit.png", (19, 29), "CITY", dict(boost=CITY_BOOST, mask_out=False, prob=0.5)),
    "plain_small": ("plain/g_labelIds.png", (19, 29), "CITY", dict(boost=CITY_BOOST, mask_out=False, prob=None)),
    "chain": ("ccroot/refinement/h_leftImg8bit.png", (19, 29), "CHAIN", dict(boost=CHAIN_BOOST, mask_out=False, prob=0.5)),
    "chain_perm": ("ccroot/refinement/h_leftImg8bit.png", (19, 29), "CHAIN_PERM", dict(boost=CHAIN_BOOST, mask_out=False, prob=0.5)),
    "prob_one": ("ccroot/refinement/i_leftImg8bit.png", (19, 29), "CITY", dict(boost=CITY_BOOST, mask_out=False, prob=1.0)),
    "prob_tiny": ("ccroot/refinement/j_leftImg8bit.png", (19, 29), "CITY", dict(boost=CITY_BOOST, mask_out=False, prob=0.001)),
    "mapillary": ("plain/k_labelIds.png", (19, 29), "EMPTY", dict(boost=None, mask_out=False, prob=None)),
    # the reference's own window on the reference's own size
    "full": ("ccroot/refinement/l_leftImg8bit.png", (1024, 2048), "CITY", dict(boost=CITY_BOOST, mask_out=True, prob=0.5)),
}
ID_MAPS = {"CITY": CITY, "CHAIN": CHAIN, "CHAIN_PERM": CHAIN_PERM, "EMPTY": {}}
# the mixed list of the centroid pass: auto-labelled and plain items of two sizes, in this order, CITY ids
CENTROID_LIST = ("refine", "plain", "refine_vidseq", "refine_small", "plain_small", "refine_no_boost", "coarse_not_refined")
CENTROID_TILE, CENTROID_CLASSES = 16, 19
CENTROID_CHAIN = ("chain",)                # and, with CHAIN ids, the chain item alone

_MAPS = {}


def item_maps(name):
    """(labels, gtCoarse, prob) uint8 [H, W] of an item (cached; read-only).  chain_perm is the chain item's files."""
    key = "chain" if name == "chain_perm" else name
    if key not in _MAPS:
        path, (H, W), ids, st = ITEMS[key]
        rng = _rng("item_" + key)
        values = CHAIN_IDS if ids.startswith("CHAIN") else CITY_IDS
        block = 37 if key == "full" else 4
        o, g = blocky(rng, H, W, values, block), blocky(rng, H, W, values, block + 1)
        if key == "full":                           # specks, and a boosted id that the drop mask removes altogether
            o[rng.randint(0, H, 300), rng.randint(0, W, 300)] = 27
            o[o == 31] = 33
            o[900:, :200] = 31
            g[rng.randint(0, H, 300), rng.randint(0, W, 300)] = 28
        p = blocky(rng, H, W, [0, 1, 2, 126, 127, 128, 129, 200, 254, 255], block)
        for a in (o, g, p):
            a.setflags(write=False)
        _MAPS[key] = (o, g, p)
    return _MAPS[key]


def coarse_name(path):
    return path.replace(CUSTOMCOARSE, CITYSCAPES_DIR + "/gtCoarse/gtCoarse").replace("leftImg8bit", "gtCoarse_labelIds")


def write_tree(names=None):
    """Write the items' PNGs under the current directory; returns {name: (image path, label path)}."""
    import os
    from PIL import Image
    out = {}
    for name in (names or ITEMS):
        path = ITEMS[name][0]
        o, g, p = item_maps(name)
        files = [(path, o)]
        if CUSTOMCOARSE in path:
            files.append((coarse_name(path), g))
        if "refinement" in path:
            files.append((path.replace(".png", "_prob.png"), p))
        for fn, a in files:
            os.makedirs(os.path.dirname(fn), exist_ok=True)
            if not os.path.exists(fn):
                Image.fromarray(np.asarray(a)).save(fn)
        img = os.path.join(os.path.dirname(path), "img_" + os.path.basename(path))
        if not os.path.exists(img):
            Image.new("RGB", (2, 2)).save(img)       # the loader opens the image; the label does not depend on it
        out[name] = (img, path)
    return out
