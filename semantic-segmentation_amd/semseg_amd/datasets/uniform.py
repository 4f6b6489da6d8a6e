"""Class-uniform sampling (--class_uniform_pct, train.py:78; datasets/uniform.py of the reference, name for name).

Every image is divided into tiles; for each tile and each class present in it the centroid of the class's pixels is
recorded, and half of every epoch's items (cfg.DATASET.CLASS_UNIFORM_PCT) are (image, label, centroid, class_id) tuples
drawn per class, around which the first joint transform places its crop (datasets/base_loader.py:129-132).

The centroid pass runs on the device (csrc/centroids.hip, ssa_class_centroids_u8): one integer pass per label map
instead of the reference's pass per (tile, class), exact to `int(center_of_mass(...))`.  The label PNGs are decoded on
host threads, maps of one size travel and are processed as one batch, and the results of a batch come back in one
copy.  The sampling itself (random_sampling, build_epoch) stays on the host and consumes np.random exactly as the
reference does, so a seeded run draws the same epoch.  The centroid cache (build_centroids) has the reference's file
name and JSON text: a cache written by either side loads in the other.

Auto-labelled items (`refinement` in the label path with cfg.DROPOUT_COARSE_BOOST_CLASSES set, uniform.py:104-120): the
gtCoarse map is decoded beside the label, in the same thread pool and the same size batching, the id2trainid loop with
the gtCoarse merge of the boosted classes runs on the device (datasets/autolabel.py, prepare_labels(mode="original")) and
the centroid pass then takes its result without a table.  Such an item whose path does not contain
cfg.DATASET.CITYSCAPES_CUSTOMCOARSE has no gtCoarse map in the reference either (a NameError there) and is refused."""
import json
import os
from collections import defaultdict
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from ..config import cfg
from .autolabel import coarse_path, label_steps, prepare_labels

MAX_DECODE_WORKERS = 16      # host threads that decode PNGs (the reference's pool has 80, uniform.py:147)
BATCH_ITEMS = 16             # label maps decoded ahead and, where their sizes agree, processed in one launch
DEVICE = "cuda"              # where decoded label maps go


def calc_tile_locations(tile_size, image_size):
    """(x_offs, y_offs) of every full tile of an image of image_size = (height, width), row of tiles by row of tiles
    (uniform.py:67-81).  What does not fill a tile at the right and bottom edges belongs to none."""
    size_y, size_x = image_size
    return [(x * tile_size, y * tile_size) for y in range(size_y // tile_size) for x in range(size_x // tile_size)]


_LUTS = {}


def id2trainid_table(id2trainid):
    """The id2trainid step of uniform.py:112-121 as 256 bytes.  The reference compares against an untouched copy of the
    mask, so the step is a plain table: lut[k] = v for the keys a uint8 label can equal, identity elsewhere; any other
    key (Cityscapes' -1) matches no pixel and drops out."""
    lut = np.arange(256, dtype=np.uint8)
    for k, v in id2trainid.items():
        if 0 <= int(k) <= 255:
            if not 0 <= int(v) <= 255:
                raise ValueError("id2trainid maps %r to %r, which a uint8 label map cannot hold" % (k, v))
            lut[int(k)] = int(v)
    return lut


def _device_lut(id2trainid, device):
    if not id2trainid:
        return None
    key = (tuple(sorted((int(k), int(v)) for k, v in id2trainid.items())), str(device))
    t = _LUTS.get(key)
    if t is None:
        t = _LUTS[key] = torch.from_numpy(id2trainid_table(id2trainid)).to(device)
    return t


def class_centroids(labels_u8_cuda, tile_size, num_classes, id2trainid=None):
    """labels_u8_cuda: uint8 device tensor [H,W] or [N,H,W] (rows may be strided) -> int32 [tiles,C,2] or [N,tiles,C,2]:
    (x, y) of the centroid of every class in every tile of calc_tile_locations, in that order, image coordinates;
    (-1, -1) where the tile has no pixel of the class.  Enqueues three launches on the current stream; nothing waits."""
    from .. import hip_backend as hb
    from .._lib import lib, check
    m = labels_u8_cuda
    if m.dtype != torch.uint8 or m.dim() not in (2, 3):
        raise ValueError("label maps are uint8 tensors [H,W] or [N,H,W]")
    squeeze = m.dim() == 2
    if squeeze:
        m = m.unsqueeze(0)
    N, H, W = (int(v) for v in m.shape)
    if H > 1 and W > 0 and m.stride(2) == 1 and m.stride(1) >= W and (N == 1 or m.stride(0) == H * m.stride(1)):
        ld = int(m.stride(1))            # rows of a wider buffer: read in place
    else:
        m, ld = m.contiguous(), W
    tile, C = int(tile_size), int(num_classes)
    if tile < 1 or not 1 <= C <= 256:
        raise ValueError("tile_size >= 1 and 1 <= num_classes <= 256, not %r and %r" % (tile_size, num_classes))
    tiles = (H // tile) * (W // tile)
    out = torch.empty((N, tiles, C, 2), dtype=torch.int32, device=m.device)
    if out.numel():
        sums = torch.empty((N, tiles, C, 3), dtype=torch.int64, device=m.device)
        check(lib().ssa_class_centroids_u8(hb._p(m), N, H, W, ld, tile, C, hb._p(_device_lut(id2trainid, m.device)),
                                           hb._p(sums), hb._p(out), hb._s()), "ssa_class_centroids_u8")
    return out[0] if squeeze else out


def _auto_labelled(label_fn, id2trainid):
    """Whether the id2trainid loop of uniform.py:113-121 may merge gtCoarse pixels into this item's classes."""
    return bool(id2trainid) and "refinement" in label_fn and cfg.DROPOUT_COARSE_BOOST_CLASSES is not None


def _check_item(label_fn):
    if ("refinement" in label_fn and cfg.DROPOUT_COARSE_BOOST_CLASSES is not None
            and cfg.DATASET.CITYSCAPES_CUSTOMCOARSE not in label_fn):
        raise NotImplementedError("the auto-labelled (refinement / gtCoarse / DROPOUT_COARSE_BOOST_CLASSES) branch of the "
                                  "centroid pass is not implemented: %s" % label_fn)


def _decode(label_fn):
    from PIL import Image
    mask = np.array(Image.open(label_fn))
    if mask.dtype != np.uint8 or mask.ndim != 2:
        raise ValueError("%s: a label map is one 8-bit channel, not %s %r" % (label_fn, mask.dtype, mask.shape))
    return mask


def _decode_pair(fns):
    """(label map, gtCoarse map or None) of (label_fn, gtCoarse file or None): one job of the decoding pool."""
    label_fn, coarse_fn = fns
    mask = _decode(label_fn)
    if coarse_fn is None:
        return mask, None
    coarse = _decode(coarse_fn)
    if coarse.shape != mask.shape:
        raise ValueError("%s is %r, the label map %s %r" % (coarse_fn, coarse.shape, label_fn, mask.shape))
    return mask, coarse


def _merged_centroids(labels, coarse, tile_size, num_classes, id2trainid):
    """class_centroids of auto-labelled maps: the loop of uniform.py:112-121 with its gtCoarse merge first (the hit taken
    against the untouched map, the last hitting step wins), then the centroid pass without a table."""
    steps = label_steps(id2trainid, cfg.DROPOUT_COARSE_BOOST_CLASSES)
    merged = prepare_labels(labels, coarse if any(steps[2::3]) else None, None, steps, "original")
    return class_centroids(merged, tile_size, num_classes, None)


def _as_dict(item, table):
    """One image's int32 [tiles, C, 2] host table as the reference's dict: the classes in the order of their first
    tile, a class's entries in tile order (uniform.py:123-133 loops tiles, then classes)."""
    image_fn, label_fn = item
    centroids = defaultdict(list)
    t_idx, c_idx = np.nonzero(table[:, :, 0] >= 0)
    for (x, y), c in zip(table[t_idx, c_idx].tolist(), c_idx.tolist()):
        centroids[c].append((image_fn, label_fn, (x, y), c))
    return centroids


def class_centroids_image(item, tile_size, num_classes, id2trainid, labels=None, coarse=None):
    """item = (image_fn, label_fn) -> {class_id: [(image_fn, label_fn, (x, y), class_id), ...]} (uniform.py:84-135).
    labels: the decoded label map as a uint8 device tensor [H,W], if the caller has it; else label_fn is read.  coarse:
    likewise the gtCoarse map of an auto-labelled item."""
    _check_item(item[1])
    auto = _auto_labelled(item[1], id2trainid)
    if labels is None:
        labels = torch.from_numpy(_decode(item[1])).to(DEVICE)
    if not auto:
        return _as_dict(item, class_centroids(labels, tile_size, num_classes, id2trainid).cpu().numpy())
    if coarse is None:
        coarse = torch.from_numpy(_decode_pair((item[1], coarse_path(item[1])))[1]).to(labels.device)
    return _as_dict(item, _merged_centroids(labels, coarse, tile_size, num_classes, id2trainid).cpu().numpy())


def pooled_class_centroids_all(items, num_classes, id2trainid, tile_size=1024):
    """items: [(image_fn, label_fn), ...] -> {class_id: [...]} over all of them, each class's list in item order as
    pool.map keeps it (uniform.py:138-164).  BATCH_ITEMS maps are decoded at a time on at most MAX_DECODE_WORKERS host
    threads; those of one size go to the device as one tensor, through one call, and come back in one copy.  The gtCoarse
    map of an auto-labelled item is decoded by the same job as its label; auto-labelled maps of one size form a group of
    their own, which goes through prepare_labels and then through the centroid call without a table."""
    items = [tuple(it) for it in items]
    for _, label_fn in items:
        _check_item(label_fn)
    centroids = defaultdict(list)
    if not items:
        return centroids
    with ThreadPoolExecutor(max_workers=min(MAX_DECODE_WORKERS, BATCH_ITEMS, len(items))) as pool:
        for lo in range(0, len(items), BATCH_ITEMS):
            batch = items[lo:lo + BATCH_ITEMS]
            auto = [_auto_labelled(label_fn, id2trainid) for _, label_fn in batch]
            masks = list(pool.map(_decode_pair, [(label_fn, coarse_path(label_fn) if a else None)
                                                 for (_, label_fn), a in zip(batch, auto)]))
            by_size = defaultdict(list)
            for i, (m, _) in enumerate(masks):
                by_size[(m.shape, auto[i])].append(i)
            tables = [None] * len(batch)
            for (_, merged), idx in by_size.items():
                stacked = torch.from_numpy(np.stack([masks[i][0] for i in idx])).to(DEVICE)
                if merged:
                    coarse = torch.from_numpy(np.stack([masks[i][1] for i in idx])).to(DEVICE)
                    host = _merged_centroids(stacked, coarse, tile_size, num_classes, id2trainid).cpu().numpy()
                else:
                    host = class_centroids(stacked, tile_size, num_classes, id2trainid).cpu().numpy()
                for j, i in enumerate(idx):
                    tables[i] = host[j]
            for item, table in zip(batch, tables):
                for class_id, entries in _as_dict(item, table).items():
                    centroids[class_id].extend(entries)
    return centroids


def class_centroids_all(items, num_classes, id2trainid, tile_size=1024):
    """uniform.py:189-197."""
    return pooled_class_centroids_all(items, num_classes, id2trainid, tile_size)


def random_sampling(alist, num):
    """num items of alist in the order of ONE np.random.shuffle of its indices, wrapping around when num exceeds the
    list (uniform.py:200-216)."""
    len_list = len(alist)
    assert len_list, 'len_list is zero!'
    indices = np.arange(len_list)
    np.random.shuffle(indices)
    return [alist[indices[i % len_list]] for i in range(num)]


def build_centroids(imgs, num_classes, train, cv=None, coarse=False, custom_coarse=False, id2trainid=None):
    """The centroid table of a training set, from the cache under cfg.DATASET.CENTROID_ROOT if it is there
    (uniform.py:219-275; same file name, same JSON).  Rank 0 builds and writes it; with torch.distributed initialised the
    ranks meet at a barrier and the others read the file.  As in the reference the tile size of the pass is
    class_centroids_all's default, 1024, whatever cfg.DATASET.CLASS_UNIFORM_TILE says: the option only names the file."""
    if not (cfg.DATASET.CLASS_UNIFORM_PCT and train):
        return []
    centroid_fn = cfg.DATASET.NAME
    if coarse or custom_coarse:
        if coarse:
            centroid_fn += '_coarse'
        if custom_coarse:
            centroid_fn += '_customcoarse_final'
    else:
        centroid_fn += '_cv{}'.format(cv)
    centroid_fn += '_tile{}.json'.format(cfg.DATASET.CLASS_UNIFORM_TILE)
    json_fn = os.path.join(cfg.DATASET.CENTROID_ROOT, centroid_fn)

    def load():
        with open(json_fn, 'r') as json_data:
            loaded = json.load(json_data)
        return {int(idx): loaded[idx] for idx in loaded}

    if os.path.isfile(json_fn):
        return load()
    distributed = torch.distributed.is_available() and torch.distributed.is_initialized()
    rank = torch.distributed.get_rank() if distributed else 0
    if rank == 0:
        os.makedirs(cfg.DATASET.CENTROID_ROOT, exist_ok=True)
        centroids = class_centroids_all(imgs, num_classes, id2trainid=id2trainid)
        with open(json_fn, 'w') as outfile:
            json.dump(centroids, outfile, indent=4)
    if distributed:
        torch.distributed.barrier()
    if rank != 0:
        assert os.path.isfile(json_fn), 'Expected to find {}'.format(json_fn)
        centroids = load()
    return centroids


def build_epoch(imgs, centroids, num_classes, train):
    """One epoch's items: the random share first (one shuffle of imgs), then per class its share of centroid items, each
    class one shuffle of its own list; a class without centroids draws nothing (uniform.py:278-324).  Called every epoch;
    returns imgs unchanged when not training or with cfg.DATASET.CLASS_UNIFORM_PCT off."""
    class_uniform_pct = cfg.DATASET.CLASS_UNIFORM_PCT
    if not (train and class_uniform_pct):
        return imgs
    num_epoch = int(len(imgs))
    num_per_class = int((num_epoch * class_uniform_pct) / num_classes)
    num_rand = num_epoch - num_per_class * num_classes
    imgs_uniform = random_sampling(imgs, num_rand)
    bias = cfg.DATASET.CLASS_UNIFORM_BIAS
    for class_id in range(num_classes):
        count = num_per_class if bias is None else int(num_per_class * bias[class_id])
        if len(centroids[class_id]) == 0:
            continue
        imgs_uniform.extend(random_sampling(centroids[class_id], count))
    return imgs_uniform
