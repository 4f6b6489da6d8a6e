"""Dry run of the class-uniform sampling glue (the pattern of tests/test_hip_glue_dryrun_cpu.py: the real library, every
launching entry point replaced by a stand-in that checks the call against the ctypes signature of semseg_amd/_lib.py
and records it): class_centroids_all over PNGs on disk -- one call and one copy back per batch of same-sized maps --,
and RandomSizeAndCrop.apply -> crop_flip_normalize on CPU tensors, padded and not."""
import collections
import ctypes
import random

import numpy as np
import pytest
import torch

import uniform_cases as K

from test_hip_glue_dryrun_cpu import DryLib


class RecLib(DryLib):
    """DryLib that also keeps the order and the arguments of the calls."""

    def __init__(self, real):
        super().__init__(real)
        self.order, self.args = [], collections.defaultdict(list)

    def __getattr__(self, name):
        fn = DryLib.__getattr__(self, name)
        if not name.startswith("ssa_"):
            return fn

        def launch(*args):
            rc = fn(*args)
            self.order.append(name)
            self.args[name].append(args)
            return rc
        return launch


class _OnDevice(torch.Tensor):
    """A CPU tensor that answers is_cuda as a device tensor does: the public entry points assert it of their inputs."""
    is_cuda = property(lambda self: True)


@pytest.fixture()
def dry(monkeypatch):
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets import uniform as U
    d = RecLib(_lib.lib())
    monkeypatch.setattr(_lib, "_LIB", d)
    monkeypatch.setattr(hb, "_s", lambda: None)
    monkeypatch.setattr(U, "DEVICE", "cpu")
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **k: collections.namedtuple("S", "cuda_stream")(0))
    return d


def _ptr(v):
    return v.value if isinstance(v, ctypes.c_void_p) else v


def test_class_centroids_all_batches_same_sized_maps(dry, tmp_path, monkeypatch):
    from PIL import Image
    from semseg_amd.datasets import class_centroids_all, uniform as U
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(U, "BATCH_ITEMS", 4)
    sizes = [(37, 53), (19, 29), (37, 53), (37, 53), (37, 53), (19, 29)]       # batches of 4 and 2: 2 + 2 calls
    items = []
    for i, (h, w) in enumerate(sizes):
        items.append(("i%d.png" % i, "l%d.png" % i))
        Image.fromarray(np.full((h, w), i, dtype=np.uint8)).save(items[-1][1])
    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(tuple(self.shape)), real_cpu(self, *a, **k))[1])
    workers = []
    real_pool = U.ThreadPoolExecutor
    monkeypatch.setattr(U, "ThreadPoolExecutor", lambda max_workers: (workers.append(max_workers), real_pool(max_workers))[1])
    got = class_centroids_all(items, 19, K.TWO_ONTO_ONE, tile_size=16)
    assert dry.order == ["ssa_class_centroids_u8"] * 4
    shapes = [a[1:7] for a in dry.args["ssa_class_centroids_u8"]]                # N, H, W, ld, tile, C
    assert shapes == [(3, 37, 53, 53, 16, 19), (1, 19, 29, 29, 16, 19), (1, 37, 53, 53, 16, 19), (1, 19, 29, 29, 16, 19)]
    luts = {_ptr(a[7]) for a in dry.args["ssa_class_centroids_u8"]}
    assert len(luts) == 1 and None not in luts                                  # one table, built once
    assert copies == [(3, 6, 19, 2), (1, 1, 19, 2), (1, 6, 19, 2), (1, 1, 19, 2)]    # one copy back per call
    assert workers == [4] and U.MAX_DECODE_WORKERS <= 16
    assert isinstance(got, dict)
    # without a table the argument is NULL; an image smaller than a tile launches nothing
    dry.order.clear()
    U.class_centroids(torch.zeros((37, 53), dtype=torch.uint8), 16, 19)
    assert dry.order == ["ssa_class_centroids_u8"] and dry.args["ssa_class_centroids_u8"][-1][7] is None
    out = U.class_centroids(torch.zeros((2, 10, 53), dtype=torch.uint8), 16, 19)
    assert tuple(out.shape) == (2, 0, 19, 2) and len(dry.order) == 1
    with pytest.raises(ValueError):
        U.class_centroids(torch.zeros((37, 53), dtype=torch.int64), 16, 19)
    with pytest.raises(ValueError):
        U.class_centroids(torch.zeros((37, 53), dtype=torch.uint8), 16, 257)


@pytest.mark.parametrize("scale,padded", [(0.5, True), (1.5, False)])
def test_apply_then_tail(dry, scale, padded):
    from semseg_amd.config import cfg
    from semseg_amd.datasets import RandomSizeAndCrop, crop_flip_normalize
    img = torch.zeros((30, 40, 3), dtype=torch.uint8).as_subclass(_OnDevice)
    lab = torch.zeros((30, 40), dtype=torch.uint8).as_subclass(_OnDevice)
    t = RandomSizeAndCrop((24, 32), False, scale_min=scale, scale_max=scale)
    random.seed(0)
    plan = t.get_params((40, 30), (20, 15))
    assert any(plan.pad) == padded and plan.size == (int(40 * scale), int(30 * scale))
    d_img, d_lab, window = t.apply(plan, img, lab)
    resizes = ["ssa_resample_u8", "ssa_resample_u8", "ssa_resize_nearest_u8"]
    assert dry.order == resizes + (["ssa_pad_u8", "ssa_pad_u8"] if padded else [])       # no padding: no extra copy
    l, tp, r, b = plan.pad
    assert tuple(d_img.shape) == (plan.size[1] + tp + b, plan.size[0] + l + r, 3) and tuple(d_lab.shape) == tuple(d_img.shape[:2])
    if padded:
        a_img, a_lab = dry.args["ssa_pad_u8"]
        assert a_img[1:8] == (plan.size[1], plan.size[0], 3, l, tp, r, b) and a_img[8] == bytes([0, 0, 0])
        assert a_lab[1:8] == (plan.size[1], plan.size[0], 1, l, tp, r, b) and a_lab[8] == bytes([cfg.DATASET.IGNORE_LABEL] * 3)
        assert _ptr(a_img[9]) == d_img.data_ptr() and _ptr(a_lab[9]) == d_lab.data_ptr()
    dry.order.clear()
    out, gts = crop_flip_normalize(d_img.as_subclass(_OnDevice), d_lab.as_subclass(_OnDevice), window, True)
    assert dry.order == ["ssa_image_u8_crop_flip_normalize", "ssa_label_u8_crop_flip"]
    a = dry.args["ssa_image_u8_crop_flip_normalize"][0]
    assert (_ptr(a[0]), *a[1:8]) == (d_img.data_ptr(), d_img.shape[0], d_img.shape[1], *window, 1)
    assert tuple(out.shape) == (1, 24, 32, 16) and tuple(gts.shape) == (1, 24, 32)
    # the call form: the reference's four results
    dry.order.clear()
    random.seed(0)
    res = t(img, lab, (20, 15))
    assert len(res) == 4 and res[2] == plan.window and res[3] == plan.scale_amt
