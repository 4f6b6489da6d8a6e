"""Dry run of the auto-labelled coarse data path's glue (the pattern of tests/test_uniform_glue_dryrun_cpu.py: the real
library, every launching entry point replaced by a stand-in that checks the call against the ctypes signature of
semseg_amd/_lib.py and records it): class_centroids_all over PNGs on disk -- plain items keep their single call with
the table, auto-labelled ones take ssa_autolabel_u8 and then the centroid call with a NULL table, one pair of calls per
size group -- and read_labels' arguments for a refinement item and for an ordinary label."""
import numpy as np
import pytest
import torch

import autolabel_cases as K

from test_uniform_glue_dryrun_cpu import RecLib, _ptr


@pytest.fixture()
def dry(monkeypatch):
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.config import cfg
    from semseg_amd.datasets import autolabel as A, uniform as U
    d = RecLib(_lib.lib())
    monkeypatch.setattr(_lib, "_LIB", d)
    monkeypatch.setattr(hb, "_s", lambda: None)
    monkeypatch.setattr(U, "DEVICE", "cpu")
    monkeypatch.setattr(A, "DEVICE", "cpu")
    saved, saved_boost = dict(cfg.DATASET), cfg.DROPOUT_COARSE_BOOST_CLASSES
    cfg.DATASET.update(CITYSCAPES_CUSTOMCOARSE=K.CUSTOMCOARSE, CITYSCAPES_DIR=K.CITYSCAPES_DIR)
    yield d
    cfg.DATASET.clear()
    cfg.DATASET.update(saved)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = saved_boost


def test_plain_items_keep_their_single_call(dry, tmp_path, monkeypatch):
    from semseg_amd.config import cfg
    from semseg_amd.datasets import class_centroids_all
    monkeypatch.chdir(tmp_path)
    files = K.write_tree(["plain", "plain_small", "coarse_not_refined"])
    cfg.DROPOUT_COARSE_BOOST_CLASSES = K.CITY_BOOST                             # on, and none of these is auto-labelled
    class_centroids_all([files[n] for n in ("plain", "plain_small", "coarse_not_refined")], 19, K.CITY, tile_size=16)
    assert dry.order == ["ssa_class_centroids_u8"] * 2
    assert [a[1:7] for a in dry.args["ssa_class_centroids_u8"]] == [(1, 37, 53, 53, 16, 19), (2, 19, 29, 29, 16, 19)]
    assert all(_ptr(a[7]) is not None for a in dry.args["ssa_class_centroids_u8"])
    # auto-labelled paths with the boost set off, or without an id map, are plain as well
    dry.order.clear()
    cfg.DROPOUT_COARSE_BOOST_CLASSES = None
    refine = K.write_tree(["refine"])["refine"]
    class_centroids_all([refine], 19, K.CITY, tile_size=16)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = K.CITY_BOOST
    class_centroids_all([refine], 19, None, tile_size=16)
    assert dry.order == ["ssa_class_centroids_u8"] * 2


def test_auto_labelled_items_merge_first(dry, tmp_path, monkeypatch):
    from semseg_amd.config import cfg
    from semseg_amd.datasets import class_centroids_all, uniform as U
    monkeypatch.chdir(tmp_path)
    files = K.write_tree(K.CENTROID_LIST)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = K.CITY_BOOST
    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(tuple(self.shape)), real_cpu(self, *a, **k))[1])
    workers = []
    real_pool = U.ThreadPoolExecutor
    monkeypatch.setattr(U, "ThreadPoolExecutor", lambda max_workers: (workers.append(max_workers), real_pool(max_workers))[1])
    class_centroids_all([files[n] for n in K.CENTROID_LIST], 19, K.CITY, tile_size=16)
    # four groups: (37 x 53, auto-labelled) x 3, (37 x 53, plain) x 1, (19 x 29, auto-labelled) x 1, (19 x 29, plain) x 2
    assert dry.order == ["ssa_autolabel_u8", "ssa_class_centroids_u8", "ssa_class_centroids_u8",
                         "ssa_autolabel_u8", "ssa_class_centroids_u8", "ssa_class_centroids_u8"]
    cent = dry.args["ssa_class_centroids_u8"]
    assert [a[1:7] for a in cent] == [(3, 37, 53, 53, 16, 19), (1, 37, 53, 53, 16, 19), (1, 19, 29, 29, 16, 19), (2, 19, 29, 29, 16, 19)]
    assert [_ptr(a[7]) is None for a in cent] == [True, False, True, False]      # merged maps take no table
    merges = dry.args["ssa_autolabel_u8"]
    steps = bytes(b for s in K.steps_of(K.CITY, K.CITY_BOOST) for b in s)
    for a, (n, h, w) in zip(merges, [(3, 37, 53), (1, 19, 29)]):
        assert a[3:9] == (n, h, w, w, w, 0) and _ptr(a[1]) is not None and a[2] is None          # gtCoarse, no probabilities
        assert a[9] == steps and a[10] == len(K.CITY)
        assert a[11:18] == (0, 0, 0, 0, 0, 0, 255)                             # mode original, no window, no threshold
        assert _ptr(a[20]) == _ptr(cent[merges.index(a) * 2][0])               # the centroid call reads what the merge wrote
        assert a[21] == w
    assert copies == [(3, 6, 19, 2), (1, 6, 19, 2), (1, 1, 19, 2), (2, 1, 19, 2)]      # one copy back per group
    assert workers == [len(K.CENTROID_LIST)]


def test_read_labels_arguments(dry, tmp_path, monkeypatch):
    from semseg_amd.config import cfg
    from semseg_amd.datasets import read_labels
    monkeypatch.chdir(tmp_path)
    K.write_tree(["full", "plain", "refine_vidseq"])
    cfg.DROPOUT_COARSE_BOOST_CLASSES = K.CITY_BOOST
    cfg.DATASET.update(MASK_OUT_CITYSCAPES=True, CUSTOM_COARSE_PROB=0.5, IGNORE_LABEL=255)
    out = read_labels(K.ITEMS["full"][0], {-1: 255, **K.CITY})
    assert dry.order == ["ssa_autolabel_u8"] and tuple(out.shape) == (1024, 2048) and out.dtype == torch.uint8
    a = dry.args["ssa_autolabel_u8"][0]
    assert all(_ptr(v) is not None for v in a[0:3]) and a[3:9] == (1, 1024, 2048, 2048, 2048, 2048)
    assert a[9] == bytes(b for s in K.steps_of(K.CITY, K.CITY_BOOST) for b in s) and a[10] == len(K.CITY)     # -1 dropped
    assert a[11:18] == (1, 14, 15, 2030, 840, 128, 255)                         # mode current, the drop mask, b / 255.0 < 0.5
    assert _ptr(a[20]) == out.data_ptr() and a[21] == 2048
    # an ordinary label: the same call, no boosted step, no gtCoarse, no probabilities, no window
    out = read_labels(K.ITEMS["plain"][0], K.CITY)
    a = dry.args["ssa_autolabel_u8"][1]
    assert a[1] is None and a[2] is None and a[3:6] == (1, 37, 53) and not any(a[9][2::3]) and a[11:17] == (1, 0, 0, 0, 0, 0)
    # a video sequence item: thresholded, not merged
    cfg.DATASET.MASK_OUT_CITYSCAPES = False
    read_labels(K.ITEMS["refine_vidseq"][0], K.CITY)
    a = dry.args["ssa_autolabel_u8"][2]
    assert a[1] is None and _ptr(a[2]) is not None and not any(a[9][2::3]) and a[11:17] == (1, 0, 0, 0, 0, 128)
    assert np.array_equal(np.frombuffer(a[9], dtype=np.uint8).reshape(-1, 3)[:, :2], np.array(list(K.CITY.items())))
