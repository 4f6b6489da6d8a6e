"""The auto-labelled coarse data path on the host (semseg_amd/datasets/autolabel.py, the auto-labelled branch of
semseg_amd/datasets/uniform.py):

  tests/autolabel_ref.py, the sequential restatement the kernels are held to, against the golden data of the real
      reference (tests/golden/autolabel_golden.json, written by make_golden_autolabel.py): the loader's label maps and the
      centroids of a mixed list -- and NOT equal to what a plain id -> trainId table gives
  the specification of ssa_autolabel_u8 (autolabel_ref.merge with label_steps and prob_cut) against the same data
  label_steps, prob_cut, the path decisions of label_plan against a table of paths and cfg states
  argument rejection through the real library, without a device; the configuration fields and their sync."""
import base64
import ctypes
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import autolabel_cases as K
import autolabel_ref as R
import uniform_ref as UR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "autolabel_golden.json")) as f:
        return json.load(f)


@pytest.fixture()
def coarse_cfg():
    """cfg as the items of autolabel_cases are read under; restored afterwards."""
    from semseg_amd.config import cfg
    saved, saved_boost = dict(cfg.DATASET), cfg.DROPOUT_COARSE_BOOST_CLASSES
    cfg.DATASET.update(CITYSCAPES_CUSTOMCOARSE=K.CUSTOMCOARSE, CITYSCAPES_DIR=K.CITYSCAPES_DIR)
    yield cfg
    cfg.DATASET.clear()
    cfg.DATASET.update(saved)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = saved_boost


def golden_labels(golden, name):
    e = golden["labels"][name]
    H, W = K.ITEMS[name][1]
    return np.frombuffer(zlib.decompress(base64.b64decode(e["z"])), dtype=np.uint8).reshape(H, W)


def restated_labels(name):
    path, _, ids, st = K.ITEMS[name]
    o, g, p = K.item_maps(name)
    return R.loader_labels(path, o, g, p, K.ID_MAPS[ids], K.CUSTOMCOARSE, st["boost"], st["mask_out"], st["prob"])


def restated_centroids(names, ids, boost):
    dicts = []
    for i, n in enumerate(names):
        path = K.ITEMS[n][0]
        o, g, _ = K.item_maps(n)
        m = R.centroid_labels(path, o, g, K.ID_MAPS[ids], K.CUSTOMCOARSE, boost)
        dicts.append(UR.as_dict((i, i), UR.centroid_table(m, K.CENTROID_TILE, K.CENTROID_CLASSES)[1]))
    m = UR.merged(dicts)
    return [[c, [[e[1], e[2][0], e[2][1]] for e in m[c]]] for c in m]


@pytest.mark.parametrize("name", list(K.ITEMS))
def test_restatement_equals_the_reference_loader(golden, name):
    got = restated_labels(name)
    if name == "full":
        assert hashlib.sha256(got.tobytes()).hexdigest() == golden["labels"][name]["sha256"]
    else:
        assert np.array_equal(got, golden_labels(golden, name))
    path, _, ids, st = K.ITEMS[name]
    plain = R.plain_table(K.item_maps(name)[0], K.ID_MAPS[ids])
    # an ordinary label IS the plain table; an auto-labelled one is far from it (merge, chain, threshold, drop mask)
    assert np.array_equal(got, plain) == ("refinement" not in path)
    if name == "full":
        assert int((got != plain).sum()) > 1000000


def test_restatement_equals_the_reference_centroids(golden):
    assert restated_centroids(K.CENTROID_LIST, "CITY", K.CITY_BOOST) == golden["centroids"]["list"]
    assert restated_centroids(K.CENTROID_CHAIN, "CHAIN", K.CHAIN_BOOST) == golden["centroids"]["chain"]
    # a plain table is not enough for the auto-labelled items of the list
    for n in ("refine", "refine_vidseq", "refine_small", "chain"):
        path, _, ids, st = K.ITEMS[n]
        o, g, _ = K.item_maps(n)
        assert not np.array_equal(R.centroid_labels(path, o, g, K.ID_MAPS[ids], K.CUSTOMCOARSE, st["boost"]),
                                  R.plain_table(o, K.ID_MAPS[ids])), n


def test_id_map_is_the_reference_s(golden):
    assert [[k, v] for k, v in K.CITY.items()] == golden["id_to_trainid"]


@pytest.mark.parametrize("name", list(K.ITEMS))
def test_the_specification_equals_the_reference(golden, coarse_cfg, name):
    """autolabel_ref.merge -- the statement of ssa_autolabel_u8 in include/semseg_hip.h -- fed what label_plan, label_steps
    and prob_cut decide for the item: the loader's label, and the centroid pass's map."""
    from semseg_amd.datasets import label_plan, label_steps
    cfg = coarse_cfg
    path, _, ids, st = K.ITEMS[name]
    cfg.DROPOUT_COARSE_BOOST_CLASSES = st["boost"]
    cfg.DATASET.update(MASK_OUT_CITYSCAPES=st["mask_out"], CUSTOM_COARSE_PROB=st["prob"])
    plan = label_plan(path)
    steps = label_steps(K.ID_MAPS[ids], plan.boost)
    triples = [tuple(steps[i:i + 3]) for i in range(0, len(steps), 3)]
    assert triples == K.steps_of(K.ID_MAPS[ids], plan.boost)
    o, g, p = K.item_maps(name)
    got = R.merge(o, g, p, triples, "current", plan.window, plan.prob_cut, cfg.DATASET.IGNORE_LABEL)
    assert np.array_equal(got, restated_labels(name))
    if st["boost"] is not None:
        triples = K.steps_of(K.ID_MAPS[ids], st["boost"] if "refinement" in path else None)
        assert np.array_equal(R.merge(o, g, None, triples, "original"),
                              R.centroid_labels(path, o, g, K.ID_MAPS[ids], K.CUSTOMCOARSE, st["boost"]))


def test_kernel_cases_tell_the_modes_and_the_gates_apart():
    """The cases are not vacuous: the two modes differ on the chains, the presence gates decide pixels, the batch of three
    has per-image bits, and no case equals a plain table where a merge happens."""
    want = {n: R.merge_batch(*_args(n)) for n in K.KERNEL}
    for n in ("chain", "chain_perm", "via_earlier", "all256"):
        assert not np.array_equal(want[n + "_current"], want[n + "_original"]), n
    assert not np.array_equal(want["chain_current"], want["chain_perm_current"])
    # only in g: nothing of g's 27 arrives (the other boosted ids, present in o, do merge)
    o, g, p = K.inputs("only_in_g_current")
    there = g == 27
    assert there.any() and np.array_equal(want["only_in_g_current"][there], R.plain_table(o, K.CITY)[there])
    assert not np.array_equal(want["only_in_g_current"], R.plain_table(o, K.CITY))
    # present only through an earlier step: g's 6 arrives in mode current and not in mode original
    o, g, p = K.inputs("via_earlier_current")
    there = (g == 6) & (o != 5)
    assert there.any() and (want["via_earlier_current"][there] == 7).all() and (want["via_earlier_original"][there] != 7).all()
    # one image of three
    o, g, p = K.inputs("n3_one_image_current")
    merged = [bool((want["n3_one_image_current"][i][(g[i] == 28) & (o[i] != 28)] == 15).all()) for i in range(3)]
    assert merged == [False, True, False]
    # the boosted id sits in the dropped region alone: absent, no merge
    o, g, p = K.inputs("in_dropped")
    assert (o == 31).any() and (g == 31).any() and not (want["in_dropped"] == 16).any()
    # thresholds: both sides of every cut occur
    for cut in (1, 128, 255):
        p = K.inputs("cut_%d" % cut)[2]
        assert (p == cut - 1).any() and (p == cut).any()
    assert (want["cut_256"] == 255).all() and not np.array_equal(want["cut_0"], want["cut_1"])


def _args(name):
    c = K.KERNEL[name]
    o, g, p = K.inputs(name)
    return o, g if c["coarse"] else None, p if c["cut"] else None, c["steps"], c["mode"], c["window"], c["cut"], c["ignore"]


def test_label_steps_and_prob_cut():
    from semseg_amd.datasets import label_steps, prob_cut
    assert label_steps({}) == b"" and label_steps(None) == b""
    assert label_steps({-1: 255, 3: 1, 300: 4, 2: 3}, [3]) == bytes([3, 1, 0, 2, 3, 1])       # order kept, -1 and 300 dropped
    assert label_steps({3: 1, 2: 3}) == bytes([3, 1, 0, 2, 3, 0])
    assert label_steps({2: 3, 3: 1}, []) == bytes([2, 3, 0, 3, 1, 0])
    assert len(label_steps(K.ALL256, K.ALL256_BOOST)) == 3 * 256
    with pytest.raises(ValueError):
        label_steps({3: 256})
    b = np.arange(256)
    for prob in (0.5, 1.0, 0.001, 0.0, -1.0, 2.0, 1 / 255.0, 128 / 255.0, 0.9):
        cut = prob_cut(prob)
        assert np.array_equal(b < cut, b / 255.0 < prob), prob
    assert [prob_cut(v) for v in (0.5, 1.0, 0.001, 0.0, 2.0)] == [128, 255, 1, 0, 256]
    with pytest.raises(ValueError):
        prob_cut(None)


CC, CS = "/data/cs/autolabelled", "/data/cs"
#          path, boost set, mask_out, prob -> refinement, boost on, gtCoarse file, window, cut
PLANS = [
    (CC + "/refinement/aachen/a_leftImg8bit.png", [14, 15], True, 0.5,
     (True, True, CS + "/gtCoarse/gtCoarse/refinement/aachen/a_gtCoarse_labelIds.png", True, 128)),
    (CC + "/refinement/aachen/a_leftImg8bit.png", [14, 15], False, 0.5, (True, True, True, False, 128)),
    (CC + "/refinement/aachen/a_leftImg8bit.png", None, True, 0.9, (True, False, True, True, 230)),
    (CC + "/refinement/vidseq/a_leftImg8bit.png", [14, 15], True, 0.5, (True, False, True, True, 128)),
    (CC + "/other/a_leftImg8bit.png", [14, 15], True, 0.5, (False, False, True, False, 0)),
    ("/elsewhere/refinement/a_leftImg8bit.png", [14, 15], True, 0.5, (True, True, None, True, 128)),
    ("/data/cs/gtFine/train/a_gtFine_labelIds.png", [14, 15], True, 0.5, (False, False, None, False, 0)),
    ("/data/cs/gtFine/train/a_gtFine_labelIds.png", None, False, None, (False, False, None, False, 0)),
]


@pytest.mark.parametrize("row", range(len(PLANS)))
def test_label_plan_decides_as_the_reference(coarse_cfg, row):
    from semseg_amd.datasets import label_plan
    from semseg_amd.datasets.autolabel import DROP_MASK_WINDOW
    path, boost, mask_out, prob, (refinement, boost_on, coarse_fn, window, cut) = PLANS[row]
    cfg = coarse_cfg
    cfg.DATASET.update(CITYSCAPES_CUSTOMCOARSE=CC, CITYSCAPES_DIR=CS, MASK_OUT_CITYSCAPES=mask_out, CUSTOM_COARSE_PROB=prob)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = boost
    p = label_plan(path)
    assert p.refinement == refinement and p.boost == (boost if boost_on else None)
    if coarse_fn is True:
        coarse_fn = path.replace(CC, CS + "/gtCoarse/gtCoarse").replace("leftImg8bit", "gtCoarse_labelIds")
    assert p.coarse_fn == coarse_fn
    assert p.window == (DROP_MASK_WINDOW if window else None) and DROP_MASK_WINDOW == R.DROP_WINDOW
    assert p.prob_cut == cut and p.prob_fn == (path.replace(".png", "_prob.png") if refinement else None)


def test_read_labels_refuses_what_the_reference_cannot_do(coarse_cfg, tmp_path, monkeypatch):
    from semseg_amd.datasets import label_plan, read_labels
    cfg = coarse_cfg
    monkeypatch.chdir(tmp_path)
    K.write_tree(["refine", "refine_small"])
    path = K.ITEMS["refine"][0]
    cfg.DROPOUT_COARSE_BOOST_CLASSES = K.CITY_BOOST
    cfg.DATASET.update(MASK_OUT_CITYSCAPES=True, CUSTOM_COARSE_PROB=None)
    with pytest.raises(ValueError, match="CUSTOM_COARSE_PROB"):          # a TypeError in the reference
        read_labels(path, K.CITY)
    cfg.DATASET.CUSTOM_COARSE_PROB = 0.5
    with pytest.raises(ValueError, match="drop mask"):                   # 1024 x 2048 times 37 x 53 in the reference
        read_labels(path, K.CITY)
    cfg.DATASET.update(MASK_OUT_CITYSCAPES=False, CITYSCAPES_CUSTOMCOARSE="/not/in/the/path")
    with pytest.raises(ValueError, match="gtCoarse"):                    # a NameError in the reference
        read_labels(path, K.CITY)
    with pytest.raises(ValueError):
        label_plan("")


def test_centroid_pass_keeps_its_refusal(coarse_cfg):
    """An auto-labelled item with the boost set on and no gtCoarse to merge (the path lacks CITYSCAPES_CUSTOMCOARSE)."""
    from semseg_amd.datasets import class_centroids_all
    coarse_cfg.DROPOUT_COARSE_BOOST_CLASSES = [14]
    with pytest.raises(NotImplementedError, match="not implemented"):
        class_centroids_all([("a.png", "elsewhere/refinement/a_leftImg8bit.png")], 19, K.CITY)


def test_argument_rejection_without_a_device():
    from semseg_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_ubyte * (65536 + 64))()
    base = ctypes.addressof(buf)
    base += -base % 16
    p = ctypes.c_void_p(base)
    steps = bytes([1, 2, 0, 2, 3, 1])
    ok = dict(labels=p, coarse=p, prob=p, N=1, H=16, W=16, ld_l=16, ld_c=16, ld_p=16, steps=steps, n=2, mode=1, win=(0, 0, 0, 0),
              cut=128, ignore=255, pairs=p, table=p, out=p, ld_o=16)

    def call(**kw):
        a = dict(ok, **kw)
        return L.ssa_autolabel_u8(a["labels"], a["coarse"], a["prob"], a["N"], a["H"], a["W"], a["ld_l"], a["ld_c"], a["ld_p"],
                                  a["steps"], a["n"], a["mode"], *a["win"], a["cut"], a["ignore"], a["pairs"], a["table"],
                                  a["out"], a["ld_o"], None)
    bad = [dict(labels=None), dict(pairs=None), dict(table=None), dict(out=None), dict(ld_l=15), dict(ld_c=15), dict(ld_p=15),
           dict(ld_o=15), dict(n=-1), dict(n=257), dict(steps=None), dict(coarse=None), dict(cut=-1), dict(cut=257),
           dict(prob=None), dict(ignore=256), dict(ignore=-1), dict(mode=2), dict(mode=-1), dict(N=-1), dict(H=-1),
           dict(W=-1), dict(win=(0, 0, 17, 16)), dict(win=(0, 0, 16, 17)), dict(win=(-1, 0, 16, 16)), dict(win=(0, -1, 16, 16)),
           dict(win=(15, 15, 17, 17)), dict(pairs=ctypes.c_void_p(base + 2))]
    for kw in bad:
        assert call(**kw) == -1, kw
    # nothing to do is not an error, and no device is touched: no image, no rows, no columns
    assert call(N=0) == 0 and call(H=0) == 0 and call(W=0, ld_l=0, ld_c=0, ld_p=0, ld_o=0) == 0
    # what may be absent: coarse without a boosted step, prob without a threshold, steps when there are none
    assert call(N=0, coarse=None, steps=bytes([1, 2, 0, 2, 3, 0])) == 0
    assert call(N=0, prob=None, cut=0) == 0 and call(N=0, steps=None, n=0, coarse=None) == 0
    # an empty window is no drop mask, wherever it lies
    assert call(N=0, win=(40, 40, 40, 90)) == 0 and call(N=0, win=(5, 9, 99, 9)) == 0


def test_prepare_labels_checks_its_arguments():
    import torch
    from semseg_amd.datasets import prepare_labels
    m = torch.zeros((4, 6), dtype=torch.uint8)
    steps = bytes([1, 2, 1])
    for bad in (lambda: prepare_labels(m, None, None, steps, "current"),                # a boosted step without gtCoarse
                lambda: prepare_labels(m, m, None, steps, "current", prob_cut=3),       # a threshold without a map
                lambda: prepare_labels(m, m, None, steps, "sideways"),
                lambda: prepare_labels(m.int(), m, None, steps, "current"),
                lambda: prepare_labels(m, m[:3], None, steps, "current"),
                lambda: prepare_labels(m, m, None, steps[:2], "current")):
        with pytest.raises(ValueError):
            bad()


def test_config_defaults_and_sync(golden):
    from semseg_amd import config
    fresh = config._defaults()
    for k, v in golden["config"].items():
        assert fresh.DATASET[k] == v, k
    assert fresh.DROPOUT_COARSE_BOOST_CLASSES is None

    class NS:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    saved = {k: (dict(v) if isinstance(v, dict) else v) for k, v in config.cfg.items()}
    base = dict(MODEL=NS(OCR=NS(MID_CHANNELS=512, KEY_CHANNELS=256), ALIGN_CORNERS=False),
                LOSS=NS(OCR_ALPHA=0.4, OCR_AUX_RMI=False, SUPERVISED_MSCALE_WT=0), OPTIONS=NS(INIT_DECODER=False))
    try:
        config.sync_from_reference(NS(DATASET=NS(NUM_CLASSES=19, IGNORE_LABEL=255, CITYSCAPES_DIR="/cs", CITYSCAPES_CUSTOMCOARSE="/cc",
                                                 COARSE_BOOST_CLASSES=[3, 4], CUSTOM_COARSE_PROB=0.5, MASK_OUT_CITYSCAPES=True),
                                      DROPOUT_COARSE_BOOST_CLASSES=[14, 15, 16], **base))
        d = config.cfg.DATASET
        assert (d.CITYSCAPES_DIR, d.CITYSCAPES_CUSTOMCOARSE, d.COARSE_BOOST_CLASSES, d.CUSTOM_COARSE_PROB, d.MASK_OUT_CITYSCAPES) == (
            "/cs", "/cc", [3, 4], 0.5, True)
        assert config.cfg.DROPOUT_COARSE_BOOST_CLASSES == [14, 15, 16]
        # a reference cfg without the fields (older call sites) leaves them alone
        config.sync_from_reference(NS(DATASET=NS(NUM_CLASSES=19, IGNORE_LABEL=255), **base))
        assert config.cfg.DATASET.CITYSCAPES_CUSTOMCOARSE == "/cc" and config.cfg.DATASET.CUSTOM_COARSE_PROB == 0.5
    finally:
        for k, v in saved.items():
            if isinstance(v, dict):
                config.cfg[k].clear()
                config.cfg[k].update(v)
            else:
                config.cfg[k] = v
