"""Class-uniform sampling on the host (semseg_amd/datasets/uniform.py, RandomSizeAndCrop of datasets/transforms.py):

  tests/uniform_ref.py, the integer restatement the kernels are held to, against the golden data of the real reference
      (tests/golden/uniform_golden.json, written by make_golden_uniform.py) and against live SciPy
  random_sampling / build_epoch / RandomSizeAndCrop.get_params against the golden data, generator state included
  the centroid cache: the JSON text of the reference from the restated tables, and a round trip through a file the
      reference wrote
  the configuration fields and their sync; argument rejection of both entry points without a device."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

import uniform_cases as K
import uniform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "uniform_golden.json")) as f:
        return json.load(f)


@pytest.fixture()
def dataset_cfg():
    from semseg_amd.config import cfg
    saved = dict(cfg.DATASET)
    yield cfg.DATASET
    cfg.DATASET.clear()
    cfg.DATASET.update(saved)


def restated(name):
    """[[class, [[image index, x, y], ...]], ...] as the golden stores a case, from the restatement."""
    N, H, W, tile, C, id2trainid, _, _ = K.CASES[name]
    maps = K.label_maps(name)
    dicts = [R.as_dict(K.file_names(name, i), R.centroid_table(maps[i], tile, C, id2trainid)[1]) for i in range(N)]
    index = {K.file_names(name, i)[1]: i for i in range(N)}
    m = R.merged(dicts)
    return [[c, [[index[e[1]], e[2][0], e[2][1]] for e in m[c]]] for c in m]


@pytest.mark.parametrize("name", list(K.CASES))
def test_restatement_equals_the_reference(golden, name):
    assert restated(name) == golden["centroids"][name]
    if name == "no_tiles":
        assert golden["centroids"][name] == []


def test_restatement_equals_live_scipy():
    from scipy.ndimage import center_of_mass
    n = 0
    for name in K.SMALL:
        N, H, W, tile, C, id2trainid, _, _ = K.CASES[name]
        for mask in K.label_maps(name):
            sums, cent = R.centroid_table(mask, tile, C, id2trainid)
            m = R.lut_of(id2trainid)[mask]
            for t, (x_offs, y_offs) in enumerate(R.tile_locations(tile, H, W)):
                patch = m[y_offs:y_offs + tile, x_offs:x_offs + tile]
                for c in range(C):
                    if c in patch:
                        cy, cx = center_of_mass((patch == c).astype(int))
                        assert (int(cx) + x_offs, int(cy) + y_offs) == tuple(cent[t, c]), (name, t, c)
                        assert int(sums[t, c, 0]) == int((patch == c).sum())
                        n += 1
                    else:
                        assert tuple(cent[t, c]) == (-1, -1) and not sums[t, c].any()
    assert n > 600
    # the adversarial quotient: sum = q * n - 1 lies 1/n below an integer
    for n_pix in (3, 1 << 10, (1 << 20) - 1, 1 << 20):
        for q in (1, 2, 1023, 2047):
            s = q * n_pix - 1
            assert int(np.float64(s) / np.float64(n_pix)) == s // n_pix


def test_tile_locations_and_table():
    from semseg_amd.datasets.uniform import calc_tile_locations, id2trainid_table
    assert calc_tile_locations(16, (37, 53)) == R.tile_locations(16, 37, 53) == [(0, 0), (16, 0), (32, 0), (0, 16), (16, 16),
                                                                                  (32, 16)]
    assert calc_tile_locations(16, (10, 53)) == []
    assert np.array_equal(id2trainid_table(K.TWO_ONTO_ONE), R.lut_of(K.TWO_ONTO_ONE))
    assert np.array_equal(id2trainid_table(K.CITY_LIKE), R.lut_of(K.CITY_LIKE))
    with pytest.raises(ValueError):
        id2trainid_table({3: 256})


def test_random_sampling_and_build_epoch(golden, dataset_cfg):
    from semseg_amd.datasets import build_epoch, random_sampling
    np.random.seed(9)
    assert random_sampling(list(range(10)), 25) == golden["random_sampling"]["items"]
    assert K.np_state_digest() == golden["random_sampling"]["state"]
    with pytest.raises(AssertionError):
        random_sampling([], 3)
    for (seed, n_items, pct, bias, train), want in zip(K.EPOCHS, golden["epochs"]):
        imgs, centroids = K.epoch_inputs(n_items)
        dataset_cfg.CLASS_UNIFORM_PCT, dataset_cfg.CLASS_UNIFORM_BIAS = pct, bias
        np.random.seed(seed)
        got = build_epoch(imgs, centroids, K.EPOCH_CLASSES, train)
        assert json.loads(json.dumps(got)) == want["items"], seed
        assert K.np_state_digest() == want["state"], seed
        if not train or not pct:
            assert got is imgs


def _plan_dict(p):
    return {"scale_amt": p.scale_amt, "size": list(p.size), "border": list(p.border), "margins": list(p.margins),
            "window": list(p.window), "state": K.py_state_digest()}


def test_plans_equal_the_reference_draw_for_draw(golden, dataset_cfg):
    from semseg_amd.datasets import RandomSizeAndCrop
    seen = set()
    for (seed, crop_size, nopad, smin, smax, full, pre, taf, size, centroid), want in zip(K.PLANS, golden["plans"]):
        dataset_cfg.TRANSLATE_AUG_FIX = taf
        t = RandomSizeAndCrop(crop_size, nopad, scale_min=smin, scale_max=smax, full_size=full, pre_size=pre)
        random.seed(seed)
        for rep, e in enumerate(want):
            p = t.get_params(size, centroid)
            assert _plan_dict(p) == e, (seed, rep)
            assert p.pad == (p.border[0] + p.margins[0], p.border[1] + p.margins[1], p.border[0] + p.margins[2],
                             p.border[1] + p.margins[3])
            if centroid is not None:
                assert p.centroid == tuple(int(c * p.scale_amt) for c in centroid)
            seen.add(("border" if any(p.border) else "margins" if any(p.margins) else "plain", centroid is not None,
                      tuple(p.size) == tuple(p.window[2:])))
    # every branch was drawn: padded by a border / by margins / not padded, each with and without a centroid
    assert {s[:2] for s in seen} == {(k, c) for k in ("border", "margins", "plain") for c in (False, True)}


def test_a_window_outside_the_pair_is_refused(dataset_cfg):
    """Under TRANSLATE_AUG_FIX with one side shorter than the crop and a centroid, the reference draws a box that
    leaves the image and Pillow fills it with zeros: no plan, after the same draws."""
    from semseg_amd.datasets import RandomSizeAndCrop
    dataset_cfg.TRANSLATE_AUG_FIX = True
    t = RandomSizeAndCrop((32, 48), False, scale_min=1.0, scale_max=1.0)
    random.seed(3)
    random.uniform(1.0, 1.0), random.randint(5 - 48, 5), random.randint(5 - 32, 5)
    want = K.py_state_digest()
    random.seed(3)
    with pytest.raises(ValueError):
        t.get_params((40, 60), (5, 5))
    assert K.py_state_digest() == want


def _write_pngs(names_and_maps):
    from PIL import Image
    for fn, m in names_and_maps:
        Image.fromarray(np.asarray(m)).save(fn)


def _json_items():
    items = [K.file_names(n, i) for n in K.JSON_SET for i in range(K.CASES[n][0])]
    maps = [K.label_maps(n)[i] for n in K.JSON_SET for i in range(K.CASES[n][0])]
    items.append((K.JSON_BIG[0] + "_leftImg8bit.png", K.JSON_BIG[0] + "_labelIds.png"))
    maps.append(K.json_big_map())
    return items, maps


def test_cache_text_from_the_restatement(golden):
    """json.dump(..., indent=4) of the merged restated dicts is the reference's file, byte for byte."""
    items, maps = _json_items()
    dicts = [R.as_dict(it, R.centroid_table(m, K.JSON_TILE, K.JSON_CLASSES, K.TWO_ONTO_ONE)[1]) for it, m in zip(items, maps)]
    assert json.dumps(R.merged(dicts), indent=4) == golden["json_text"]
    assert len(json.loads(golden["json_text"])) >= 5


def test_build_centroids_reads_a_reference_cache(golden, dataset_cfg, tmp_path, monkeypatch):
    from semseg_amd.datasets import uniform as U
    dataset_cfg.CENTROID_ROOT, dataset_cfg.NAME, dataset_cfg.CLASS_UNIFORM_TILE = str(tmp_path), "toy", 512
    assert golden["json_name"] == "toy_cv0_tile512.json"
    (tmp_path / golden["json_name"]).write_text(golden["json_text"])
    monkeypatch.setattr(U, "class_centroids_all", lambda *a, **k: pytest.fail("the cache is there"))
    got = U.build_centroids([("a", "b")], K.JSON_CLASSES, True, cv=0)
    assert got == {int(k): v for k, v in json.loads(golden["json_text"]).items()}
    assert U.build_centroids([("a", "b")], K.JSON_CLASSES, False, cv=0) == []
    dataset_cfg.CLASS_UNIFORM_PCT = 0
    assert U.build_centroids([("a", "b")], K.JSON_CLASSES, True, cv=0) == []


def test_build_centroids_file_names(dataset_cfg, tmp_path, monkeypatch):
    from semseg_amd.datasets import uniform as U
    dataset_cfg.CENTROID_ROOT, dataset_cfg.NAME, dataset_cfg.CLASS_UNIFORM_TILE = str(tmp_path / "deep" / "er"), "city", 1024
    calls = []

    def fake(imgs, num_classes, id2trainid=None, **kw):
        calls.append((imgs, num_classes, id2trainid, kw))       # no tile size: class_centroids_all's default, 1024
        return {0: [("i", "l", (1, 2), 0)]}
    monkeypatch.setattr(U, "class_centroids_all", fake)
    for kw, name in (({"cv": 2}, "city_cv2_tile1024.json"), ({"coarse": True}, "city_coarse_tile1024.json"),
                     ({"custom_coarse": True}, "city_customcoarse_final_tile1024.json"),
                     ({"coarse": True, "custom_coarse": True}, "city_coarse_customcoarse_final_tile1024.json")):
        got = U.build_centroids([("i", "l")], 19, True, id2trainid={1: 0}, **kw)
        assert got == {0: [("i", "l", (1, 2), 0)]}
        assert (tmp_path / "deep" / "er" / name).read_text() == json.dumps(got, indent=4)
    assert len(calls) == 4 and all(c[3] == {} and c[2] == {1: 0} for c in calls)


def test_refinement_branch_is_not_implemented(monkeypatch):
    from semseg_amd.config import cfg
    from semseg_amd.datasets import class_centroids_all, class_centroids_image
    monkeypatch.setitem(cfg, "DROPOUT_COARSE_BOOST_CLASSES", [3])
    with pytest.raises(NotImplementedError):
        class_centroids_image(("a.png", "x/refinement/a.png"), 1024, 19, None)
    with pytest.raises(NotImplementedError):
        class_centroids_all([("a.png", "x/refinement/a.png")], 19, None)


def test_config_defaults_and_sync(golden):
    from semseg_amd import config
    fresh = config._defaults().DATASET
    for k, v in golden["config"].items():
        assert fresh[k] == v, k

    class NS:
        def __init__(self, **kw):
            self.__dict__.update(kw)
    saved = {k: (dict(v) if isinstance(v, dict) else v) for k, v in config.cfg.items()}
    ref = NS(MODEL=NS(OCR=NS(MID_CHANNELS=512, KEY_CHANNELS=256), ALIGN_CORNERS=False),
             LOSS=NS(OCR_ALPHA=0.4, OCR_AUX_RMI=False, SUPERVISED_MSCALE_WT=0), OPTIONS=NS(INIT_DECODER=False),
             DATASET=NS(NUM_CLASSES=19, IGNORE_LABEL=255, NAME="mapillary", CLASS_UNIFORM_PCT=0.25, CLASS_UNIFORM_TILE=512,
                        CLASS_UNIFORM_BIAS=[1.0] * 19, CENTROID_ROOT="/somewhere", TRANSLATE_AUG_FIX=True))
    try:
        config.sync_from_reference(ref)
        d = config.cfg.DATASET
        assert (d.NAME, d.CLASS_UNIFORM_PCT, d.CLASS_UNIFORM_TILE, d.CLASS_UNIFORM_BIAS, d.CENTROID_ROOT, d.TRANSLATE_AUG_FIX) == (
            "mapillary", 0.25, 512, [1.0] * 19, "/somewhere", True)
    finally:
        for k, v in saved.items():
            if isinstance(v, dict):
                config.cfg[k].clear()
                config.cfg[k].update(v)
            else:
                config.cfg[k] = v


def test_argument_rejection_without_a_device():
    from semseg_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_ubyte * 4096)()
    p = ctypes.c_void_p(ctypes.addressof(buf))
    ok = dict(labels=p, N=1, H=16, W=16, ld=16, tile=8, C=19, lut=None, sums=p, centroids=p)

    def cent(**kw):
        a = dict(ok, **kw)
        return L.ssa_class_centroids_u8(a["labels"], a["N"], a["H"], a["W"], a["ld"], a["tile"], a["C"], a["lut"], a["sums"],
                                        a["centroids"], None)
    for bad in (dict(labels=None), dict(sums=None), dict(centroids=None), dict(ld=15), dict(tile=0), dict(tile=-3), dict(C=0),
                dict(C=257), dict(N=-1), dict(H=-1), dict(W=-1, ld=0)):
        assert cent(**bad) == -1, bad
    # an image smaller than a tile has no tiles: nothing to launch, not an error -- and no device is touched
    assert cent(H=7) == 0 and cent(W=7, ld=7) == 0 and cent(N=0) == 0

    def pad(src=p, H=4, W=4, ch=3, l=1, t=1, r=1, b=1, fill=b"\0\0\0", dst=p):
        return L.ssa_pad_u8(src, H, W, ch, l, t, r, b, fill, dst, None)
    for bad in (dict(src=None), dict(dst=None), dict(fill=None), dict(H=0), dict(W=0), dict(ch=2), dict(ch=4), dict(l=-1),
                dict(t=-1), dict(r=-1), dict(b=-1)):
        assert pad(**bad) == -1, bad
