"""Golden data of the class-uniform sampling tests: the REAL reference (datasets/uniform.py, transforms/
joint_transforms.py through ref_bootstrap) on the cases of tests/uniform_cases.py -> tests/golden/uniform_golden.json.

  centroids   per case the merged dict of pooled_class_centroids_all over the case's label maps, written as PNGs in a
              temporary directory under the fixed relative names of uniform_cases.file_names: [[class, [[image index,
              x, y], ...]], ...] in the dict's own key order
  json_text   what build_centroids writes for uniform_cases.JSON_SET + JSON_BIG, and its file name
  epochs      build_epoch for uniform_cases.EPOCHS, with the digest of np.random's state afterwards
  plans       what RandomSizeAndCrop decided for uniform_cases.PLANS (scale, resized size, border, margins, crop box),
              read off the Pillow calls it made, with the digest of random's state after every call
  pairs       the same for uniform_cases.PAIRS, with the bytes of the pair it returned
  config      the reference's defaults of the fields semseg_amd/config.py copies

Build-container only; run from the repository root:  python tests/golden/make_golden_uniform.py"""
import importlib.util
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_bootstrap  # noqa: E402
import uniform_cases as K  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_bootstrap.REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    cfg = ref_bootstrap.bootstrap()
    import torch
    from PIL import Image, ImageOps
    # by file: the packages' __init__ modules pull in scikit-image, which is not installed and which neither module uses
    U = _load("ref_uniform", "datasets/uniform.py")
    JT = _load("ref_joint_transforms", "transforms/joint_transforms.py")
    out = {}
    d = cfg.DATASET
    out["config"] = {"NAME": d.NAME, "CLASS_UNIFORM_PCT": d.CLASS_UNIFORM_PCT, "CLASS_UNIFORM_TILE": d.CLASS_UNIFORM_TILE,
                     "CLASS_UNIFORM_BIAS": None,            # config.py:253, set by assert_and_infer_cfg
                     "CENTROID_ROOT": d.CENTROID_ROOT, "TRANSLATE_AUG_FIX": d.TRANSLATE_AUG_FIX}
    torch.distributed.barrier = lambda *a, **k: None        # build_centroids meets its ranks there; there is one
    cfg.GLOBAL_RANK = 0
    cfg.DROPOUT_COARSE_BOOST_CLASSES = None
    work = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(work)
    try:
        # ---- centroids
        out["centroids"] = {}
        for name, (N, H, W, tile, C, id2trainid, _, _) in K.CASES.items():
            maps = K.label_maps(name)
            items = []
            for i in range(N):
                image_fn, label_fn = K.file_names(name, i)
                Image.fromarray(maps[i]).save(label_fn)
                items.append((image_fn, label_fn))
            got = U.pooled_class_centroids_all(items, C, id2trainid, tile)
            index = {it[1]: i for i, it in enumerate(items)}
            out["centroids"][name] = [[int(c), [[index[e[1]], int(e[2][0]), int(e[2][1])] for e in got[c]]] for c in got]
            assert all(e[3] == c for c in got for e in got[c])
            print(name, sum(len(got[c]) for c in got), "centroids")
        # ---- the cache file
        items = [K.file_names(n, i) for n in K.JSON_SET for i in range(K.CASES[n][0])]
        big = (K.JSON_BIG[0] + "_leftImg8bit.png", K.JSON_BIG[0] + "_labelIds.png")
        Image.fromarray(K.json_big_map()).save(big[1])
        items.append(big)
        d.CENTROID_ROOT, d.NAME, d.CLASS_UNIFORM_TILE, d.CLASS_UNIFORM_PCT = "centroid_cache", "toy", 512, 0.5
        got = U.build_centroids(items, K.JSON_CLASSES, True, cv=0, id2trainid=K.TWO_ONTO_ONE)
        (fn,) = os.listdir("centroid_cache")
        out["json_name"], out["json_text"] = fn, open(os.path.join("centroid_cache", fn)).read()
        assert U.build_centroids(items, K.JSON_CLASSES, True, cv=0) == {int(k): v for k, v in json.loads(out["json_text"]).items()}
        assert U.build_centroids(items, K.JSON_CLASSES, False, cv=0) == []
    finally:
        os.chdir(cwd)
    # ---- epochs
    out["epochs"] = []
    for seed, n_items, pct, bias, train in K.EPOCHS:
        imgs, centroids = K.epoch_inputs(n_items)
        d.CLASS_UNIFORM_PCT, d.CLASS_UNIFORM_BIAS = pct, bias
        np.random.seed(seed)
        got = U.build_epoch(imgs, centroids, K.EPOCH_CLASSES, train)
        out["epochs"].append({"items": json.loads(json.dumps(got)), "state": K.np_state_digest()})
    np.random.seed(9)
    out["random_sampling"] = {"items": U.random_sampling(list(range(10)), 25), "state": K.np_state_digest()}
    d.CLASS_UNIFORM_PCT, d.CLASS_UNIFORM_BIAS = 0.5, None

    # ---- plans: what the transform decided, read off the Pillow calls it made
    rec = {}
    real_resize, real_crop, real_expand, real_margin = Image.Image.resize, Image.Image.crop, ImageOps.expand, JT.add_margin

    def resize(self, size, *a, **k):
        rec["size"] = [int(size[0]), int(size[1])]
        return real_resize(self, size, *a, **k)

    def crop(self, box=None):
        rec["window"] = [int(box[0]), int(box[1]), int(box[2] - box[0]), int(box[3] - box[1])]
        return real_crop(self, box)

    def expand(image, border=0, fill=0):
        assert border[0] == border[2] and border[1] == border[3]
        rec["border"] = [int(border[0]), int(border[1])]
        return real_expand(image, border=border, fill=fill)

    def add_margin(pil_img, top, right, bottom, left, margin_color):
        rec["margins"] = [int(left), int(top), int(right), int(bottom)]
        return real_margin(pil_img, top, right, bottom, left, margin_color)

    Image.Image.resize, Image.Image.crop, ImageOps.expand, JT.add_margin = resize, crop, expand, add_margin

    def run(t, img, mask, centroid):
        rec.clear()
        res = t(img, mask, centroid)
        w, h = res[0].size
        assert res[0].size == res[1].size
        e = {"scale_amt": res[2], "size": rec["size"], "border": rec.get("border", [0, 0]),
             "margins": rec.get("margins", [0, 0, 0, 0]), "window": rec.get("window", [0, 0, w, h]),
             "state": K.py_state_digest()}
        assert e["window"][2:] == [w, h]
        return e, res

    try:
        out["plans"] = []
        for seed, crop_size, nopad, smin, smax, full, pre, taf, size, centroid in K.PLANS:
            d.TRANSLATE_AUG_FIX = taf
            t = JT.RandomSizeAndCrop(crop_size, nopad, scale_min=smin, scale_max=smax, full_size=full, pre_size=pre)
            random.seed(seed)
            draws = []
            for _ in range(K.PLAN_REPEATS):
                e, _ = run(t, Image.new("RGB", size), Image.new("L", size), centroid)
                draws.append(e)
            out["plans"].append(draws)
        out["pairs"] = []
        for seed, crop_size, (smin, smax), taf, size, centroid in K.PAIRS:
            d.TRANSLATE_AUG_FIX = taf
            img, lab = K.pair(seed, size)
            t = JT.RandomSizeAndCrop(crop_size, False, scale_min=smin, scale_max=smax)
            random.seed(seed)
            e, res = run(t, Image.fromarray(img), Image.fromarray(lab), centroid)
            e["img"] = np.array(res[0]).tobytes().hex()
            e["lab"] = np.array(res[1]).tobytes().hex()
            out["pairs"].append(e)
    finally:
        Image.Image.resize, Image.Image.crop, ImageOps.expand, JT.add_margin = real_resize, real_crop, real_expand, real_margin
        d.TRANSLATE_AUG_FIX = False
    path = os.path.join(HERE, "uniform_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
