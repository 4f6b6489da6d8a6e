"""Golden data of the auto-labelled coarse data path tests: the REAL reference (BaseLoader.__getitem__ of
datasets/base_loader.py and pooled_class_centroids_all of datasets/uniform.py, through ref_bootstrap) on the items of
tests/autolabel_cases.py, written as PNGs in a temporary tree -> tests/golden/autolabel_golden.json.

  id_to_trainid   Cityscapes' label2trainid as the reference has it, without negative keys, in order: [[id, trainId], ...]
                  (under NumPy 2 the reference's own `mask == -1` ... `mask[...] = v` loop raises OverflowError on a uint8
                  mask with the key -1, which matches no pixel anyway)
  labels          per item the label map BaseLoader.__getitem__ returned: zlib + base64 of the bytes, or for the full-size
                  item their SHA-256
  centroids       pooled_class_centroids_all over autolabel_cases.CENTROID_LIST (CITY ids) and over CENTROID_CHAIN (CHAIN
                  ids): [[class, [[item index, x, y], ...]], ...] in the dict's own key order
  config          the reference's defaults of the fields semseg_amd/config.py copies for this path

Build-container only; run from the repository root:  python tests/golden/make_golden_autolabel.py"""
import base64
import hashlib
import importlib.util
import json
import os
import sys
import tempfile
import types
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_bootstrap  # noqa: E402
import autolabel_cases as K  # noqa: E402
import autolabel_ref as R  # noqa: E402


def _load(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref_bootstrap.REF, rel))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    cfg = ref_bootstrap.bootstrap()
    d = cfg.DATASET
    out = {"config": {"CITYSCAPES_DIR": d.CITYSCAPES_DIR, "CITYSCAPES_CUSTOMCOARSE": d.CITYSCAPES_CUSTOMCOARSE,
                      "COARSE_BOOST_CLASSES": d.COARSE_BOOST_CLASSES, "CUSTOM_COARSE_PROB": d.CUSTOM_COARSE_PROB,
                      "MASK_OUT_CITYSCAPES": d.MASK_OUT_CITYSCAPES, "IGNORE_LABEL": d.IGNORE_LABEL}}
    # by file, with stand-ins for the packages whose __init__ modules pull in scikit-image (not installed, not used here)
    U = _load("ref_uniform", "datasets/uniform.py")
    labels_mod = _load("ref_cityscapes_labels", "datasets/cityscapes_labels.py")
    sys.modules["datasets"] = types.ModuleType("datasets")
    sys.modules["datasets"].uniform = U
    sys.modules["utils"] = types.ModuleType("utils")
    sys.modules["utils.misc"] = types.ModuleType("utils.misc")
    sys.modules["utils.misc"].tensor_to_pil = None
    BL = _load("ref_base_loader", "datasets/base_loader.py")
    city = {k: v for k, v in labels_mod.label2trainid.items() if k >= 0}
    assert city == K.CITY and list(city) == list(K.CITY)
    out["id_to_trainid"] = [[int(k), int(v)] for k, v in city.items()]
    d.CITYSCAPES_CUSTOMCOARSE, d.CITYSCAPES_DIR, d.DUMP_IMAGES = K.CUSTOMCOARSE, K.CITYSCAPES_DIR, False
    work = tempfile.mkdtemp()
    cwd = os.getcwd()
    os.chdir(work)
    try:
        files = K.write_tree()
        out["labels"] = {}
        for name, (path, (H, W), ids, st) in K.ITEMS.items():
            cfg.DROPOUT_COARSE_BOOST_CLASSES, d.MASK_OUT_CITYSCAPES, d.CUSTOM_COARSE_PROB = st["boost"], st["mask_out"], st["prob"]
            loader = BL.BaseLoader("semantic", "train", None, None, None)
            loader.id_to_trainid = dict(K.ID_MAPS[ids])
            loader.imgs = [files[name]]
            _, mask, _, _ = loader[0]
            got = np.array(mask)
            assert got.dtype == np.uint8 and got.shape == (H, W)
            raw = got.tobytes()
            out["labels"][name] = ({"sha256": hashlib.sha256(raw).hexdigest()} if name == "full" else
                                   {"z": base64.b64encode(zlib.compress(raw, 9)).decode()})
            print(name, got.shape, "differs from a plain id -> trainId table in",
                  int((got != R.plain_table(K.item_maps(name)[0], K.ID_MAPS[ids])).sum()), "pixels")
        d.MASK_OUT_CITYSCAPES, d.CUSTOM_COARSE_PROB = False, None
        out["centroids"] = {}
        for key, names, ids, boost in (("list", K.CENTROID_LIST, "CITY", K.CITY_BOOST), ("chain", K.CENTROID_CHAIN, "CHAIN", K.CHAIN_BOOST)):
            cfg.DROPOUT_COARSE_BOOST_CLASSES = boost
            items = [files[n] for n in names]
            got = U.pooled_class_centroids_all(items, K.CENTROID_CLASSES, dict(K.ID_MAPS[ids]), K.CENTROID_TILE)
            index = {it[1]: i for i, it in enumerate(items)}
            out["centroids"][key] = [[int(c), [[index[e[1]], int(e[2][0]), int(e[2][1])] for e in got[c]]] for c in got]
            print(key, sum(len(got[c]) for c in got), "centroids")
    finally:
        os.chdir(cwd)
    path = os.path.join(HERE, "autolabel_golden.json")
    with open(path, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
