"""Generate tests/golden/fboundary_golden.npz from the REAL reference: the boundary F-score of utils/f_boundary.py.

Run in the build container (where the reference checkout exists):
    python tests/golden/make_golden_fboundary.py
For every case of tests/fboundary_cases.py: eval_mask_boundary(pred, gt, C, bound_th=...) itself (its process pool
included) under the case's cfg.DATASET.IGNORE_LABEL, and db_eval_boundary on the arguments eval_mask_boundary builds for
every (image, class).  Stored per case: `Fpc`, `Fc`, the per-(image, class) `F` and `P` (precision); per input set the
uint8 prediction and the int64 ground truth.  Only data: no line of the reference is copied.

The reference does not run as shipped (SHIMS below, also stored in the fixture's `meta`): seg2bmap uses `np.bool`, which
NumPy 1.24 removed -- aliased to `bool` for the run; scikit-image is not installed where this was recorded, so
skimage.morphology.disk and binary_dilation are restated over NumPy / scipy.ndimage as scikit-image defines them (disk:
X**2 + Y**2 <= radius**2 over arange(-radius, radius + 1); binary_dilation: scipy.ndimage.binary_dilation with the
footprint as structure)."""
import json
import os
import sys

import numpy as np
import scipy
import scipy.ndimage as ndi

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import fboundary_cases as K                       # noqa: E402
from ref_bootstrap import _mod, bootstrap         # noqa: E402

SHIMS = ["np.bool = bool",
         "skimage.morphology.disk(radius): L = np.arange(-radius, radius + 1); X, Y = np.meshgrid(L, L); "
         "(X ** 2 + Y ** 2 <= radius ** 2).astype(np.uint8)",
         "skimage.morphology.binary_dilation(image, footprint): scipy.ndimage.binary_dilation(image, structure=footprint)",
         "eval_mask_boundary called with num_proc=2"]


def _disk(radius, dtype=np.uint8):
    L = np.arange(-radius, radius + 1)
    X, Y = np.meshgrid(L, L)
    return np.array((X ** 2 + Y ** 2) <= radius ** 2, dtype=dtype)


def _binary_dilation(image, footprint=None, out=None):
    return ndi.binary_dilation(image, structure=footprint, output=out)


def reference_module():
    cfg = bootstrap()
    if not hasattr(np, "bool"):
        np.bool = bool
    sk = _mod("skimage")
    sk.morphology = _mod("skimage.morphology", disk=_disk, binary_dilation=_binary_dilation)
    import utils.f_boundary as FB
    return cfg, FB


def main():
    cfg, FB = reference_module()
    out = {"meta": np.array(json.dumps({"scipy": scipy.__version__, "numpy": np.__version__, "shims": SHIMS}))}
    for name in K.ALL:
        k = K.CASES[name]
        cfg.DATASET.IGNORE_LABEL = k["ignore"]
        pred, gt = K.inputs(name)
        seg, gtm = pred.astype(np.int64), gt.copy()
        Fpc, Fc = FB.eval_mask_boundary(seg, gtm, k["C"], num_proc=2, bound_th=k["bound_th"])
        assert np.array_equal(seg, pred) and np.array_equal(gtm, gt)
        B = pred.shape[0]
        F = np.zeros((B, k["C"]))
        P = np.zeros((B, k["C"]))
        for c in range(k["C"]):
            for i in range(B):
                F[i, c], P[i, c] = FB.db_eval_boundary((seg[i] == c).astype(np.uint8), (gtm[i] == c).astype(np.uint8),
                                                       gtm[i] == cfg.DATASET.IGNORE_LABEL, k["bound_th"])
        assert not np.isnan(F).any() and np.array_equal(Fc, np.full(k["C"], float(B))), name
        out[name + "/Fpc"], out[name + "/Fc"], out[name + "/F"], out[name + "/P"] = Fpc, Fc, F, P
        out[k["inp"] + "/pred"], out[k["inp"] + "/gt"] = pred, gt
        print("%-12s Fpc/Fc mean %.6f" % (name, float(np.mean(Fpc / Fc))))
    np.savez_compressed(os.path.join(HERE, "fboundary_golden.npz"), **out)


if __name__ == "__main__":
    main()
