"""Golden vectors for the device RandomGaussianBlur, recorded from the REAL reference (transforms/transforms.py:154-162,
imported through ref_bootstrap.py).
    python tests/golden/make_golden_gblur.py   ->   gblur_golden.npz

  in<i> / out<i>   per entry: the uint8 image handed to the reference's RandomGaussianBlur.__call__ after
                   random.seed(seed), and what it returned
  entries          per entry: the seed, the sigma the reference drew (seen by the stand-in below), its radius and weights
                   as live SciPy derives them (scipy.ndimage._filters._gaussian_kernel1d), and random.random() drawn right
                   after the call: the state the reference leaves Python's generator in
  meta             the SciPy and NumPy versions, and the wrapper assumption

scikit-image is NOT installed where this fixture was recorded.  The reference calls skimage.filters.gaussian(image, sigma,
multichannel=True); the stand-in below restates that function as the thin wrapper it is -- img_as_float of a uint8 image
(skimage/util/dtype.py: np.multiply(image, 1. / 255, dtype=float64)), then scipy.ndimage.gaussian_filter(image, [sigma,
sigma, 0], mode='nearest', cval=0, truncate=4.0) -- over LIVE SciPy.  Everything else (the draw, the * 255, the cast, the
PIL round trip) is the reference's own code.  tests/test_gblur_cpu.py holds the test that compares the restatement with
scikit-image itself wherever that can be imported."""
import json
import os
import random
import sys

import numpy as np
import scipy
import scipy.ndimage
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import colorjit_ref as CR                          # noqa: E402  (pink_image)
from ref_bootstrap import _mod, bootstrap         # noqa: E402

SEEN = []


def gaussian(image, sigma=1, output=None, mode="nearest", cval=0, multichannel=None, preserve_range=False,
             truncate=4.0):
    """skimage.filters.gaussian for a uint8 H x W x 3 image with multichannel=True, restated (see the module docstring)."""
    assert image.dtype == np.uint8 and image.ndim == 3 and multichannel is True and not preserve_range
    SEEN.append(float(sigma))
    image = np.multiply(image, 1. / 255, dtype=np.float64)
    return scipy.ndimage.gaussian_filter(image, [sigma, sigma, 0], output=output, mode=mode, cval=cval, truncate=truncate)


def reference_transforms():
    bootstrap()
    tr = sys.modules["torchvision.transforms"]
    tr.Lambda = tr.Compose = None
    sk = _mod("skimage")
    sk.filters = _mod("skimage.filters", gaussian=gaussian)
    sk.restoration = _mod("skimage.restoration", denoise_bilateral=None)
    sk.segmentation = _mod("skimage.segmentation", find_boundaries=None)
    try:
        import scipy.ndimage.interpolation  # noqa: F401
    except ImportError:
        _mod("scipy.ndimage.interpolation", shift=None)
    import transforms.transforms as T
    return T


def main():
    try:
        import skimage  # noqa: F401
        raise SystemExit("scikit-image is importable here: record from it (drop the stand-in) instead")
    except ImportError:
        pass
    T = reference_transforms()
    from scipy.ndimage._filters import _gaussian_kernel1d
    rng = np.random.RandomState(21)
    rand = lambda h, w: rng.randint(0, 256, (h, w, 3)).astype(np.uint8)          # noqa: E731
    const = np.empty((16, 16, 3), np.uint8)
    const[...] = (77, 200, 255)
    cases = [(0, rand(37, 53)), (1, CR.pink_image(48, 64, 5)), (2, const), (3, rand(1, 64)), (5, rand(3, 2)),
             (15, CR.pink_image(37, 53, 6)), (31, rand(24, 31))]
    arrays, entries = {}, []
    for i, (seed, img) in enumerate(cases):
        random.seed(seed)
        out = np.array(T.RandomGaussianBlur()(Image.fromarray(img)))
        after = random.random()
        sigma = SEEN[-1]
        radius = int(4.0 * sigma + 0.5)
        weights = _gaussian_kernel1d(sigma, 0, radius)[::-1][radius:]
        assert out.shape == img.shape and out.dtype == np.uint8 and len(SEEN) == i + 1
        arrays["in%d" % i], arrays["out%d" % i] = img, out
        entries.append({"seed": seed, "sigma": sigma, "radius": radius, "weights": [float(w) for w in weights],
                        "random_after": after, "shape": list(img.shape)})
    assert sorted({e["radius"] for e in entries}) == [1, 2, 3, 4, 5]
    meta = {"scipy": scipy.__version__, "numpy": np.__version__, "skimage": None,
            "wrapper": "scikit-image absent: skimage.filters.gaussian restated as np.multiply(image, 1 / 255, dtype=float64) "
                       "followed by scipy.ndimage.gaussian_filter(image, [sigma, sigma, 0], mode='nearest', cval=0, "
                       "truncate=4.0)",
            "entries": entries}
    path = os.path.join(HERE, "gblur_golden.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **arrays)
    print("entries", len(entries), "radii", [e["radius"] for e in entries], "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
