"""Golden vectors for the device ColorJitter, recorded from the REAL reference (transforms/transforms.py:192-362,
imported through ref_bootstrap.py) and from Pillow.
    python tests/golden/make_golden_colorjitter.py   ->   colorjitter_golden.npz

  images     a 37x53 random RGB image and a 1/f-like one (tests/colorjit_ref.py pink_image)
  entries    per seed: the constructor arguments, the (operation, factor) list that the reference's
             ColorJitter.get_params drew after np.random.seed(seed), in the shuffled order, and the output of the
             reference's ColorJitter.__call__ after the same seeding.  The reference's adjust_hue writes
             np.uint8(hue_factor * 255), which NumPy 2 refuses for a negative factor (OverflowError; NumPy 1.x wrapped
             it): those entries are marked "wrapped" and their output comes from the same Pillow calls in the drawn
             order with the wrapped byte trunc(hue_factor * 255) mod 256.
  hashes     SHA-256 of Pillow's output over the 4096x4096 image of all 2^24 colours: ImageEnhance.Brightness and
             ImageEnhance.Color at 0.75, 1.0, 1.25 and 1.9 (clips), the HSV round trip with H + {0, 1, 63, 193, 255}.

The reference module imports torchvision.transforms (Lambda, Compose), skimage and scipy.ndimage.interpolation at its
top; ref_bootstrap stubs torchvision with an empty module, so the two classes get inert shims here, as does skimage."""
import hashlib
import json
import os
import sys

import numpy as np
from PIL import Image, ImageEnhance

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import colorjit_ref as R                          # noqa: E402
from ref_bootstrap import _mod, bootstrap         # noqa: E402


class Lambda:
    def __init__(self, lambd):
        self.lambd = lambd

    def __call__(self, img):
        return self.lambd(img)


class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, img):
        for t in self.transforms:
            img = t(img)
        return img


def reference_transforms():
    bootstrap()
    tr = sys.modules["torchvision.transforms"]
    tr.Lambda, tr.Compose = Lambda, Compose
    sk = _mod("skimage")
    sk.filters = _mod("skimage.filters", gaussian=None)
    sk.restoration = _mod("skimage.restoration", denoise_bilateral=None)
    sk.segmentation = _mod("skimage.segmentation", find_boundaries=None)
    try:
        import scipy.ndimage.interpolation  # noqa: F401
    except ImportError:
        _mod("scipy.ndimage.interpolation", shift=None)
    import transforms.transforms as T
    return T


def drawn(transform):
    """The (operation, factor) list of the Compose that get_params returned: each Lambda closes over `<op>_factor`."""
    out = []
    for t in transform.transforms:
        (name,), (cell,) = t.lambd.__code__.co_freevars, t.lambd.__closure__
        assert name.endswith("_factor"), name
        out.append((name[:-len("_factor")], float(cell.cell_contents)))
    return out


def pillow_hue(pil, byte):
    h, s, v = pil.convert("HSV").split()
    np_h = (np.array(h, dtype=np.uint8).astype(np.int64) + byte).astype(np.uint8)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def pillow_chain(pil, draws):
    for op, v in draws:
        if op == "brightness":
            pil = ImageEnhance.Brightness(pil).enhance(v)
        elif op == "contrast":
            pil = ImageEnhance.Contrast(pil).enhance(v)
        elif op == "saturation":
            pil = ImageEnhance.Color(pil).enhance(v)
        else:
            pil = pillow_hue(pil, R.hue_byte(v))
    return pil


def main():
    T = reference_transforms()
    rng = np.random.RandomState(11)
    images = np.stack([rng.randint(0, 256, (37, 53, 3)).astype(np.uint8), R.pink_image(37, 53, 12)])
    cases = [(seed, (0.25, 0.25, 0.25, 0.25)) for seed in range(32)]
    cases += [(100, (0.25, 0, 0.25, 0)), (101, (0, 0.25, 0, 0.25)), (102, (0, 0, 0, 0.1)), (103, (0, 0, 0, 0.1)),
              (104, (0.4, 0.4, 0, 0)), (105, (0, 0.9, 0.9, 0.5)), (106, (0, 0.25, 0, 0)), (107, (0, 0, 0, 0))]
    entries, outputs = [], []
    for k, (seed, args) in enumerate(cases):
        np.random.seed(seed)
        draws = drawn(T.ColorJitter.get_params(*args))
        pil = Image.fromarray(images[k % 2])
        np.random.seed(seed)
        wrapped = False
        try:
            out = T.ColorJitter(*args)(pil)
            assert np.array_equal(np.array(out), np.array(pillow_chain(pil, draws))), seed   # the stand-in is the same chain
        except OverflowError:
            wrapped = True
            out = pillow_chain(pil, draws)
        outputs.append(np.array(out))
        entries.append({"seed": seed, "args": list(args), "image": k % 2, "draws": [[op, v] for op, v in draws],
                        "wrapped": wrapped})
    cube = Image.fromarray(R.all_colours())
    hashes = {}
    for f in (0.75, 1.0, 1.25, 1.9):
        hashes["brightness:%r" % f] = hashlib.sha256(np.array(ImageEnhance.Brightness(cube).enhance(f)).tobytes()).hexdigest()
        hashes["saturation:%r" % f] = hashlib.sha256(np.array(ImageEnhance.Color(cube).enhance(f)).tobytes()).hexdigest()
    for byte in (0, 1, 63, 193, 255):
        hashes["hue:%d" % byte] = hashlib.sha256(np.array(pillow_hue(cube, byte)).tobytes()).hexdigest()
    meta = {"pillow": Image.__version__, "numpy": np.__version__, "entries": entries, "hashes": hashes}
    np.savez_compressed(os.path.join(HERE, "colorjitter_golden.npz"), images=images, outputs=np.stack(outputs),
                        meta=np.array(json.dumps(meta)))
    print("entries", len(entries), "wrapped", sum(e["wrapped"] for e in entries), "hashes", len(hashes))


if __name__ == "__main__":
    main()
