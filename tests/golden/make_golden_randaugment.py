"""Golden vectors for the device RandAugment, recorded from the REAL reference (datasets/randaugment.py, loaded through
ref_bootstrap.py) running on the installed Pillow.
    python tests/golden/make_golden_randaugment.py   ->   randaugment_golden.npz

  images, labels   a 37x53 random RGB image and a 1/f-like one (tests/colorjit_ref.py pink_image), each with a 19-class
                   label map (tests/randaug_ref.py label_map)
  ops              every operation of augment_list at m in {0, 1, 9, 15, 30}, called as RandAugment.__call__ calls it
                   (val = m / 30 * (maxval - minval) + minval) after random.seed(seed); for the five operations that draw
                   a sign, one seed per sign.  Entry k runs on image k % 2.
  chains           RandAugment(n, m)(img, mask) after random.seed(seed) for (n, m) in {(1,9), (2,9), (3,15), (2,30)} over
                   8 seeds each: the drawn program (recorded by wrapping the module's operations), both outputs and the
                   next random.random() after the call.
Outputs that occur more than once (Identity, the operations without a magnitude, m = 0) are stored once: an entry holds
the indices of its image and label output in `out_images` / `out_labels`."""
import importlib.util
import json
import os
import random
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import colorjit_ref as CR                         # noqa: E402
import randaug_ref as R                           # noqa: E402
from ref_bootstrap import REF, bootstrap          # noqa: E402

SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
MAGNITUDES = (0, 1, 9, 15, 30)
CHAINS = ((1, 9), (2, 9), (3, 15), (2, 30))


def reference_module():
    bootstrap()
    spec = importlib.util.spec_from_file_location("ref_randaugment", os.path.join(REF, "datasets", "randaugment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def seed_with_sign(negate, start):
    """The first seed >= start whose first random.random() is > 0.5 (the reference then negates v) or is not."""
    s = start
    while True:
        random.seed(s)
        if (random.random() > 0.5) == negate:
            return s
        s += 1


class Store:
    def __init__(self):
        self.arrays, self.index = [], {}

    def put(self, a):
        a = np.ascontiguousarray(a)
        key = a.tobytes()
        if key not in self.index:
            self.index[key] = len(self.arrays)
            self.arrays.append(a)
        return self.index[key]


def main():
    ra = reference_module()
    assert [f.__name__ for f, _, _ in ra.augment_list()] == list(R.OPS)
    assert [(lo, hi) for _, lo, hi in ra.augment_list()] == list(R.RANGES)
    fill = int(ra.fillmask)
    rng = np.random.RandomState(11)
    images = np.stack([rng.randint(0, 256, (37, 53, 3)).astype(np.uint8), CR.pink_image(37, 53, 12)])
    labels = np.stack([R.label_map(37, 53, 5), R.label_map(37, 53, 6)])
    out_i, out_l = Store(), Store()

    def record(entry, pair):
        entry["out_image"], entry["out_label"] = out_i.put(np.array(pair[0])), out_l.put(np.array(pair[1]))
        return entry

    ops, k = [], 0
    for op, lo, hi in ra.augment_list():
        for m in MAGNITUDES:
            for negate in ((False, True) if op.__name__ in SIGNED else (None,)):
                seed = 1000 + k if negate is None else seed_with_sign(negate, 1000 + k)
                val = (float(m) / 30) * float(hi - lo) + lo
                random.seed(seed)
                pair = op((Image.fromarray(images[k % 2]), Image.fromarray(labels[k % 2])), val)
                ops.append(record({"op": op.__name__, "m": m, "seed": seed, "image": k % 2, "negated": negate,
                                   "random_after": random.random()}, pair))
                k += 1

    # the drawn program of a chain: every operation of the module wrapped so that it notes its name and the value it was
    # called with; the sign is the draw the operation itself makes, repeated here from the same generator state
    log = []

    def wrap(f):
        def g(pair, v):
            signed = v
            if f.__name__ in SIGNED:
                state = random.getstate()
                signed = -v if random.random() > 0.5 else v
                random.setstate(state)
                if f.__name__ == "TranslateX":
                    signed = signed * pair[0].size[0]
                if f.__name__ == "TranslateY":
                    signed = signed * pair[0].size[1]
            if f.__name__ == "Posterize":
                signed = int(v)
            log.append([f.__name__, signed])
            return f(pair, v)
        g.__name__ = f.__name__
        return g

    chains = []
    for c, (n, m) in enumerate(CHAINS):
        for s in range(8):
            seed = 100 * c + s
            t = ra.RandAugment(n, m)
            t.augment_list = [(wrap(f), lo, hi) for f, lo, hi in t.augment_list]
            del log[:]
            random.seed(seed)
            pair = t(Image.fromarray(images[s % 2]), Image.fromarray(labels[s % 2]))
            chains.append(record({"n": n, "m": m, "seed": seed, "image": s % 2, "program": list(log),
                                  "random_after": random.random()}, pair))
    meta = {"pillow": Image.__version__, "numpy": np.__version__, "ignore_label": fill, "ops": ops, "chains": chains}
    path = os.path.join(HERE, "randaugment_golden.npz")
    np.savez_compressed(path, images=images, labels=labels, out_images=np.stack(out_i.arrays),
                        out_labels=np.stack(out_l.arrays), meta=np.array(json.dumps(meta)))
    print("ops", len(ops), "chains", len(chains), "image outputs", len(out_i.arrays), "label outputs", len(out_l.arrays),
          "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
