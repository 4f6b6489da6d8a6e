#!/usr/bin/env python
"""What RandAugment costs on the device, in ONE process on one GPU: a 1024 x 1024 window at (901, 577) of a 2177 x 2903
RGB frame with its label map, mirrored, by device events:

  op:<name>      every operation of augment_list alone at m = 9 (the geometric ones negated), through the C ABI
                 (ssa_randaug_u8) with preallocated buffers; the five geometric ones with the labels, the others on the
                 image alone; AutoContrast / Equalize include the clearing of their histogram
  copy:image, copy:pair   a device-to-device copy (Tensor.copy_) of the bytes such an operation reads and writes: 3 B per
                 pixel in and out for the image, 4 B with the labels
  pillow:<name>  the same operation by Pillow on one host core (where Pillow is importable)
  chain_2_9      the chain RandAugment(2, 9).get_params draws after random.seed(--seed), through rand_augment()
  chain_jitter_tail   crop_flip_normalize(..., augment=that chain, jitter=a four-step program): chain + luma sum + tail

There is no threshold on any of these: each op row carries its ratio to the copy of the same bytes.  The paths alternate
inside every round; a round times --reps back-to-back calls of one path between two events and divides.  Writes (--out,
default profiles/randaugment_bench.json) the median over the rounds with the spread.  Every op's output is compared with
the NumPy restatement (tests/randaug_ref.py) on a 96 x 160 corner of the setup before anything is timed.

    python tools/randaugbench.py [--rounds 25] [--reps 20] [--out FILE]                 needs a GPU"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

SRC, WIN = (2177, 2903), (901, 577, 1024, 1024)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": (max(ms) - min(ms)) / 2,
            "rounds_ms": [round(v, 5) for v in ms]}


def timed(paths, rounds, reps):
    for fn in paths.values():                      # warm-up: code objects, allocator
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(rounds):
        for name, fn in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / reps)
    return times


def pillow_ms(img, lab, op, v, rounds=3):
    try:
        from PIL import Image, ImageEnhance, ImageOps
    except ImportError:
        return None
    import randaug_ref as R
    out = []
    for _ in range(rounds):
        pi, pl = Image.fromarray(img), Image.fromarray(lab)
        t0 = time.perf_counter()
        if op in ("ShearX", "ShearY", "TranslateX", "TranslateY"):
            a = R.matrix_of(op, v, *pi.size)
            pi.transform(pi.size, Image.AFFINE, a, resample=Image.BILINEAR, fillcolor=(0, 0, 0))
            pl.transform(pl.size, Image.AFFINE, a, resample=Image.NEAREST, fillcolor=255)
        elif op == "Rotate":
            pi.rotate(v, fillcolor=(0, 0, 0))
            pl.rotate(v, resample=Image.NEAREST, fillcolor=255)
        else:
            {"Identity": lambda: pi, "AutoContrast": lambda: ImageOps.autocontrast(pi), "Invert": lambda: ImageOps.invert(pi),
             "Equalize": lambda: ImageOps.equalize(pi), "Solarize": lambda: ImageOps.solarize(pi, v),
             "Posterize": lambda: ImageOps.posterize(pi, int(v)), "Color": lambda: ImageEnhance.Color(pi).enhance(v),
             "Brightness": lambda: ImageEnhance.Brightness(pi).enhance(v),
             "Sharpness": lambda: ImageEnhance.Sharpness(pi).enhance(v)}[op]()
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "randaugment_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "randaugbench needs a GPU"
    import randaug_cases as K
    import randaug_ref as R
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets import AugmentParams, JitterParams, RandAugment, crop_flip_normalize, rand_augment
    L = _lib.lib()
    P = hb._p
    Hs, Ws = SRC
    x0, y0, cw, ch = WIN
    n = cw * ch
    rng = np.random.RandomState(1)
    src_np = rng.randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    lab_np = R.label_map(Hs, Ws, 2)
    src, lab = torch.from_numpy(src_np).cuda(), torch.from_numpy(lab_np).cuda()
    out, tmp = (torch.empty((ch, cw, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    lout, ltmp = (torch.empty((ch, cw), dtype=torch.uint8, device="cuda") for _ in range(2))
    hist = torch.zeros((768,), dtype=torch.int32, device="cuda")
    c3a, c3b = (torch.empty((n * 3,), dtype=torch.uint8, device="cuda") for _ in range(2))
    c4a, c4b = (torch.empty((n * 4,), dtype=torch.uint8, device="cuda") for _ in range(2))
    s = hb._s()

    programs = {op: [(op, K.signed_value(op, 9, True, cw, ch))] for op in R.OPS}
    # every op against the restatement on a small corner of the same setup, before anything is timed
    small = (901, 577, 160, 96)
    for op in R.OPS:
        program = [(op, K.signed_value(op, 9, True, 160, 96))]
        gi, gl = rand_augment(src, lab, AugmentParams(program, (160, 96)), small, True)
        wi, wl = R.augment(src_np, lab_np, program, small, True)
        assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gl.cpu().numpy(), wl), op

    def op_path(op):
        pg = AugmentParams(programs[op], (cw, ch)).program()
        geo = op in R.GEOMETRIC
        table = op in ("AutoContrast", "Equalize")

        def fn():
            if table:
                hist.zero_()
            _lib.check(L.ssa_randaug_u8(P(src), P(lab) if geo else None, Hs, Ws, x0, y0, cw, ch, 1, ctypes.byref(pg), 255,
                                        P(hist), P(out), P(tmp), P(lout) if geo else None, P(ltmp) if geo else None, s), op)
        return fn

    paths = {"copy:image": lambda: c3b.copy_(c3a), "copy:pair": lambda: c4b.copy_(c4a)}
    for op in R.OPS:
        paths["op:" + op] = op_path(op)
    random.seed(a.seed)
    chain = RandAugment(2, 9).get_params((cw, ch))
    jitter = JitterParams(("saturation", "brightness", "contrast", "hue"), saturation=1.25, brightness=1.2, contrast=0.8,
                          hue=-0.1)
    paths["chain_2_9"] = lambda: rand_augment(src, lab, chain, WIN, True)
    paths["chain_jitter_tail"] = lambda: crop_flip_normalize(src, lab, WIN, True, jitter=jitter, augment=chain)
    paths["jitter_tail_alone"] = lambda: crop_flip_normalize(src, lab, WIN, True, jitter=jitter)
    times = timed(paths, a.rounds, a.reps)
    res = {"setup": {"source": list(SRC), "window": list(WIN), "flip": True, "m": 9, "chain": chain.ops,
                     "rounds": a.rounds, "reps": a.reps, "device": torch.cuda.get_device_name(0)}}
    for name in paths:
        st = stats(times[name])
        if name.startswith("op:"):
            op = name[3:]
            base = "copy:pair" if op in R.GEOMETRIC else "copy:image"
            st["bytes"] = n * (8 if op in R.GEOMETRIC else 6)
            st["copy"] = base
            st["over_copy"] = st["median_ms"] / statistics.median(times[base])
        res[name] = st
    win_np = np.ascontiguousarray(src_np[y0:y0 + ch, x0:x0 + cw][:, ::-1])
    wlab_np = np.ascontiguousarray(lab_np[y0:y0 + ch, x0:x0 + cw][:, ::-1])
    for op in R.OPS:
        res["pillow:" + op] = pillow_ms(win_np, wlab_np, op, programs[op][0][1])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    for name in paths:
        print("%-22s %8.4f ms  +- %.4f%s" % (name, res[name]["median_ms"], res[name]["spread_ms"],
                                              "   x%.2f of %s" % (res[name]["over_copy"], res[name]["copy"])
                                              if "over_copy" in res[name] else ""))
    for op in R.OPS:
        if res["pillow:" + op]:
            print("pillow:%-15s %8.3f ms" % (op, res["pillow:" + op]["median_ms"]))


if __name__ == "__main__":
    main()
