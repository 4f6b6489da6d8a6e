#!/usr/bin/env python
"""What ColorJitter costs on the device per training image, in ONE process on one GPU: a 1024 x 2048 crop of a
1024 x 2048 RGB frame, mirrored, under a four-operation program (saturation, brightness, contrast, hue), through the
C ABI with preallocated outputs, by device events:

  (i)   ssa_image_u8_crop_flip_normalize alone -- the input tail without the augmentation
  (ii)  ssa_jitter_luma_sum + ssa_jitter_crop_flip_normalize -- what crop_flip_normalize(..., jitter=p) launches
  (iii) ssa_jitter_luma_sum + ssa_jitter_apply_u8 + ssa_image_u8_crop_flip_normalize -- color_jitter() then the tail
  (iv)  where Pillow is importable: ImageEnhance.Color / Brightness / Contrast and the HSV round trip on one host core

With RandomGaussianBlur (--gblur) the same measurement on a 1024 x 1024 window at (901, 577) of a 2177 x 2903 frame, mirrored,
at sigma 1.2999 (radius 5: the most taps and the widest halo), reported under gblur_* keys, and again at the median draw
0.725 (radius 3) under gblur_at_median_sigma:

  gblur_tail_alone              ssa_image_u8_crop_flip_normalize on that window
  gblur_tail_plus_blur          ssa_gblur_crop_flip_normalize without a program -- crop_flip_normalize(..., blur=b)
  gblur_jitter_blur_fused       ssa_jitter_luma_sum + ssa_gblur_crop_flip_normalize with the program -- (..., jitter=p, blur=b)
  gblur_jitter_then_blur        ssa_jitter_luma_sum + ssa_jitter_apply_u8 + ssa_gblur_crop_flip_normalize on its output
  gblur_scipy_one_core          where SciPy is importable: the restated reference blur (np.multiply(img, 1 / 255),
                                scipy.ndimage.gaussian_filter, * 255, astype(uint8)) of the same window on one host core

There is no threshold on any of these: every device row is reported beside gblur_tail_alone of the same run.

The paths alternate inside every round; a round times --reps back-to-back calls of one path between two events and
divides.  Writes (--out, default profiles/colorjitter_bench.json) the median over the rounds with the spread (half the
range), the algorithmic bytes of each path and the bytes/s they amount to.  The outputs of (ii) and (iii) are compared
bit for bit before anything is timed.

    python tools/jitterbench.py [--rounds 25] [--reps 20] [--out FILE]                 needs a GPU"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

H, W = 1024, 2048
ORDER = ("saturation", "brightness", "contrast", "hue")
FACTORS = dict(saturation=1.25, brightness=1.2, contrast=0.8, hue=-0.1)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": (max(ms) - min(ms)) / 2,
            "rounds_ms": [round(v, 5) for v in ms]}


def pillow_chain_ms(img, p, rounds=3):
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return None
    torch.set_num_threads(1)
    out = []
    for _ in range(rounds):
        pil = Image.fromarray(img)
        t0 = time.perf_counter()
        pil = ImageEnhance.Color(pil).enhance(p.saturation)
        pil = ImageEnhance.Brightness(pil).enhance(p.brightness)
        pil = ImageEnhance.Contrast(pil).enhance(p.contrast)
        h, s, v = pil.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h += np.uint8(p.hue_byte)
        pil = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def scipy_blur_ms(win_np, sigma, rounds=3):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    out = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        b = ndimage.gaussian_filter(np.multiply(win_np, 1. / 255, dtype=np.float64), [sigma, sigma, 0], mode="nearest",
                                    cval=0, truncate=4.0)
        b *= 255
        b.astype(np.uint8)
        out.append((time.perf_counter() - t0) * 1e3)
    return stats(out)


def timed(paths, rounds, reps):
    """Median-ready per-call times of every path: the paths alternate inside every round, --reps calls between two events."""
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


GB_SRC, GB_WIN, GB_SIGMA, GB_MEDIAN_SIGMA = (2177, 2903), (901, 577, 1024, 1024), 1.2999, 0.725


def gblur_rows(a, L, pg, mean, std, sigma):
    """The gblur_* entries of the result at one sigma (see the module docstring)."""
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets import BlurParams
    from semseg_amd.datasets.transforms import _gblur_lut
    P = ctypes.c_void_p
    Hs, Ws = GB_SRC
    x0, y0, cw, ch = GB_WIN
    src_np = np.random.RandomState(1).randint(0, 256, (Hs, Ws, 3)).astype(np.uint8)
    src = torch.from_numpy(src_np).cuda()
    tp = BlurParams(sigma).taps()
    lut = _gblur_lut(src.device)
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    u8 = torch.empty((ch, cw, 3), dtype=torch.uint8, device="cuda")
    o_tail, o_blur, o_fused, o_two = (torch.empty((1, ch, cw, 16), dtype=hb.ACT_DTYPE, device="cuda") for _ in range(4))
    s = hb._s()
    win = (Hs, Ws, x0, y0, cw, ch)

    def tail_alone():
        _lib.check(L.ssa_image_u8_crop_flip_normalize(P(src.data_ptr()), *win, 1, mean, std, P(o_tail.data_ptr()), 16, s), "tail")

    def tail_plus_blur():
        _lib.check(L.ssa_gblur_crop_flip_normalize(P(src.data_ptr()), *win, 1, None, None, ctypes.byref(tp), P(lut.data_ptr()),
                                                   mean, std, P(o_blur.data_ptr()), 16, s), "blur tail")

    def jitter_blur_fused():
        _lib.check(L.ssa_jitter_luma_sum(P(src.data_ptr()), *win, ctypes.byref(pg), P(counter.data_ptr()), s), "luma")
        _lib.check(L.ssa_gblur_crop_flip_normalize(P(src.data_ptr()), *win, 1, ctypes.byref(pg), P(counter.data_ptr()),
                                                   ctypes.byref(tp), P(lut.data_ptr()), mean, std, P(o_fused.data_ptr()), 16, s),
                   "jitter + blur tail")

    def jitter_then_blur():
        _lib.check(L.ssa_jitter_luma_sum(P(src.data_ptr()), *win, ctypes.byref(pg), P(counter.data_ptr()), s), "luma")
        _lib.check(L.ssa_jitter_apply_u8(P(src.data_ptr()), *win, 1, ctypes.byref(pg), P(counter.data_ptr()), P(u8.data_ptr()), s),
                   "apply")
        _lib.check(L.ssa_gblur_crop_flip_normalize(P(u8.data_ptr()), ch, cw, 0, 0, cw, ch, 0, None, None, ctypes.byref(tp),
                                                   P(lut.data_ptr()), mean, std, P(o_two.data_ptr()), 16, s), "blur tail")

    paths = {"gblur_tail_alone": tail_alone, "gblur_tail_plus_blur": tail_plus_blur,
             "gblur_jitter_blur_fused": jitter_blur_fused, "gblur_jitter_then_blur": jitter_then_blur}
    times = timed(paths, a.rounds, a.reps)
    assert torch.equal(o_fused.view(torch.int16), o_two.view(torch.int16)), "fused and two-step jitter + blur differ"
    assert not torch.equal(o_blur.view(torch.int16), o_tail.view(torch.int16))
    n = cw * ch
    nbytes = {"gblur_tail_alone": n * (3 + 32), "gblur_tail_plus_blur": n * (3 + 32), "gblur_jitter_blur_fused": n * (3 + 3 + 32),
              "gblur_jitter_then_blur": n * (3 + 3 + 3 + 3 + 32)}
    res = {}
    for name in paths:
        st = stats(times[name])
        st["algorithmic_bytes"] = nbytes[name]
        st["bytes_per_s_at_median"] = nbytes[name] / (st["median_ms"] * 1e-3)
        st["over_gblur_tail_alone"] = st["median_ms"] / statistics.median(times["gblur_tail_alone"])
        res[name] = st
    res["gblur_setup"] = {"source": list(GB_SRC), "window": list(GB_WIN), "flip": True, "sigma": sigma, "radius": tp.radius}
    res["gblur_scipy_one_core"] = scipy_blur_ms(src_np[y0:y0 + ch, x0:x0 + cw], sigma)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorjitter_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "jitterbench needs a GPU"
    from semseg_amd import _lib, hip_backend as hb
    from semseg_amd.datasets import JitterParams
    from semseg_amd.datasets.transforms import MEAN_STD
    L = _lib.lib()
    P = ctypes.c_void_p
    img_np = np.random.RandomState(0).randint(0, 256, (H, W, 3)).astype(np.uint8)
    img = torch.from_numpy(img_np).cuda()
    p = JitterParams(ORDER, **FACTORS)
    pg = p.program()
    mean, std = (ctypes.c_float * 3)(*MEAN_STD[0]), (ctypes.c_float * 3)(*MEAN_STD[1])
    counter = torch.zeros(1, dtype=torch.int64, device="cuda")
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device="cuda")
    out_plain, out_fused, out_two = (torch.empty((1, H, W, 16), dtype=hb.ACT_DTYPE, device="cuda") for _ in range(3))
    s = hb._s()
    win = (H, W, 0, 0, W, H)

    def tail_alone():
        _lib.check(L.ssa_image_u8_crop_flip_normalize(P(img.data_ptr()), *win, 1, mean, std, P(out_plain.data_ptr()), 16, s), "tail")

    def fused_pair():
        _lib.check(L.ssa_jitter_luma_sum(P(img.data_ptr()), *win, ctypes.byref(pg), P(counter.data_ptr()), s), "luma")
        _lib.check(L.ssa_jitter_crop_flip_normalize(P(img.data_ptr()), *win, 1, ctypes.byref(pg), P(counter.data_ptr()), mean,
                                                    std, P(out_fused.data_ptr()), 16, s), "fused")

    def unfused():
        _lib.check(L.ssa_jitter_luma_sum(P(img.data_ptr()), *win, ctypes.byref(pg), P(counter.data_ptr()), s), "luma")
        _lib.check(L.ssa_jitter_apply_u8(P(img.data_ptr()), *win, 1, ctypes.byref(pg), P(counter.data_ptr()),
                                         P(u8.data_ptr()), s), "apply")
        _lib.check(L.ssa_image_u8_crop_flip_normalize(P(u8.data_ptr()), *win, 0, mean, std, P(out_two.data_ptr()), 16, s), "tail")

    paths = {"tail_alone": tail_alone, "luma_sum_plus_fused_apply": fused_pair, "unfused_u8_then_tail": unfused}
    for fn in paths.values():                      # once, for the comparison below (timed() warms up itself)
        fn()
    torch.cuda.synchronize()
    assert torch.equal(out_fused.view(torch.int16), out_two.view(torch.int16)), "fused and unfused outputs differ"
    assert not torch.equal(out_fused.view(torch.int16), out_plain.view(torch.int16))
    times = timed(paths, a.rounds, a.reps)
    n = H * W
    nbytes = {"tail_alone": n * (3 + 32), "luma_sum_plus_fused_apply": n * (3 + 3 + 32),
              "unfused_u8_then_tail": n * (3 + 3 + 3 + 3 + 32)}
    res = {"device": torch.cuda.get_device_name(0), "storage": _lib.ACT, "crop": [H, W], "program": list(ORDER),
           "factors": FACTORS, "timed_launch_groups_per_path": a.rounds * a.reps, "paths": {}}
    for name in paths:
        st = stats(times[name])
        st["algorithmic_bytes"] = nbytes[name]
        st["bytes_per_s_at_median"] = nbytes[name] / (st["median_ms"] * 1e-3)
        res["paths"][name] = st
    res["fused_over_tail_alone"] = res["paths"]["luma_sum_plus_fused_apply"]["median_ms"] / res["paths"]["tail_alone"]["median_ms"]
    res["unfused_over_fused"] = res["paths"]["unfused_u8_then_tail"]["median_ms"] / res["paths"]["luma_sum_plus_fused_apply"]["median_ms"]
    res["pillow_chain_one_core"] = pillow_chain_ms(img_np, p)
    res.update(gblur_rows(a, L, pg, mean, std, GB_SIGMA))
    res["gblur_at_median_sigma"] = gblur_rows(a, L, pg, mean, std, GB_MEDIAN_SIGMA)
    print(json.dumps(res, indent=1, sort_keys=True))
    if a.out != "/dev/null":
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
