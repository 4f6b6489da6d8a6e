#!/usr/bin/env python
"""What the label half of the auto-labelled coarse data path (csrc/autolabel.hip, semseg_amd/datasets/autolabel.py) costs,
in ONE process on one GPU, for one 1024 x 2048 item of the headline recipe (Cityscapes ids, boost classes 14, 15, 16, the
drop mask, CUSTOM_COARSE_PROB 0.5; labels in blocks of 37 pixels with specks):

  kernel       ssa_autolabel_u8 through prepare_labels, both modes: its four launches (clear, pair presence, resolve,
               apply) and the three workspace / output allocations of the call
  launches     the device time of each of the four kernels, read off torch.profiler's kernel records over --reps calls
               (null where the profiler reports no kernels)
  copy         a device copy of the same bytes (copy_ of H * W bytes reads and writes them)
  host_loop    the reference's arithmetic on one host core: the drop mask, one whole-image pass per label id with the
               gtCoarse merge, the float64 threshold (datasets/base_loader.py:172-183, 216-223)
  decode       the three PNGs alone;  h2d: the three host-to-device copies alone (pageable memory)
  read_labels  read_labels end to end: path decisions, three decodes, three copies, the four launches

kernel and copy: device events around --reps back-to-back calls, alternating inside every round, --rounds rounds (at
least 5) after a warm-up; the host paths: a host clock, the device synchronised before it stops; median and half the
range.  Writes --out (default profiles/autolabel_bench.json) and prints one JSON line.

    python tools/autolabelbench.py [--rounds 7] [--reps 50] [--out FILE]               needs a GPU"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOF = 8.0e12
CITY = {i: t for i, t in zip(range(34), [255] * 7 + [0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255] + list(range(6, 16)) +
                             [255, 255, 16, 17, 18])}
BOOST = [14, 15, 16]
H, W = 1024, 2048
PROB = 0.5


def make(seed, values, specks):
    rng = np.random.RandomState(seed)
    grid = np.asarray(values, dtype=np.uint8)[rng.randint(0, len(values), ((H + 36) // 37, (W + 36) // 37))]
    m = np.ascontiguousarray(np.repeat(np.repeat(grid, 37, 0), 37, 1)[:H, :W])
    m[rng.randint(0, H, 500), rng.randint(0, W, 500)] = specks
    return m


def host_loop(o, g, p):
    """The reference's arithmetic, statement for statement, on one core."""
    drop = np.zeros((1024, 2048))
    drop[15:840, 14:2030] = 1.0
    mask = (drop * o).copy()
    for k, v in CITY.items():
        hit = (mask == k)
        if v in BOOST and hit.sum() > 0:
            hit += (g == k)
            hit[hit >= 1] = 1
            mask[hit] = g[hit]
        mask[hit] = v
    mask = mask.astype(np.uint8)
    mask[(p / 255.0) < PROB] = 255
    return mask


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summary(ts):
    return {"median_us": statistics.median(ts) * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6,
            "spread_us": (max(ts) - min(ts)) * 0.5e6, "rounds_us": [round(t * 1e6, 2) for t in ts]}


def per_launch(fn, reps):
    """{kernel: mean device microseconds} of the four kernels over reps calls, or None."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            for key in ("clear", "pairs", "resolve", "apply"):
                if "autolabel_%s_kernel" % key in e.key:
                    t = getattr(e, "device_time_total", None)
                    t = getattr(e, "cuda_time_total", 0.0) if t is None else t
                    out[key] = {"mean_us": t / max(e.count, 1), "count": e.count}
        return out or None
    except Exception as e:      # noqa: BLE001  (a profiler that cannot trace this process is not the tool's business)
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "autolabel_bench.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five rounds"
    if not torch.cuda.is_available():
        sys.exit("tools/autolabelbench.py needs a GPU")
    from PIL import Image
    from semseg_amd.config import cfg
    from semseg_amd.datasets import label_steps, prepare_labels, prob_cut, read_labels
    from semseg_amd.datasets.autolabel import DROP_MASK_WINDOW
    ids = [0, 7, 8, 11, 24, 26, 27, 28, 31, 33]
    o, g = make(1, ids, 27), make(2, ids, 28)
    p = make(3, [0, 60, 126, 127, 128, 129, 200, 255], 90)
    work = tempfile.mkdtemp()
    cc, cs = os.path.join(work, "autolabelled"), os.path.join(work, "cityscapes")
    label_fn = os.path.join(cc, "refinement", "city", "a_leftImg8bit.png")
    coarse_fn = os.path.join(cs, "gtCoarse", "gtCoarse", "refinement", "city", "a_gtCoarse_labelIds.png")
    prob_fn = label_fn.replace(".png", "_prob.png")
    for fn, m in ((label_fn, o), (coarse_fn, g), (prob_fn, p)):
        os.makedirs(os.path.dirname(fn), exist_ok=True)
        Image.fromarray(m).save(fn)
    cfg.DATASET.update(CITYSCAPES_CUSTOMCOARSE=cc, CITYSCAPES_DIR=cs, MASK_OUT_CITYSCAPES=True, CUSTOM_COARSE_PROB=PROB)
    cfg.DROPOUT_COARSE_BOOST_CLASSES = BOOST
    steps, cut = label_steps(CITY, BOOST), prob_cut(PROB)
    d_o, d_g, d_p = (torch.from_numpy(m).cuda() for m in (o, g, p))
    dst = torch.empty_like(d_o)
    want = host_loop(o, g, p)
    got = read_labels(label_fn, CITY)
    assert np.array_equal(got.cpu().numpy(), want), "read_labels differs from the reference's arithmetic"
    loader = lambda: prepare_labels(d_o, d_g, d_p, steps, "current", window=DROP_MASK_WINDOW, prob_cut=cut)   # noqa: E731
    paths = {"kernel_current": loader,
             "kernel_original": lambda: prepare_labels(d_o, d_g, None, steps, "original"),
             "copy": lambda: dst.copy_(d_o)}
    hosts = {"decode": lambda: [np.array(Image.open(fn)) for fn in (label_fn, coarse_fn, prob_fn)],
             "h2d": lambda: [torch.from_numpy(m).cuda() for m in (o, g, p)],
             "read_labels": lambda: read_labels(label_fn, CITY)}
    for fn in paths.values():                           # warm-up: code objects, allocator
        events(fn, 3)
    for fn in hosts.values():
        clock(fn)
    times = {k: [] for k in list(paths) + list(hosts)}
    for _ in range(a.rounds):                           # alternating
        for k, fn in paths.items():
            times[k].append(events(fn, a.reps))
        for k, fn in hosts.items():
            times[k].append(clock(fn))
    times["host_loop"] = [clock(lambda: host_loop(o, g, p)) for _ in range(3)]
    rec = {k: summary(v) for k, v in times.items()}
    rec["launches_current"] = per_launch(loader, a.reps)
    n = H * W
    t = rec["kernel_current"]["median_us"] * 1e-6
    rec["label_bytes"] = n
    rec["kernel_bytes"] = 6 * n                         # o and g twice, p once, one store
    rec["kernel_bytes_per_s"] = 6 * n / t
    rec["kernel_share_of_roof"] = 6 * n / t / ROOF
    rec["copy_bytes_per_s"] = 2 * n / (rec["copy"]["median_us"] * 1e-6)
    rec["kernel_rate_over_copy_rate"] = rec["kernel_bytes_per_s"] / rec["copy_bytes_per_s"]
    rec["kernel_over_copy"] = rec["kernel_current"]["median_us"] / rec["copy"]["median_us"]
    rec["host_loop_over_kernel"] = rec["host_loop"]["median_us"] / rec["kernel_current"]["median_us"]
    rec["host_loop_over_read_labels"] = rec["host_loop"]["median_us"] / rec["read_labels"]["median_us"]
    rec["decode_share_of_read_labels"] = rec["decode"]["median_us"] / rec["read_labels"]["median_us"]
    result = {"device": torch.cuda.get_device_name(0), "roof_bytes_per_s": ROOF, "reps": a.reps, "shape": [H, W],
              "n_steps": len(steps) // 3, "prob_cut": cut, "item": rec}
    print(json.dumps(rec, indent=1))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"autolabelbench": {k: rec[k]["median_us"] for k in ("kernel_current", "kernel_original", "copy", "host_loop",
                                                                         "decode", "h2d", "read_labels")}}))


if __name__ == "__main__":
    main()
