#!/usr/bin/env python
"""What the centroid pass of class-uniform sampling (--class_uniform_pct, csrc/centroids.hip) costs, in ONE process on
one GPU, per label map:

  kernel      ssa_class_centroids_u8: the clearing launch, the pass over the label bytes and the finalize launch
  copy        a device copy of the same bytes (copy_ of H * W bytes reads and writes them: twice the pass's traffic)
  host_loop   the reference's per-image loop on one host core: per tile and class `class_id in patch`,
              `(patch == class_id).astype(int)` and scipy.ndimage.center_of_mass (datasets/uniform.py:123-133)
  decode      np.array(Image.open(label.png)) alone
  h2d         the host-to-device copy of the decoded map alone (pageable memory, as class_centroids_image sends it)
  image_path  class_centroids_image end to end: decode, copy, the three launches, the copy back and the dict

for a 1024 x 2048 map with 19 classes behind a 34-entry id table (Cityscapes) and a 3000 x 4000 map with 65 classes
(Mapillary), tile 1024, labels in blocks of 37 pixels with specks.  kernel and copy: device events around --reps
back-to-back calls, alternating inside every round, --rounds rounds (at least 5) after a warm-up; the host paths: a host
clock, the device synchronised before it stops; median and half the range.  Writes --out (default
profiles/centroids_bench.json) and prints one JSON line.

    python tools/centroidbench.py [--rounds 7] [--reps 50] [--out FILE]               needs a GPU"""
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
SHAPES = {"1024x2048_c19_lut": (1024, 2048, 19, CITY, 34), "3000x4000_c65": (3000, 4000, 65, None, 66)}
TILE = 1024


def make(H, W, n_values, seed):
    rng = np.random.RandomState(seed)
    grid = rng.randint(0, n_values, ((H + 36) // 37, (W + 36) // 37)).astype(np.uint8)
    m = np.ascontiguousarray(np.repeat(np.repeat(grid, 37, 0), 37, 1)[:H, :W])
    m[rng.randint(0, H, 500), rng.randint(0, W, 500)] = 3
    return m


def host_loop(mask, tile, C, id2trainid):
    """The reference's arithmetic, statement for statement, on one core."""
    from scipy.ndimage import center_of_mass
    mask = mask.copy()
    original = mask.copy()
    for k, v in (id2trainid or {}).items():
        mask[original == k] = v
    found = 0
    for y in range(mask.shape[0] // tile):
        for x in range(mask.shape[1] // tile):
            patch = mask[y * tile:(y + 1) * tile, x * tile:(x + 1) * tile]
            for c in range(C):
                if c in patch:
                    cy, cx = center_of_mass((patch == c).astype(int))
                    found += int(cx) + int(cy) >= 0
    return found


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centroids_bench.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five rounds"
    if not torch.cuda.is_available():
        sys.exit("tools/centroidbench.py needs a GPU")
    from PIL import Image
    from semseg_amd.datasets import class_centroids, class_centroids_image
    result = {"device": torch.cuda.get_device_name(0), "roof_bytes_per_s": ROOF, "reps": a.reps, "tile": TILE, "shapes": {}}
    work = tempfile.mkdtemp()
    for name, (H, W, C, id2trainid, n_values) in SHAPES.items():
        mask = make(H, W, n_values, C)
        label_fn = os.path.join(work, name + ".png")
        Image.fromarray(mask).save(label_fn)
        item = (name + "_image.png", label_fn)
        lab = torch.from_numpy(mask).cuda()
        dst = torch.empty_like(lab)
        paths = {"kernel": lambda: class_centroids(lab, TILE, C, id2trainid), "copy": lambda: dst.copy_(lab)}
        hosts = {"decode": lambda: np.array(Image.open(label_fn)), "h2d": lambda: torch.from_numpy(mask).cuda(),
                 "image_path": lambda: class_centroids_image(item, TILE, C, id2trainid)}
        for fn in paths.values():                       # warm-up: code objects, allocator, the id table
            events(fn, 3)
        for fn in hosts.values():
            clock(fn)
        times = {k: [] for k in list(paths) + list(hosts)}
        for _ in range(a.rounds):                       # alternating
            for k, fn in paths.items():
                times[k].append(events(fn, a.reps))
            for k, fn in hosts.items():
                times[k].append(clock(fn))
        times["host_loop"] = [clock(lambda: host_loop(mask, TILE, C, id2trainid)) for _ in range(3)]
        rec = {k: summary(v) for k, v in times.items()}
        n_bytes = H * W
        t = rec["kernel"]["median_us"] * 1e-6
        rec["label_bytes"] = n_bytes
        rec["tiles"] = (H // TILE) * (W // TILE)
        rec["counted_bytes"] = rec["tiles"] * TILE * TILE          # what lies in no full tile is never read
        rec["kernel_bytes_per_s"] = rec["counted_bytes"] / t
        rec["kernel_share_of_roof"] = rec["counted_bytes"] / t / ROOF
        rec["copy_bytes_per_s"] = 2 * n_bytes / (rec["copy"]["median_us"] * 1e-6)
        rec["kernel_over_copy"] = rec["kernel"]["median_us"] / rec["copy"]["median_us"]
        rec["host_loop_over_kernel"] = rec["host_loop"]["median_us"] / rec["kernel"]["median_us"]
        rec["host_loop_over_image_path"] = rec["host_loop"]["median_us"] / rec["image_path"]["median_us"]
        rec["decode_share_of_image_path"] = rec["decode"]["median_us"] / rec["image_path"]["median_us"]
        result["shapes"][name] = rec
        print(name, json.dumps(rec, indent=1))
        del lab, dst, paths, hosts
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"centroidbench": {k: {p: v[p]["median_us"] for p in ("kernel", "copy", "host_loop", "decode", "h2d",
                                                                          "image_path")}
                                        for k, v in result["shapes"].items()}}))


if __name__ == "__main__":
    main()
