#!/usr/bin/env python
"""What the boundary F-score (eval_mask_boundary, csrc/fboundary.hip) costs, in ONE process on one GPU:

  fboundary   boundary_counts: both boundary maps as four class bytes per pixel, then the match pass
  copy        a device copy of the bytes it must move: prediction (1 B) and int64 ground truth (8 B) read, two entries
              of 4 B written, each entry read once as a tile's own and once as the other map's (halo not counted):
              33 B per pixel (copy_(src) of n / 2 bytes moves n)
  torch       the device composition in torch: per class two boolean boundary maps, F.conv2d with the disk (in strips of
              128 rows through torch's own im2col + GEMM convolution, as tests/test_fboundary_gpu.py takes it)
  host        the reference's arithmetic (NumPy + scipy.ndimage, what tests/fboundary_ref.py states) on one host core,
              timed on --host-classes classes of the typical row and scaled to all C (an estimate, marked as such)

for 1 x 1024 x 2048 x 19 at radius 19 and 1 x 2177 x 2177 x 65 at radius 25.  Labels in 64 x 64 blocks with 5 % ignore.
Row `typical`: the prediction is the ground truth shifted by (3, -5) plus 3 % noise.  Row `adversarial`: an i.i.d. random
prediction, where every pixel is a boundary.  Device events around --reps back-to-back calls (one call for torch), the
paths alternating inside every round, --rounds rounds (at least 5) after a warm-up; median and half the range over the
rounds.  Writes --out (default profiles/fboundary_bench.json) and prints one JSON line.

    python tools/fboundarybench.py [--rounds 5] [--reps 10] [--host-classes 1] [--no-torch] [--out FILE]     needs a GPU"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from fboundary_torch import torch_composition  # noqa: E402  (the yardstick of tests/test_fboundary_gpu.py)

SHAPES = {"1x1024x2048x19_r19": (1, 1024, 2048, 19, 255, 19), "1x2177x2177x65_r25": (1, 2177, 2177, 65, 65, 25)}
BYTES_PER_PIXEL = 1 + 8 + 8 + 16


def make(B, H, W, C, ignore, adversarial):
    g = torch.Generator().manual_seed(C + B)
    gt = torch.randint(0, C, (B, (H + 63) // 64, (W + 63) // 64), generator=g)
    gt = gt.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :H, :W].clone()
    if adversarial:
        pred = torch.randint(0, C, (B, H, W), generator=g)
    else:
        pred = torch.roll(gt, (3, -5), (1, 2)).clone()
        noise = torch.rand(B, H, W, generator=g) < 0.03
        pred[noise] = torch.randint(0, C, (int(noise.sum()),), generator=g)
    gt[torch.rand(B, H, W, generator=g) < 0.05] = ignore
    return pred.to(torch.uint8).cuda(), gt.long().cuda()


def boundary_pixel_share(pred, gt, C, ignore):
    """share of the pixels that are a boundary pixel of some class (a 2 x 2 quad that is not uniform), per map; the
    last row and column, a sliver of these shapes, are left out"""
    ign = gt == ignore
    out = {}
    for key, lab in (("pred", pred.long()), ("gt", gt)):
        a = torch.where(ign | (lab < 0) | (lab >= C), torch.full_like(lab, -1), lab)
        q = (a[:, :-1, :-1] != a[:, :-1, 1:]) | (a[:, :-1, :-1] != a[:, 1:, :-1]) | (a[:, :-1, :-1] != a[:, 1:, 1:])
        out[key] = float(q.float().mean())
    return out


def host_one_core(pred, gt, classes, ignore, r):
    """seconds per class of the reference's arithmetic on this core"""
    import scipy.ndimage as ndi
    torch.set_num_threads(1)
    ax = np.arange(-r, r + 1)
    disk = ax[:, None] ** 2 + ax[None, :] ** 2 <= r * r

    def seg2bmap(seg):
        e, s, se = np.zeros_like(seg), np.zeros_like(seg), np.zeros_like(seg)
        e[:, :-1], s[:-1, :], se[:-1, :-1] = seg[:, 1:], seg[1:, :], seg[1:, 1:]
        b = seg ^ e | seg ^ s | seg ^ se
        b[-1, :], b[:, -1] = seg[-1, :] ^ e[-1, :], seg[:, -1] ^ s[:, -1]
        b[-1, -1] = 0
        return b
    p, g = pred[0].cpu().numpy(), gt[0].cpu().numpy()
    t0 = time.perf_counter()
    for c in range(classes):
        ign = g == ignore
        fg_b, gt_b = seg2bmap((p == c) & ~ign), seg2bmap((g == c) & ~ign)
        fg_d, gt_d = ndi.binary_dilation(fg_b, structure=disk), ndi.binary_dilation(gt_b, structure=disk)
        (gt_b & fg_d).sum(), (fg_b & gt_d).sum(), fg_b.sum(), gt_b.sum()
    return (time.perf_counter() - t0) / classes


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def summary(ts):
    return {"median_us": statistics.median(ts) * 1e6, "min_us": min(ts) * 1e6, "max_us": max(ts) * 1e6,
            "spread_us": (max(ts) - min(ts)) * 0.5e6, "rounds_us": [round(t * 1e6, 2) for t in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-classes", type=int, default=1)
    ap.add_argument("--no-torch", action="store_true", help="leave the torch composition out")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fboundary_bench.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five rounds"
    if not torch.cuda.is_available():
        sys.exit("tools/fboundarybench.py needs a GPU")
    from semseg_amd.utils import boundary_counts
    result = {"device": torch.cuda.get_device_name(0), "reps": a.reps, "bytes_per_pixel": BYTES_PER_PIXEL, "shapes": {}}
    for name, (B, H, W, C, ignore, r) in SHAPES.items():
        for row in ("typical", "adversarial"):
            pred, gt = make(B, H, W, C, ignore, row == "adversarial")
            nbytes = B * H * W * BYTES_PER_PIXEL
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            paths = {"fboundary": (lambda: boundary_counts(pred, gt, C, ignore, r), a.reps),
                     "copy": (lambda: dst.copy_(src), a.reps)}
            if not a.no_torch and row == "typical":
                paths["torch"] = (lambda: torch_composition(pred, gt, C, ignore, r), 1)
            for fn, _ in paths.values():                    # warm-up: code objects, allocator
                events(fn, 1)
            times = {k: [] for k in paths}
            for _ in range(a.rounds):                       # alternating
                for k, (fn, reps) in paths.items():
                    times[k].append(events(fn, reps))
            rec = {k: summary(v) for k, v in times.items()}
            counts = boundary_counts(pred, gt, C, ignore, r)
            if "torch" in paths:
                rec["equals_torch_composition"] = bool(torch.equal(counts, torch_composition(pred, gt, C, ignore, r)))
            c = counts.cpu()
            rec["entries_per_pixel"] = {"pred": float(c[..., 0].sum() / (B * H * W)), "gt": float(c[..., 1].sum() / (B * H * W))}
            rec["boundary_pixel_share"] = boundary_pixel_share(pred, gt, C, ignore)
            rec["bytes"] = nbytes
            rec["fboundary_over_copy"] = rec["fboundary"]["median_us"] / rec["copy"]["median_us"]
            if row == "typical" and a.host_classes > 0:
                per = host_one_core(pred, gt, min(a.host_classes, C), ignore, r)
                rec["host_one_core_estimate_s"] = per * C
                rec["host_classes_timed"] = min(a.host_classes, C)
            result["shapes"][name + "/" + row] = rec
            print(name, row, json.dumps(rec, indent=1), flush=True)
            del pred, gt, src, dst, paths
            torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"fboundarybench": {k: {"fboundary_us": v["fboundary"]["median_us"], "copy_us": v["copy"]["median_us"],
                                             "torch_us": v.get("torch", {}).get("median_us"),
                                             "host_one_core_estimate_s": v.get("host_one_core_estimate_s")}
                                         for k, v in result["shapes"].items()}}))


if __name__ == "__main__":
    main()
