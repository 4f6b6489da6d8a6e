#!/usr/bin/env python
"""What the label relaxation criterion (--jointwtborder, csrc/relax_loss.hip) costs, in ONE process on one GPU:

  relax_fwd_bwd   RelaxNllFn forward + backward from int64 label maps: class sets + counts, class weights, the loss,
                  finalize, and the backward recomputed from the logits
  relax_fwd       its forward alone
  ce_fwd_bwd      CrossEntropyFn forward + backward on the SAME logits and labels
  copy            a device copy of the bytes the relaxation pass must move: the logits read by the forward, read again
                  and the gradient written by the backward, 16 B of class sets per pixel written once and read twice
                  (copy_(src) of n / 2 bytes moves n)

for 1 x 1024 x 1024 x 19, 2 x 1024 x 1024 x 19 and 1 x 1024 x 1024 x 65 (labels in 64 x 64 blocks, 5 % ignore).  Device
events around --reps back-to-back calls, the four paths alternating inside every round, --rounds rounds (at least 5)
after a warm-up of every shape; median and half the range over the rounds.  Writes --out (default
profiles/relaxloss_bench.json) and prints one JSON line.

    python tools/relaxbench.py [--rounds 7] [--reps 20] [--out FILE]               needs a GPU
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/relaxbench.py --rounds 5 --out /dev/null"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

ROOF = 8.0e12
SHAPES = {"1x1024x1024x19": (1, 1024, 1024, 19, 255), "2x1024x1024x19": (2, 1024, 1024, 19, 255),
          "1x1024x1024x65": (1, 1024, 1024, 65, 65)}


def make(B, H, W, C, ignore):
    g = torch.Generator().manual_seed(C + B)
    x = (torch.randn(B, H, W, C, generator=g) * 2.0).cuda().requires_grad_(True)
    lab = torch.randint(0, C, (B, H // 64, W // 64), generator=g).repeat_interleave(64, 1).repeat_interleave(64, 2).clone()
    lab[torch.rand(B, H, W, generator=g) < 0.05] = ignore
    return x, lab.long().cuda()


def bytes_moved(B, H, W, C):
    """the relaxation's forward + backward: labels read, sets written, then (logits + sets) read twice, gradient written"""
    P = B * H * W
    logits, sets = P * C * 4, P * 16
    return {"labels_read": P * 8, "sets_written": sets, "sets_read": 2 * B * sets, "logits_read": 2 * logits,
            "grad_written": logits, "total": P * 8 + sets + 2 * B * sets + 3 * logits}


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relaxloss_bench.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five rounds"
    if not torch.cuda.is_available():
        sys.exit("tools/relaxbench.py needs a GPU")
    from semseg_amd import hip_backend as hb
    result = {"device": torch.cuda.get_device_name(0), "roof_bytes_per_s": ROOF, "reps": a.reps, "shapes": {}}
    for name, (B, H, W, C, ignore) in SHAPES.items():
        x, lab = make(B, H, W, C, ignore)
        up = torch.ones((), device="cuda")
        nb = bytes_moved(B, H, W, C)
        src = torch.empty(nb["total"] // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)

        def relax(backward=True):
            loss = hb.RelaxNllFn.apply(x, lab, C, ignore, 1, None, 1.0, False)[0]
            if backward:
                torch.autograd.grad(loss, x, up)

        def ce():
            torch.autograd.grad(hb.CrossEntropyFn.apply(x, lab, ignore), x, up)

        paths = {"relax_fwd_bwd": relax, "relax_fwd": lambda: relax(False), "ce_fwd_bwd": ce,
                 "copy": lambda: dst.copy_(src)}
        for fn in paths.values():                       # warm-up: code objects, allocator, LDS limits
            events(fn, 3)
        times = {k: [] for k in paths}
        for _ in range(a.rounds):                       # alternating
            for k, fn in paths.items():
                times[k].append(events(fn, a.reps))
        rec = {k: summary(v) for k, v in times.items()}
        rec["bytes"] = nb
        t = rec["relax_fwd_bwd"]["median_us"] * 1e-6
        rec["relax_bytes_per_s"] = nb["total"] / t
        rec["relax_share_of_roof"] = nb["total"] / t / ROOF
        rec["copy_bytes_per_s"] = nb["total"] / (rec["copy"]["median_us"] * 1e-6)
        rec["relax_over_ce"] = rec["relax_fwd_bwd"]["median_us"] / rec["ce_fwd_bwd"]["median_us"]
        rec["relax_over_copy"] = rec["relax_fwd_bwd"]["median_us"] / rec["copy"]["median_us"]
        result["shapes"][name] = rec
        print(name, json.dumps(rec, indent=1))
        del x, lab, src, dst, paths
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"relaxbench": {k: {"relax_fwd_bwd_us": v["relax_fwd_bwd"]["median_us"],
                                         "relax_fwd_us": v["relax_fwd"]["median_us"],
                                         "ce_fwd_bwd_us": v["ce_fwd_bwd"]["median_us"], "copy_us": v["copy"]["median_us"],
                                         "relax_over_ce": v["relax_over_ce"]} for k, v in result["shapes"].items()}}))


if __name__ == "__main__":
    main()
