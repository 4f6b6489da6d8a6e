#!/usr/bin/env python
"""What the tail of eval_minibatch costs per validation image, four ways, in ONE process on one GPU:

  (i)   the reference's tail restated on the same device tensors (utils/trnval_utils.py:116-196): flip by index gather,
        add, two divisions, CrossEntropyLoss2d, softmax(output).cpu(), max(1) on the host, numpy error mask and bincount
  (ii)  the best the package offered before ssa_eval_tail: torch.flip + add + divide, this package's CrossEntropyLoss2d,
        confusion_matrix(..., return_predictions=True), softmax().max(1) for the probability, small results to the host
  (iii) semseg_amd.utils.eval_tail including its host copies (what eval_minibatch does after the last net(...))
  (iv)  the ssa_eval_tail kernel alone, by device events

for (a) 1 x 19 x 1024 x 2048 (Cityscapes) and (b) 1 x 65 x 1632 x 2177 (Mapillary): two sources, the first mirrored,
labels with 10 % ignore.  The paths alternate inside every round; every timed section starts from an idle host (a
quarter second of sleep) and ends in a synchronise.  Prints
and writes (--out, default profiles/evaltail_bench.json) the times with their spread (half the range over the
rounds), the algorithmic bytes of the kernel (n_src P C 4 + 8 P read, 6 P written), the bytes/s it reaches and their
share of the 8 TB/s roof, and whether (iii) beats (i) and (ii) by more than three spreads.

    python tools/evaltail_bench.py [--rounds 7] [--out FILE]                       needs a GPU
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/evaltail_bench.py --rounds 5 --out /dev/null"""
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
import torch.nn.functional as F  # noqa: E402

ROOF = 8.0e12
SHAPES = {"cityscapes_19x1024x2048": (19, 1024, 2048, 255), "mapillary_65x1632x2177": (65, 1632, 2177, 65)}


def make(C, H, W, ignore):
    g = torch.Generator().manual_seed(C)
    srcs = [(torch.randn(1, H, W, C, generator=g) * 3.0).cuda().permute(0, 3, 1, 2) for _ in range(2)]   # NHWC buffers
    gts = torch.randint(0, C, (1, H, W), generator=g)
    gts[torch.rand(1, H, W, generator=g) < 0.1] = ignore
    return srcs, gts.long()


def reference_tail(srcs, gts_host, gts_dev, C, ignore):
    a, b = srcs
    idx = torch.arange(a.size(3) - 1, -1, -1).long()
    output = 0.0
    output = output + a[:, :, :, idx]
    output = output + b
    output = output / 1 / 2
    loss = F.nll_loss(F.log_softmax(output, dim=1), gts_dev, ignore_index=ignore).item()
    output_data = F.softmax(output, dim=1).cpu().data
    max_probs, predictions = output_data.max(1)
    predictions = predictions.numpy()
    g = gts_host.numpy()
    err = ((g >= 0) & (g != ignore) & (predictions != g)).astype(int)
    p, gf = predictions.flatten(), g.flatten()
    mask = (gf >= 0) & (gf < C)
    hist = np.bincount(C * gf[mask].astype(int) + p[mask], minlength=C ** 2).reshape(C, C)
    torch.cuda.synchronize()
    return predictions, max_probs, err, hist, loss


def parent_tail(srcs, gts_dev, C, ignore, criterion):
    from semseg_amd.utils import confusion_matrix
    a, b = srcs
    output = (torch.flip(a, (3,)) + b) / 2
    loss = criterion(output, gts_dev)
    hist, pred = confusion_matrix(output, gts_dev, C, return_predictions=True)
    prob = F.softmax(output, dim=1).max(1)[0]
    err = ((gts_dev >= 0) & (gts_dev != ignore) & (pred != gts_dev)).to(torch.uint8)
    out = [t.cpu() for t in (pred, prob, err, hist, loss)]
    torch.cuda.synchronize()
    return out


def new_tail(srcs, gts_dev, C, ignore):
    from semseg_amd.utils.eval_tail import eval_tail, _to_host
    r = eval_tail(srcs, [1, 0], C, gts=gts_dev, ignore_label=ignore, n_scales=1, n_flips=2)
    out = _to_host([r.pred, r.prob, r.err, r.hist, r.loss_acc])
    torch.cuda.synchronize()
    return out


class KernelOnly:
    def __init__(self, srcs, gts_dev, C, ignore):
        from semseg_amd import _lib
        self.L = _lib.lib()
        self.srcs = [s.permute(0, 2, 3, 1) for s in srcs]
        assert all(s.is_contiguous() for s in self.srcs)
        _, H, W, _ = self.srcs[0].shape
        dev = gts_dev.device
        self.keep = (gts_dev, torch.empty((H, W), dtype=torch.uint8, device=dev), torch.empty((H, W), device=dev),
                     torch.empty((H, W), dtype=torch.uint8, device=dev), torch.zeros((C, C), dtype=torch.int64, device=dev),
                     torch.zeros(2, dtype=torch.float64, device=dev))
        P = ctypes.c_void_p
        self.args = ((P * 2)(*[s.data_ptr() for s in self.srcs]), (ctypes.c_int * 2)(1, 0), 2, C, 1, H, W, C,
                     P(gts_dev.data_ptr()), ignore, 1.0, 2.0) + tuple(P(t.data_ptr()) for t in self.keep[1:]) + (None,)

    def run(self, reps=5):
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            rc = self.L.ssa_eval_tail(*self.args, stream)
            assert rc == 0, rc
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps


def summary(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "spread_ms": (max(ts) - min(ts)) * 0.5e3, "rounds_ms": [round(t * 1e3, 4) for t in ts]}


def timed(fn):
    # from an idle host: the reference path before it ran 16 CPU threads for 50-250 ms; the quarter second lets their
    # spinning workers go to sleep and a CPU quota refill, which otherwise stretch the next (host-light) path's launches
    torch.cuda.synchronize()
    time.sleep(0.25)
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "evaltail_bench.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five rounds"
    if not torch.cuda.is_available():
        sys.exit("tools/evaltail_bench.py needs a GPU")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    from semseg_amd.loss.criteria import CrossEntropyLoss2d
    result = {"device": torch.cuda.get_device_name(0), "roof_bytes_per_s": ROOF, "shapes": {}}
    for name, (C, H, W, ignore) in SHAPES.items():
        srcs, gts = make(C, H, W, ignore)
        gd = gts.cuda()
        crit = CrossEntropyLoss2d(ignore_index=ignore)
        ko = KernelOnly(srcs, gd, C, ignore)
        paths = {"reference_tail": lambda: reference_tail(srcs, gts, gd, C, ignore),
                 "parent_best": lambda: parent_tail(srcs, gd, C, ignore, crit),
                 "eval_tail_with_host_copies": lambda: new_tail(srcs, gd, C, ignore)}
        for _ in range(2):                  # warm-up: allocator, pinned buffers, LDS limits
            for fn in paths.values():
                fn()
        ko.run(2)
        times = {k: [] for k in paths}
        kern = []
        for _ in range(a.rounds):           # alternating
            for k, fn in paths.items():
                times[k].append(timed(fn))
            kern.append(ko.run())
        Pn = H * W
        rd, wr = 2 * Pn * C * 4 + 8 * Pn, 6 * Pn
        rec = {k: summary(v) for k, v in times.items()}
        rec["kernel_alone"] = summary(kern)
        kt = statistics.median(kern)
        rec["kernel_bytes_read"], rec["kernel_bytes_written"] = rd, wr
        rec["kernel_bytes_per_s"] = (rd + wr) / kt
        rec["kernel_share_of_roof"] = (rd + wr) / kt / ROOF
        new = rec["eval_tail_with_host_copies"]
        for other in ("reference_tail", "parent_best"):
            o = rec[other]
            margin = 3.0 * max(o["spread_ms"], new["spread_ms"])
            rec["faster_than_%s_by_3_spreads" % other] = bool(o["median_ms"] - new["median_ms"] > margin)
            rec["speedup_over_%s" % other] = o["median_ms"] / new["median_ms"]
        result["shapes"][name] = rec
        print(name, json.dumps(rec, indent=1))
        del srcs, ko, paths
        torch.cuda.empty_cache()
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"evaltail_bench": {k: {"new_ms": v["eval_tail_with_host_copies"]["median_ms"],
                                             "parent_ms": v["parent_best"]["median_ms"],
                                             "reference_ms": v["reference_tail"]["median_ms"],
                                             "kernel_ms": v["kernel_alone"]["median_ms"],
                                             "kernel_share_of_roof": v["kernel_share_of_roof"]}
                                         for k, v in result["shapes"].items()}}))


if __name__ == "__main__":
    main()
