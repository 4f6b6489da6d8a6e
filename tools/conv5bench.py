#!/usr/bin/env python
"""The 5x5 convs of the Deeper decoders (csrc/conv_halo5.hip) against the implicit GEMM (csrc/conv_igemm.hip: the route
these layers had before the kernel existed, so the yardstick), forward and data gradient, at the sizes of an 800 x 800
crop, batch 1, in ONE call:
    python tools/conv5bench.py [reps] [--rounds N] [--json profiles/conv5x5_bench.json]
      conv_up2  200 x 200 x 320 -> 256      its data gradient 200 x 200 x 256 -> 320
      conv_up3  400 x 400 x 288 -> 256      its data gradient 400 x 400 x 256 -> 288
Per point three things are timed ALTERNATELY, round by round, with device events around a replayed graph of `reps`
launches (reps x rounds >= 50 launches per figure; medians): halo5, halo5 a second time (the distance of the two medians
and the (max - min) / median over the rounds are the spread), igemm.  Both write the BatchNorm partial sums in the
forward direction (the training form).  `faster` = halo5 x (1 + spread) < igemm.  Also reported: TFLOP/s, the fraction
of the 2.5 PFLOP/s dense MFMA peak, and the largest difference between the two routes' outputs in units of the storage
format's spacing.  Needs a GPU."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from semseg_amd import _lib, hip_backend as hb  # noqa: E402

PEAK_MFMA = 2.5e15
# layer, direction, H, W, Cin, Cout of the launch (a data gradient reads dy: Cin = the layer's output channels)
POINTS = [("conv_up2", "forward", 200, 200, 320, 256), ("conv_up2", "dgrad", 200, 200, 256, 320),
          ("conv_up3", "forward", 400, 400, 288, 256), ("conv_up3", "dgrad", 400, 400, 256, 288)]


def _opt(name, dflt=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else dflt


def capture(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    return g.replay


def timed_us(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


class Problem:
    def __init__(self, direction, H, W, Cin, Cout, seed):
        g = torch.Generator().manual_seed(seed)
        self.L = hb.lib()
        self.fwd = direction == "forward"
        self.x = torch.randn((1, H, W, Cin), generator=g).to(hb.ACT_DTYPE).cuda()
        # the layer's own OIHW weight: [256][320 or 288][5][5] in both directions
        co, ci = (Cout, Cin) if self.fwd else (Cin, Cout)
        self.w = (torch.randn((co, ci, 5, 5), generator=g) * (2.0 / (25 * ci)) ** 0.5).cuda()
        self.y5 = torch.empty((1, H, W, Cout), dtype=hb.ACT_DTYPE, device="cuda")
        self.yg = torch.empty_like(self.y5)
        self.stats = torch.zeros(hb.stat_replicas() * 2 * Cout, dtype=torch.float64, device="cuda") if self.fwd else None
        self.d5 = _lib.ConvDesc(1, H, W, Cin, Cin, H, W, Cout, Cout, 5, 5, 1, 2, 1, 0, 0, 0, -1)
        assert self.L.ssa_conv2d_halo5_supported(ctypes.byref(self.d5)) == 1
        if self.fwd:
            self.w5, _ = hb._packed_filter(self.w, 2, Cin, 0)
            self.wg, kpad = hb._packed_filter(self.w, 0, Cin, 0)
        else:
            self.w5, _ = hb._packed_filter(self.w, 3, 0, Cin)
            self.wg, kpad = hb._packed_filter(self.w, 1, 0, Cin)
        self.dg = _lib.ConvDesc(1, H, W, Cin, Cin, H, W, Cout, Cout, 5, 5, 1, 2, 1, 0, kpad, 0, -1)
        self.flops = 2.0 * H * W * Cout * Cin * 25

    def halo5(self):
        hb.check(self.L.ssa_conv2d_halo5(ctypes.byref(self.d5), hb._p(self.x), hb._p(self.w5), None, hb._p(self.y5),
                                         hb._p(self.stats), hb._s()), "ssa_conv2d_halo5")

    def igemm(self):
        hb.check(self.L.ssa_conv2d_igemm_stats(ctypes.byref(self.dg), hb._p(self.x), hb._p(self.wg), None, hb._p(self.yg),
                                               hb._p(self.stats), hb._s()), "ssa_conv2d_igemm_stats")

    def agreement(self):
        """Largest |halo5 - igemm| in units of the storage format's spacing at the larger of the two results."""
        self.halo5(), self.igemm()
        torch.cuda.synchronize()
        a, b = self.y5.double(), self.yg.double()
        bits, emin = (7, -126) if hb.ACT_DTYPE == torch.bfloat16 else (10, -14)
        sp = 2.0 ** (torch.floor(torch.log2(torch.maximum(a.abs(), b.abs()).clamp(min=2.0 ** emin))) - bits)
        return round(float(((a - b).abs() / sp).max()), 3)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    rounds = int(_opt("--rounds", "7"))
    assert reps * rounds >= 50, "at least 50 launches per figure"
    out = _opt("--json")
    results = []
    for i, (layer, direction, H, W, Cin, Cout) in enumerate(POINTS):
        pr = Problem(direction, H, W, Cin, Cout, 50 + i)
        agree = pr.agreement()
        runs = {"halo5": capture(pr.halo5, reps), "halo5_again": capture(pr.halo5, reps), "igemm": capture(pr.igemm, reps)}
        t = {k: [] for k in runs}
        for _ in range(rounds):
            for k, run in runs.items():
                t[k].append(timed_us(run, reps))
        med = {k: statistics.median(v) for k, v in t.items()}
        spr = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
        spread = max(abs(med["halo5"] - med["halo5_again"]) / min(med["halo5"], med["halo5_again"]), spr["halo5"], spr["halo5_again"])
        rec = {"layer": layer, "direction": direction, "shape": [1, H, W, Cin], "cout": Cout,
               "dtype": str(hb.ACT_DTYPE).replace("torch.", ""), "reps": reps, "rounds": rounds, "lib_sha": _lib.built_sha(),
               "flops": pr.flops,
               "us": {k: {"median": round(med[k], 2), "min": round(min(t[k]), 2), "max": round(max(t[k]), 2),
                          "spread": round(spr[k], 4)} for k in t},
               "spread_allowed": round(spread, 4),
               "halo5_TFLOPs": round(pr.flops / med["halo5"] / 1e6, 1), "igemm_TFLOPs": round(pr.flops / med["igemm"] / 1e6, 1),
               "halo5_mfma_frac": round(pr.flops / (med["halo5"] * 1e-6) / PEAK_MFMA, 4),
               "igemm_mfma_frac": round(pr.flops / (med["igemm"] * 1e-6) / PEAK_MFMA, 4),
               "igemm_over_halo5": round(med["igemm"] / med["halo5"], 3),
               "faster": bool(med["halo5"] * (1 + spread) < med["igemm"]),
               "max_difference_in_storage_spacings": agree}
        results.append(rec)
        print("%-8s %-7s %dx%dx%d->%d  halo5 %8.1f / %8.1f us (%.3f of MFMA peak)  igemm %8.1f us (%.3f)  igemm/halo5 %.2f  %s" % (
            layer, direction, H, W, Cin, Cout, med["halo5"], med["halo5_again"], rec["halo5_mfma_frac"], med["igemm"],
            rec["igemm_mfma_frac"], rec["igemm_over_halo5"], "faster" if rec["faster"] else "NOT FASTER"), flush=True)
        del pr
        hb.clear_pack_cache()
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0 if all(r["faster"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
