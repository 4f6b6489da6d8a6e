#!/usr/bin/env python
"""The convs of the Dense Prediction Cell (csrc/conv_dil.hip) at the 100 x 100 map of an 800 x 800 crop, batch 1, in ONE
call:
    python tools/dpcbench.py [reps] [--rounds N] [--json profiles/dpc_bench.json]
      a   2048 -> 256 and 4096 -> 256, dilation (2, 12)
      b   256 -> 256 (36, 30)     c   256 -> 256 (12, 42)     d   256 -> 256 (2, 2)     e   256 -> 256 (12, 6)
Passes: forward with the BatchNorm partial sums, data gradient, weight gradient (partials + ordered reduce); b, c, d also
as ONE grouped launch (forward, data gradient).  Baselines, per shape:
  (a) ssa_conv2d_igemm_stats / ssa_conv2d_igemm (+ ssa_conv2d_wgrad / _reduce) on the same shape with SQUARE dilation
      dil_h and again with dil_w -- the only route a dilated 3x3 of these widths had before; the same FLOPs, and the two
      bracket what the taps outside the image save;
  (b) torch's F.conv2d with the tuple dilation on the device (forward; autograd for the two gradients together);
  (c) a device copy of the bytes the conv must move (x + y + the 16-bit filter once).
Every figure: device events around a replayed graph of `reps` launches, `rounds` rounds taken ALTERNATELY over the
candidates of a shape (reps x rounds >= 50 launches per figure), medians with (max - min) / median as the spread; the
new kernel is timed twice and the distance of its two medians counts into the spread.  `slower_than_a` = the new kernel
beyond the spread slower than the FASTER of the two square runs.  One process.  Needs a GPU."""
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
H = W = 100
# layer, Cin, Cout, (dil_h, dil_w)
POINTS = [("a2048", 2048, 256, (2, 12)), ("a4096", 4096, 256, (2, 12)), ("b", 256, 256, (36, 30)), ("c", 256, 256, (12, 42)),
          ("d", 256, 256, (2, 2)), ("e", 256, 256, (12, 6))]


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


def valid_fraction(dil):
    """Fraction of (tap, pixel) pairs inside the image: what a kernel that skips nothing computes in vain."""
    rows = [max(0, H - dil[0]), H, max(0, H - dil[0])]
    cols = [max(0, W - dil[1]), W, max(0, W - dil[1])]
    return sum(r * c for r in rows for c in cols) / (9.0 * H * W)


class Problem:
    def __init__(self, Cin, Cout, dil, seed):
        g = torch.Generator().manual_seed(seed)
        self.L = hb.lib()
        self.Cin, self.Cout, self.dil = Cin, Cout, dil
        self.x = torch.randn((1, H, W, Cin), generator=g).to(hb.ACT_DTYPE).cuda()
        self.dy = torch.randn((1, H, W, Cout), generator=g).to(hb.ACT_DTYPE).cuda()
        self.w = (torch.randn((Cout, Cin, 3, 3), generator=g) * (2.0 / (9 * Cin)) ** 0.5).cuda()
        self.y = torch.empty((1, H, W, Cout), dtype=hb.ACT_DTYPE, device="cuda")
        self.dx = torch.empty((1, H, W, Cin), dtype=hb.ACT_DTYPE, device="cuda")
        self.dw = torch.empty((Cout, Cin, 3, 3), dtype=torch.float32, device="cuda")
        self.stats = torch.zeros(hb.stat_replicas() * 2 * Cout, dtype=torch.float64, device="cuda")
        self.flops = 2.0 * H * W * Cout * Cin * 9
        self.bytes = 2.0 * (H * W * (Cin + Cout) + 9 * Cin * Cout)
        # the new family
        self.df = _lib.DilConvDesc(1, H, W, Cin, Cin, Cout, Cout, dil[0], dil[1])
        self.dd = _lib.DilConvDesc(1, H, W, Cout, Cout, Cin, Cin, dil[0], dil[1])
        self.wf, _ = hb._packed_filter(self.w, 2, Cin, 0)
        self.wd, _ = hb._packed_filter(self.w, 3, 0, Cout)
        ns, nb = ctypes.c_int(0), ctypes.c_size_t(0)
        hb.check(self.L.ssa_dilconv3x3_wgrad_plan(ctypes.byref(self.df), ctypes.byref(ns), ctypes.byref(nb)), "plan")
        self.nsplit = ns.value
        self.ws = torch.empty((nb.value // 4,), dtype=torch.float32, device="cuda")
        # baseline (a): the implicit GEMM with a square dilation, forward operand mode 0, data gradient mode 1
        self.g0, self.kpad0 = hb._packed_filter(self.w, 0, Cin, 0)
        self.g1, self.kpad1 = hb._packed_filter(self.w, 1, 0, Cout)
        self.sq = {}
        for d in sorted(set(dil)):
            fw = _lib.ConvDesc(1, H, W, Cin, Cin, H, W, Cout, Cout, 3, 3, 1, d, d, 0, self.kpad0, 0, -1)
            bw = _lib.ConvDesc(1, H, W, Cout, Cout, H, W, Cin, Cin, 3, 3, 1, d, d, 0, self.kpad1, 0, -1)
            ns, nb = ctypes.c_int(0), ctypes.c_size_t(0)
            hb.check(self.L.ssa_conv2d_wgrad_plan(ctypes.byref(fw), Cout, ctypes.byref(ns), ctypes.byref(nb)), "wgrad_plan")
            self.sq[d] = (fw, bw, ns.value, torch.empty((nb.value // 4,), dtype=torch.float32, device="cuda"))
        # baseline (b)
        self.xt = self.x.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        self.wt = self.w.to(hb.ACT_DTYPE).contiguous(memory_format=torch.channels_last)
        self.dyt = self.dy.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)
        # baseline (c)
        self.src = torch.empty((int(self.bytes) // 2,), dtype=hb.ACT_DTYPE, device="cuda")
        self.dst = torch.empty_like(self.src)

    # -- the new kernels
    def fwd(self):
        hb.check(self.L.ssa_dilconv3x3(ctypes.byref(self.df), hb._p(self.x), hb._p(self.wf), hb._p(self.y), hb._p(self.stats),
                                       hb._s()), "ssa_dilconv3x3")

    def dgrad(self):
        hb.check(self.L.ssa_dilconv3x3(ctypes.byref(self.dd), hb._p(self.dy), hb._p(self.wd), hb._p(self.dx), None, hb._s()),
                 "ssa_dilconv3x3")

    def wgrad(self):
        hb.check(self.L.ssa_dilconv3x3_wgrad(ctypes.byref(self.df), hb._p(self.x), hb._p(self.dy), self.Cout, hb._p(self.dw), 0,
                                             hb._p(self.ws), hb._s()), "ssa_dilconv3x3_wgrad")

    # -- baseline (a)
    def sq_fwd(self, d):
        fw = self.sq[d][0]
        return lambda: hb.check(self.L.ssa_conv2d_igemm_stats(ctypes.byref(fw), hb._p(self.x), hb._p(self.g0), None, hb._p(self.y),
                                                              hb._p(self.stats), hb._s()), "ssa_conv2d_igemm_stats")

    def sq_dgrad(self, d):
        bw = self.sq[d][1]
        return lambda: hb.check(self.L.ssa_conv2d_igemm(ctypes.byref(bw), hb._p(self.dy), hb._p(self.g1), None, hb._p(self.dx),
                                                        hb._s()), "ssa_conv2d_igemm")

    def sq_wgrad(self, d):
        fw, _, ns, part = self.sq[d]

        def run():
            hb.check(self.L.ssa_conv2d_wgrad(ctypes.byref(fw), hb._p(self.x), hb._p(self.dy), self.Cout, self.Cout, ns, hb._p(part),
                                             hb._s()), "ssa_conv2d_wgrad")
            hb.check(self.L.ssa_conv2d_wgrad_reduce(hb._p(part), ns, self.Cout, self.Cout, self.Cin, self.Cin, 3, 3, hb._p(self.dw),
                                                    0, hb._s()), "ssa_conv2d_wgrad_reduce")
        return run

    # -- baseline (b), (c)
    def torch_fwd(self):
        return torch.nn.functional.conv2d(self.xt, self.wt, None, 1, self.dil, self.dil)

    def torch_bwd(self):
        return torch.ops.aten.convolution_backward(self.dyt, self.xt, self.wt, None, (1, 1), self.dil, self.dil, False, (0, 0), 1,
                                                   (True, True, False))

    def copy(self):
        self.dst.copy_(self.src)

    def agreement(self):
        """Largest |new - torch| of the forward in units of the storage format's spacing at the larger of the two."""
        self.fwd()
        torch.cuda.synchronize()
        a, b = self.y.double(), self.torch_fwd().permute(0, 2, 3, 1).double()
        bits, emin = (7, -126) if hb.ACT_DTYPE == torch.bfloat16 else (10, -14)
        sp = 2.0 ** (torch.floor(torch.log2(torch.maximum(a.abs(), b.abs()).clamp(min=2.0 ** emin))) - bits)
        return round(float(((a - b).abs() / sp).max()), 3)


def measure(runs, reps, rounds):
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, run in runs.items():
            t[k].append(timed_us(run, reps))
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2),
                "spread": round((max(v) - min(v)) / statistics.median(v), 4)} for k, v in t.items()}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    rounds = int(_opt("--rounds", "5"))
    assert reps * rounds >= 50, "at least 50 launches per figure"
    out = _opt("--json")
    results = []
    probs = {}
    for i, (layer, Cin, Cout, dil) in enumerate(POINTS):
        pr = Problem(Cin, Cout, dil, 70 + i)
        rec = {"layer": layer, "shape": [1, H, W, Cin], "cout": Cout, "dil": list(dil), "nsplit": pr.nsplit,
               "dtype": str(hb.ACT_DTYPE).replace("torch.", ""), "reps": reps, "rounds": rounds, "lib_sha": _lib.built_sha(),
               "flops": pr.flops, "min_bytes": pr.bytes, "valid_tap_fraction": round(valid_fraction(dil), 4),
               "max_difference_from_torch_in_storage_spacings": pr.agreement(), "passes": {}}
        for pas, new, sq, tch in (("forward", pr.fwd, pr.sq_fwd, pr.torch_fwd), ("dgrad", pr.dgrad, pr.sq_dgrad, None),
                                  ("wgrad", pr.wgrad, pr.sq_wgrad, None)):
            runs = {"new": capture(new, reps), "new_again": capture(new, reps)}
            for d in sorted(set(dil)):
                runs["square_%d" % d] = capture(sq(d), reps)
            if tch is not None:
                runs["torch"] = capture(tch, reps)
                runs["copy"] = capture(pr.copy, reps)
            us = measure(runs, reps, rounds)
            a = min(us[k]["median"] for k in us if k.startswith("square_"))
            spread = max(abs(us["new"]["median"] - us["new_again"]["median"]) / min(us["new"]["median"], us["new_again"]["median"]),
                         us["new"]["spread"], us["new_again"]["spread"])
            p = {"us": us, "spread_allowed": round(spread, 4), "new_TFLOPs": round(pr.flops / us["new"]["median"] / 1e6, 1),
                 "new_mfma_frac": round(pr.flops / (us["new"]["median"] * 1e-6) / PEAK_MFMA, 4),
                 "square_over_new": {k: round(us[k]["median"] / us["new"]["median"], 3) for k in us if k.startswith("square_")},
                 "slower_than_a": bool(us["new"]["median"] > a * (1 + spread))}
            if tch is not None:
                p["torch_over_new"] = round(us["torch"]["median"] / us["new"]["median"], 3)
                p["new_over_copy"] = round(us["new"]["median"] / us["copy"]["median"], 3)
            rec["passes"][pas] = p
            print("%-6s %-7s %5d->%d %-9s new %8.1f / %8.1f us (%.3f of MFMA peak)  square %s%s  %s" % (
                layer, pas, Cin, Cout, tuple(dil), us["new"]["median"], us["new_again"]["median"], p["new_mfma_frac"],
                " ".join("%s %.1f" % (k[7:], us[k]["median"]) for k in us if k.startswith("square_")),
                "  torch %.1f copy %.1f" % (us["torch"]["median"], us["copy"]["median"]) if tch is not None else "",
                "SLOWER than (a)" if p["slower_than_a"] else ""), flush=True)
        # torch's two gradients together (one autograd call) against the new kernel's two
        us = measure({"torch_bwd": capture(pr.torch_bwd, reps)}, reps, rounds)
        rec["passes"]["torch_dgrad_plus_wgrad_us"] = us["torch_bwd"]
        results.append(rec)
        if layer in ("b", "c", "d"):
            probs[layer] = pr
        else:
            del pr
    # b, c, d as ONE grouped launch against the three alone
    def grouped(which):
        def run():
            with hb.group():
                for k in ("b", "c", "d"):
                    getattr(probs[k], which)()
        return run

    def alone(which):
        def run():
            for k in ("b", "c", "d"):
                getattr(probs[k], which)()
        return run
    grp = {}
    for which in ("fwd", "dgrad"):
        us = measure({"grouped": capture(grouped(which), reps), "alone": capture(alone(which), reps),
                      "grouped_again": capture(grouped(which), reps)}, reps, rounds)
        grp[which] = {"us": us, "alone_over_grouped": round(us["alone"]["median"] / us["grouped"]["median"], 3)}
        print("b+c+d %-6s grouped %8.1f / %8.1f us  alone %8.1f us" % (which, us["grouped"]["median"], us["grouped_again"]["median"],
                                                                     us["alone"]["median"]), flush=True)
    results.append({"layer": "b+c+d grouped", "passes": grp})
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
