#!/usr/bin/env python
"""Depthwise 3x3 conv (csrc/dwconv.hip) against torch's grouped conv and against a copy, over the depthwise shapes of
DeepV3PlusX71 at an 800 x 800 crop, batch 1, in ONE call:
    python tools/dwbench.py [reps] [--rounds N] [--json profiles/dwconv_bench.json]
Per shape and direction three things are timed ALTERNATELY, round by round, with device events around a replayed graph of
`reps` launches (reps x rounds >= 50 launches per figure; medians):
  ours      ssa_dwconv3x3 with the BatchNorm sums (the training form) / ssa_dwconv3x3_bwd (dx and dW in one pass, plus
            its small partial-sum launch) -- measured TWICE in the same alternation (ours, ours_again): the distance of
            the two medians is the spread the comparison allows;
  torch     the reference's own op: F.conv2d(groups = C) on 16-bit channels_last tensors / aten.convolution_backward for
            input and weight (a form this torch build does not offer, or cannot capture, is reported, not hidden: it is
            then timed eagerly, or left out with the error);
  copy      Tensor.copy_ of the bytes the algorithm must move, from the shapes: forward reads x and writes y, backward
            reads dy and x and writes dx (weights, sums and the dW partials are not counted).
`not_slower` = ours <= torch x (1 + spread), spread = the largest of |ours - ours_again| / the smaller median and the
(max - min) / median over the rounds of each of the two measurements of ours.  The fraction of the copy rate is
reported, not gated.  Needs a GPU."""
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

# (H, W, C, stride, dil) at B = 1: the (C, stride, dil) set of the trunk at the resolution each occurs at
SHAPES = [(400, 400, 64, 1, 1), (400, 400, 128, 1, 1), (400, 400, 128, 2, 1), (200, 200, 256, 1, 1), (200, 200, 728, 1, 1),
          (200, 200, 728, 2, 1), (100, 100, 728, 1, 2), (100, 100, 1024, 1, 4), (100, 100, 1536, 1, 4)]


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


def eager(fn, reps):
    def run():
        for _ in range(reps):
            fn()
    return run


def timed_us(run, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


class Problem:
    def __init__(self, H, W, C, s, d, seed):
        g = torch.Generator().manual_seed(seed)
        L = hb.lib()
        self.L, self.C, self.s, self.d = L, C, s, d
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        self.P_in, self.P_out = H * W, Ho * Wo
        self.x = torch.randn((1, H, W, C), generator=g).to(hb.ACT_DTYPE).cuda()
        self.dy = torch.randn((1, Ho, Wo, C), generator=g).to(hb.ACT_DTYPE).cuda()
        self.w = (torch.randn((C, 1, 3, 3), generator=g) * 0.3).cuda()
        self.y, self.dx = torch.empty_like(self.dy), torch.empty_like(self.x)
        self.dw = torch.zeros_like(self.w)
        self.stats = torch.zeros(hb.stat_replicas() * 2 * C, dtype=torch.float64, device="cuda")
        self.desc = _lib.DwConvDesc(1, H, W, C, C, Ho, Wo, C, s, d)
        n = ctypes.c_size_t(0)
        hb.check(L.ssa_dwconv3x3_bwd_plan(ctypes.byref(self.desc), ctypes.byref(n)), "ssa_dwconv3x3_bwd_plan")
        self.ws = torch.empty(n.value // 4, dtype=torch.float32, device="cuda")
        # the reference's op on its own layout: NCHW shape, channels_last strides, 16-bit
        self.xt = self.x.permute(0, 3, 1, 2)
        self.dyt = self.dy.permute(0, 3, 1, 2)
        self.wt = self.w.to(hb.ACT_DTYPE)
        self.cf = [torch.empty((self.P_in + self.P_out) // 2 * C, dtype=hb.ACT_DTYPE, device="cuda") for _ in range(2)]
        self.cb = [torch.empty((self.P_out + 2 * self.P_in) // 2 * C, dtype=hb.ACT_DTYPE, device="cuda") for _ in range(2)]

    def ours_fwd(self):
        hb.check(self.L.ssa_dwconv3x3(ctypes.byref(self.desc), hb._p(self.x), hb._p(self.w), hb._p(self.y), hb._p(self.stats), None,
                                      0, hb._s()), "ssa_dwconv3x3")

    def ours_bwd(self):
        hb.check(self.L.ssa_dwconv3x3_bwd(ctypes.byref(self.desc), hb._p(self.x), hb._p(self.dy), self.C, hb._p(self.w),
                                          hb._p(self.dx), self.C, hb._p(self.dw), 0, hb._p(self.ws), hb._s()), "ssa_dwconv3x3_bwd")

    def torch_fwd(self):
        self.yt = torch.nn.functional.conv2d(self.xt, self.wt, None, self.s, self.d, self.d, self.C)

    def torch_bwd(self):
        self.gt = torch.ops.aten.convolution_backward(self.dyt, self.xt, self.wt, None, [self.s] * 2, [self.d] * 2, [self.d] * 2,
                                                      False, [0, 0], self.C, [True, True, False])

    def copy_fwd(self):
        self.cf[1].copy_(self.cf[0])

    def copy_bwd(self):
        self.cb[1].copy_(self.cb[0])

    def agreement(self):
        """Largest difference of ours from torch's op relative to the largest value (the two round differently)."""
        self.ours_fwd(), self.ours_bwd(), self.torch_fwd(), self.torch_bwd()
        torch.cuda.synchronize()
        rel = lambda a, b: float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-30))  # noqa: E731
        return {"y": round(rel(self.y, self.yt.permute(0, 2, 3, 1)), 5), "dx": round(rel(self.dx, self.gt[0].permute(0, 2, 3, 1)), 5),
                "dw": round(rel(self.dw, self.gt[1]), 5)}


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    rounds = int(_opt("--rounds", "7"))
    assert reps * rounds >= 50, "at least 50 launches per figure"
    out = _opt("--json")
    results = []
    for i, (H, W, C, s, d) in enumerate(SHAPES):
        pr = Problem(H, W, C, s, d, 80 + i)
        try:
            agree, torch_err = pr.agreement(), None
        except Exception as e:                  # noqa: BLE001 -- a form this torch build does not offer on this device
            agree, torch_err = None, "%s: %s" % (type(e).__name__, str(e)[:200])
        for direction, ours, ref, cp, nbytes in (("forward", pr.ours_fwd, pr.torch_fwd, pr.copy_fwd, 2.0 * C * (pr.P_in + pr.P_out)),
                                                 ("backward", pr.ours_bwd, pr.torch_bwd, pr.copy_bwd, 2.0 * C * (pr.P_out + 2 * pr.P_in))):
            runs = {"ours": capture(ours, reps), "ours_again": capture(ours, reps), "copy": capture(cp, reps)}
            torch_mode = None
            if torch_err is None:
                try:
                    runs["torch"], torch_mode = capture(ref, reps), "graph"
                except Exception as e:          # noqa: BLE001 -- the library behind it does not capture: timed eagerly
                    torch.cuda.synchronize()
                    torch_mode = "eager (%s)" % type(e).__name__
                    runs["torch"] = eager(ref, reps)
            t = {k: [] for k in runs}
            for _ in range(rounds):
                for k, run in runs.items():
                    t[k].append(timed_us(run, reps))
            med = {k: statistics.median(v) for k, v in t.items()}
            spr = {k: (max(v) - min(v)) / med[k] for k, v in t.items()}
            spread = max(abs(med["ours"] - med["ours_again"]) / min(med["ours"], med["ours_again"]), spr["ours"], spr["ours_again"])
            rec = {"shape": [1, H, W, C], "stride": s, "dil": d, "direction": direction, "dtype": str(hb.ACT_DTYPE).replace("torch.", ""),
                   "reps": reps, "rounds": rounds, "lib_sha": _lib.built_sha(), "bytes": nbytes,
                   "us": {k: {"median": round(med[k], 2), "min": round(min(t[k]), 2), "max": round(max(t[k]), 2),
                              "spread": round(spr[k], 4)} for k in t},
                   "spread_allowed": round(spread, 4), "ours_TBps": round(nbytes / med["ours"] / 1e6, 3),
                   "copy_TBps": round(nbytes / med["copy"] / 1e6, 3), "fraction_of_copy_rate": round(med["copy"] / med["ours"], 3),
                   "torch_mode": torch_mode, "torch_error": torch_err, "agreement_with_torch": agree}
            if "torch" in med:
                rec["ours_over_torch"] = round(med["ours"] / med["torch"], 4)
                rec["not_slower"] = bool(med["ours"] <= med["torch"] * (1 + spread))
            results.append(rec)
            print("%-16s s%d d%d %-8s ours %8.1f / %8.1f us  torch %8s us  copy %8.1f us  of copy rate %.2f  %s" % (
                "x".join(map(str, (H, W, C))), s, d, direction, med["ours"], med["ours_again"],
                ("%.1f" % med["torch"]) if "torch" in med else "n/a", med["copy"], med["copy"] / med["ours"],
                "n/a" if "torch" not in med else ("ok" if rec["not_slower"] else "LOST")))
        del pr
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
