#!/usr/bin/env python
"""Micro-benchmark of the implicit-GEMM conv kernel (csrc/conv_igemm.hip) on the device, through hb._igemm (no autograd):
the problems of the stage-4 fuse layer's first level at both scale passes (1.0x and 0.5x of a 1024 x 1024 crop) -- the
stride-2 3x3 convs, the 1x1 fuse convs -- and layer1's 64 -> 256 1x1, each alone and all of them as ONE grouped launch per
tile configuration, the way the step issues them.
python tools/igemmbench.py [reps] [--lib <variant>]        (tools/expbuild.sh / a copied library: lib/libsemseg_hip[_f16]_<variant>.so)
Per problem: tile configuration, time, TFLOP/s, and a CRC of the output bytes (equal CRCs = bit-identical outputs between
two builds) with the largest deviation from torch's fp32 conv of the same 16-bit operands as the checker."""
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from semseg_amd import _lib  # noqa: E402

if "--lib" in sys.argv:
    i = sys.argv.index("--lib")
    _lib.LIB_PATH = _lib.LIB_PATH[:-len(".so")] + "_%s.so" % sys.argv[i + 1]
    del sys.argv[i:i + 2]
from semseg_amd import hip_backend as hb  # noqa: E402
from semseg_amd._lib import ConvDesc  # noqa: E402

DEV = "cuda"
ACT = hb.ACT_DTYPE


def timeit(fn, reps):
    """us per call: `reps` calls captured in one graph, the second replay timed (as tools/tilebench.py)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


class Prob:
    def __init__(self, name, Cin, Cout, k, stride, H, W, seed):
        g = torch.Generator().manual_seed(seed)
        self.name, self.Cin, self.Cout, self.k, self.stride, self.H, self.W = name, Cin, Cout, k, stride, H, W
        self.pad = k // 2
        self.Ho, self.Wo = (H + 2 * self.pad - k) // stride + 1, (W + 2 * self.pad - k) // stride + 1
        self.x = torch.randn(1, H, W, Cin, generator=g).to(DEV).to(ACT)
        self.w = (torch.randn(Cout, Cin, k, k, generator=g) / (k * Cin ** 0.5)).to(DEV)
        self.wp, self.Kpad = hb._packed_filter(self.w, 0, Cin, 0)
        self.y = torch.empty(1, self.Ho, self.Wo, Cout, device=DEV, dtype=ACT)
        self.stats = torch.zeros(hb.stat_replicas() * 2 * Cout, device=DEV, dtype=torch.float64)
        self.flops = 2.0 * self.Ho * self.Wo * Cout * Cin * k * k
        d = ConvDesc(1, H, W, Cin, Cin, self.Ho, self.Wo, Cout, Cout, k, k, stride, self.pad, 1, 0, self.Kpad, 0, -1)
        self.cfg = hb.lib().ssa_conv2d_igemm_tile(d)

    def run(self):
        hb._igemm(self.x, self.Cin, (1, self.H, self.W, self.Cin), self.wp, self.Kpad, None, (self.Ho, self.Wo), self.Cout,
                  (self.k, self.k), self.stride, self.pad, 1, False, False, stats=self.stats, out=self.y)

    def check(self):
        self.run()
        torch.cuda.synchronize()
        ref = torch.nn.functional.conv2d(self.x.float().permute(0, 3, 1, 2), self.w.to(ACT).float(), None, self.stride, self.pad)
        err = float((self.y.float().permute(0, 3, 1, 2) - ref).abs().max() / ref.abs().max())
        return zlib.crc32(self.y.cpu().view(torch.int16).numpy().tobytes()), err


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    probs = []
    for scale, tag in ((1, "1.0x"), (2, "0.5x")):
        s = lambda v: v // scale  # noqa: E731
        level = [("s2 48->48", 48, 48, 3, 2, 256), ("s2 48->96", 48, 96, 3, 2, 256), ("s2 96->96", 96, 96, 3, 2, 128),
                 ("s2 96->192", 96, 192, 3, 2, 128), ("s2 192->384", 192, 384, 3, 2, 64), ("1x1 384->48", 384, 48, 1, 1, 32),
                 ("1x1 192->48", 192, 48, 1, 1, 64), ("1x1 96->48", 96, 48, 1, 1, 128), ("1x1 64->256 layer1", 64, 256, 1, 1, 256)]
        for i, (n, ci, co, k, st, hw) in enumerate(level):
            probs.append(Prob("%s %s @%d" % (tag, n, s(hw)), ci, co, k, st, s(hw), s(hw), 10 * scale + i))
    print("library %s, storage %s, %d reps per graph replay" % (os.path.basename(_lib.LIB_PATH), _lib.ACT, reps))
    print("%-32s %4s %9s %9s %11s %9s" % ("problem", "cfg", "us", "TFLOP/s", "crc32", "max err"))
    for p in probs:
        crc, err = p.check()
        t = timeit(p.run, reps)
        print("%-32s %4d %9.1f %9.1f  %08x %9.1e" % (p.name, p.cfg, t, p.flops / t / 1e6, crc, err))

    def level_run():
        with hb.group():
            for p in probs:
                p.run()
    fl = sum(p.flops for p in probs)
    t = timeit(level_run, reps)
    print("all %d problems in one bracket (%.1f GFLOP): %.1f us = %.1f TFLOP/s" % (len(probs), fl / 1e9, t, fl / t / 1e6))
    s2 = [p for p in probs if p.stride == 2]

    def s2_run():
        with hb.group():
            for p in s2:
                p.run()
    fl = sum(p.flops for p in s2)
    t = timeit(s2_run, reps)
    print("the %d stride-2 problems in one bracket (%.1f GFLOP): %.1f us = %.1f TFLOP/s" % (len(s2), fl / 1e9, t, fl / t / 1e6))


if __name__ == "__main__":
    main()
