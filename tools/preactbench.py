#!/usr/bin/env python
"""Micro-benchmark of the pre-activation passes on the device, through the C ABI (no autograd): a chain of eight identity
pre-activation steps (network/wider_resnet.py:172-185) with an elementwise stand-in for the block's convs, forward and
backward, FUSED (ssa_add_bn_stats, ssa_bn_bwd_apply_add) against the UNFUSED composition of the older entry points.
    python tools/preactbench.py [reps] [--rounds N] [--json profiles/wrn38_preact_bench.json]

  step k forward    unfused: ssa_sum_act(u, v) -> s; ssa_bn_stats(s); ssa_bn_apply_train(s) -> z        (6 B/element x 2 bytes)
                    fused:   ssa_add_bn_stats(u, v) -> s, sums; ssa_bn_apply_train(s) -> z                 (5)
                    both:    u' = stand-in(z) (ssa_sum_act of one operand: read 1, write 1), v' = s
  step k backward   both:    dz = stand-in(G') (read 1, write 1); ssa_bn_bwd_reduce(s, dz)
                    unfused: ssa_bn_bwd_apply -> dx; ssa_sum_act(dx, G') -> G                                (8, reduce included)
                    fused:   ssa_bn_bwd_apply_add(dadd = G') -> G                                             (6)
  (G' = the gradient of the next step's input, which reaches this step's input over the conv path AND over the shortcut.)

Method: each variant's chain is captured into a hipGraph `reps` times over and replayed; the two variants alternate within
one process for `rounds` rounds (after a warm-up replay of each), timed with device events around a replay.  Reported per
shape and direction: median, min and max of the rounds in microseconds per chain, the spread (max - min) / median of each
variant, and `not_slower` = fused median <= unfused median x (1 + the larger of the two spreads).  Needs a GPU."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from semseg_amd import _lib  # noqa: E402
from semseg_amd import hip_backend as hb  # noqa: E402

SHAPES = [(1, 200, 200, 256), (1, 100, 100, 512), (1, 100, 100, 2048)]
STEPS = 8
P_ = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731


def _opt(name, dflt=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else dflt


class Chain:
    def __init__(self, shape, seed):
        assert torch.cuda.is_available(), "preactbench needs a GPU"
        self.L = hb.lib()
        B, H, W, C = shape
        self.P, self.C, self.hw = B * H * W, C, H * W
        g = torch.Generator().manual_seed(seed)
        mk = lambda scale=1.0: (torch.randn(shape, generator=g) * scale).to("cuda").to(hb.ACT_DTYPE)  # noqa: E731
        self.u0, self.v0, self.g_last = mk(), mk(), mk(0.1)
        new = lambda: torch.empty(shape, dtype=hb.ACT_DTYPE, device="cuda")  # noqa: E731
        self.s = [new() for _ in range(STEPS)]
        self.z = [new() for _ in range(STEPS)]
        self.u = [new() for _ in range(STEPS)]
        self.dz, self.dx = new(), new()
        self.G = [new() for _ in range(STEPS)]
        self.sums = torch.zeros(STEPS, 2, C, dtype=torch.float64, device="cuda")
        self.nrep = hb.stat_replicas()
        self.bsums = torch.zeros(STEPS, self.nrep, 2, C, dtype=torch.float64, device="cuda")
        self.coef = [torch.empty(4, C, device="cuda") for _ in range(STEPS)]
        self.gamma = torch.rand(C, generator=g).to("cuda") * 0.2 + 0.4
        self.beta = (torch.rand(C, generator=g).to("cuda") - 0.5) * 0.1
        self.pg = torch.zeros(2, C, device="cuda")

    def _sum(self, a, b, out):
        hb.check(self.L.ssa_sum_act(P_(a), P_(b), None, None, P_(out), out.numel(), 0, hb._s()), "ssa_sum_act")

    def forward(self, fused):
        L, P, C = self.L, self.P, self.C
        self.sums.zero_()
        u, v = self.u0, self.v0
        for k in range(STEPS):
            s, z = self.s[k], self.z[k]
            if fused:
                hb.check(L.ssa_add_bn_stats(P_(u), C, P_(v), C, P_(s), C, P, C, P_(self.sums[k]), 0, hb._s()), "ssa_add_bn_stats")
            else:
                self._sum(u, v, s)
                hb.check(L.ssa_bn_stats(P_(s), P, C, C, P_(self.sums[k]), 0, hb._s()), "ssa_bn_stats")
            hb.check(L.ssa_bn_apply_train(P_(s), C, None, 0, P_(z), C, P, C, P_(self.sums[k]), 1, float(P), P_(self.gamma),
                                          P_(self.beta), None, None, None, 0.1, 1e-5, P_(self.coef[k]), None, 1, None, self.hw,
                                          None, hb._s()), "ssa_bn_apply_train")
            self._sum(z, None, self.u[k])               # stand-in for the block's convs
            u, v = self.u[k], s

    def backward(self, fused):
        L, P, C = self.L, self.P, self.C
        self.bsums.zero_()
        Gn = self.g_last
        for k in range(STEPS - 1, -1, -1):
            coef = self.coef[k]
            self._sum(Gn, None, self.dz)                # stand-in for the convs' data gradient
            hb.check(L.ssa_bn_bwd_reduce(P_(self.s[k]), C, P_(self.dz), C, None, 0, P, C, P_(coef[2]), P_(coef[3]), 1, None,
                                         self.hw, P_(self.bsums[k]), self.nrep, 0, P_(coef[0]), P_(coef[1]), None, hb._s()),
                     "ssa_bn_bwd_reduce")
            args = (P_(self.s[k]), C, P_(self.dz), C, None, 0, P_(self.G[k] if fused else self.dx), C, None, 0, P, C,
                    P_(self.gamma), P_(coef[2]), P_(coef[3]), P_(self.bsums[k]), self.nrep, float(P), 1, None, self.hw,
                    P_(self.pg[0]), P_(self.pg[1]), 1.0, P_(coef[0]), P_(coef[1]), 1, None)
            if fused:
                hb.check(L.ssa_bn_bwd_apply_add(*args, P_(Gn), C, hb._s()), "ssa_bn_bwd_apply_add")
            else:
                hb.check(L.ssa_bn_bwd_apply(*args, hb._s()), "ssa_bn_bwd_apply")
                self._sum(self.dx, Gn, self.G[k])
            Gn = self.G[k]


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
    return g


def replay_us(g, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 20
    rounds = int(_opt("--rounds", "9"))
    out = _opt("--json")
    results = []
    for i, shape in enumerate(SHAPES):
        ch = Chain(shape, 70 + i)
        elems = ch.P * ch.C
        # same results first (section "when results must not change"): the stored sums, z and the input gradients
        ch.forward(False), ch.backward(False)
        torch.cuda.synchronize()
        ref = [t.clone() for t in ch.s + ch.z + ch.G]
        ch.forward(True), ch.backward(True)
        torch.cuda.synchronize()
        same_s = all(torch.equal(a, b) for a, b in zip(ref[:STEPS], ch.s))
        worst = max(float((a.float() - b.float()).abs().max() / (a.float().abs().max() + 1e-30))
                    for a, b in zip(ref[STEPS:], ch.z + ch.G))
        for direction, run, bytes_f, bytes_u in (("forward", ch.forward, 7, 8), ("backward", ch.backward, 8, 10)):
            gu, gf = capture(lambda: run(False), reps), capture(lambda: run(True), reps)
            tu, tf = [], []
            for _ in range(rounds):
                tu.append(replay_us(gu, reps))
                tf.append(replay_us(gf, reps))
            mu, mf = statistics.median(tu), statistics.median(tf)
            su, sf = (max(tu) - min(tu)) / mu, (max(tf) - min(tf)) / mf
            rec = {"shape": list(shape), "direction": direction, "steps": STEPS, "dtype": str(hb.ACT_DTYPE).replace("torch.", ""),
                   "reps": reps, "rounds": rounds, "lib_sha": _lib.built_sha(),
                   "unfused_us": {"median": round(mu, 2), "min": round(min(tu), 2), "max": round(max(tu), 2), "spread": round(su, 4)},
                   "fused_us": {"median": round(mf, 2), "min": round(min(tf), 2), "max": round(max(tf), 2), "spread": round(sf, 4)},
                   "fused_over_unfused": round(mf / mu, 4), "bytes_fused_over_unfused": round(bytes_f / bytes_u, 4),
                   "fused_TBps_algorithmic": round(STEPS * elems * 2 * bytes_f / mf / 1e6, 3),
                   "unfused_TBps_algorithmic": round(STEPS * elems * 2 * bytes_u / mu / 1e6, 3),
                   "not_slower": bool(mf <= mu * (1 + max(su, sf))), "s_bit_equal": same_s, "worst_rel_difference_z_G": round(worst, 5)}
            results.append(rec)
            print("%-18s %-8s unfused %8.1f us (spread %.1f%%)  fused %8.1f us (spread %.1f%%)  ratio %.3f (bytes %.3f)  %s" % (
                "x".join(map(str, shape)), direction, mu, 100 * su, mf, 100 * sf, mf / mu, bytes_f / bytes_u,
                "ok" if rec["not_slower"] else "FUSED IS SLOWER"))
        del ch
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0 if all(r["not_slower"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
