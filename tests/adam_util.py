"""Shared by the Adam / AMSGrad / RAdam tests: the golden trajectories of the reference, the references the
parity bound is measured against, and the bound itself.

The bound (per tensor and per step):   max|mine - f64| <= 2 * max|reference_fp32 - f64| + one ulp of the largest |p|.
Against torch and the reference the kernel may round in a different, equally valid order (fused multiply-adds, the
bias corrections precomputed in double and rounded once), so the yardstick is what the reference itself loses in
fp32 against the same trajectory in float64; the factor 2 is the sum of two independent rounding histories of the
same length, the ulp floor covers tensors where the reference happens to round exactly."""
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_golden.json")
SHAPES = [(5, 7), (5,), (3, 5), (3,)]
ADAM, AMSGRAD, RADAM = 0, 1, 2
BETAS, EPS = (0.9, 0.999), 1e-8


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def case_mode(case):
    c = case["case"]
    return RADAM if c["optimizer"] == "radam" else (AMSGRAD if c["amsgrad"] else ADAM)


def case_id(case):
    c = case["case"]
    return "%s%s-wd%g" % (c["optimizer"], "-amsgrad" if c["amsgrad"] else "", c["weight_decay"])


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def grad_scale(step):
    """The gradient scale jumps by 100x every three steps, up and down (AMSGrad's running maximum matters)."""
    return 0.01 * (100.0 if (step // 3) % 2 else 1.0)


def poly_lr(lr0, step, steps, power=2.0):
    return lr0 * math.pow(1.0 - step / (steps + 2.0), power)


class RAdamRestated:
    """The recursion of the reference's RAdam, restated on tensors of any dtype (float32: the reference's own
    arithmetic, checked against the golden trajectories; float64: the yardstick).  Per parameter: its own step count
    t;  v = b2 v + (1 - b2) g^2, then m = b1 m + (1 - b1) g;  N_sma = N_max - 2 t b2^t / (1 - b2^t);  the decay scales p
    by (1 - wd lr) before the update;  N_sma >= 5: p -= lr sqrt((1 - b2^t)(N_sma - 4)/(N_max - 4)(N_sma - 2)/N_sma
    N_max/(N_max - 2)) / (1 - b1^t) * m / (sqrt(v) + eps), else p -= lr / (1 - b1^t) * m."""

    def __init__(self, params, betas=BETAS, eps=EPS, weight_decay=0.0):
        self.p = params
        self.m = [torch.zeros_like(p) for p in params]
        self.v = [torch.zeros_like(p) for p in params]
        self.t = [0] * len(params)
        self.b1, self.b2 = betas
        self.eps, self.wd = eps, weight_decay
        self.rectified = []                  # per step() call: was the first updated parameter's step rectified

    def step(self, grads, lr):
        flagged = False
        for i, (p, g) in enumerate(zip(self.p, grads)):
            if g is None:
                continue
            g = g.to(p.dtype)
            self.v[i].mul_(self.b2).addcmul_(g, g, value=1 - self.b2)
            self.m[i].mul_(self.b1).add_(g, alpha=1 - self.b1)
            self.t[i] += 1
            t = self.t[i]
            b2t = self.b2 ** t
            n_max = 2 / (1 - self.b2) - 1
            n_sma = n_max - 2 * t * b2t / (1 - b2t)
            if not flagged:
                self.rectified.append(n_sma >= 5)
                flagged = True
            if self.wd != 0:
                p.add_(p, alpha=-self.wd * lr)
            if n_sma >= 5:
                size = lr * math.sqrt((1 - b2t) * (n_sma - 4) / (n_max - 4) * (n_sma - 2) / n_sma * n_max /
                                      (n_max - 2)) / (1 - self.b1 ** t)
                p.addcdiv_(self.m[i], self.v[i].sqrt().add_(self.eps), value=-size)
            else:
                p.add_(self.m[i], alpha=-lr / (1 - self.b1 ** t))


class TorchAdam:
    """torch.optim.Adam(foreach=False) on copies of `init` in `dtype` on `device`, stepped with explicit gradients
    (None: no gradient in that step) and learning rates."""

    def __init__(self, init, dtype, device, weight_decay, amsgrad):
        self.p = [t.detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for t in init]
        self.opt = torch.optim.Adam(self.p, lr=1e-3, betas=BETAS, eps=EPS, weight_decay=weight_decay, amsgrad=amsgrad,
                                    foreach=False)

    def step(self, grads, lr):
        for p, g in zip(self.p, grads):
            p.grad = None if g is None else g.to(device=p.device, dtype=p.dtype)
        self.opt.param_groups[0]["lr"] = lr
        self.opt.step()


def references(mode, init, weight_decay, device="cpu"):
    """(fp32 reference, float64 yardstick) for `mode` on copies of `init`: objects with .p and .step(grads, lr)."""
    if mode == RADAM:
        return tuple(RAdamRestated([t.detach().to(device=device, dtype=dt).clone() for t in init],
                                   weight_decay=weight_decay) for dt in (torch.float32, torch.float64))
    return tuple(TorchAdam(init, dt, device, weight_decay, mode == AMSGRAD) for dt in (torch.float32, torch.float64))


def check_bound(mine, ref32, ref64, what):
    """Asserts the bound for every tensor; returns (worst |mine - f64|, worst |reference - f64|, worst ratio to the
    bound) for the printout."""
    worst_m = worst_r = worst_q = 0.0
    for i, (a, r, d) in enumerate(zip(mine, ref32, ref64)):
        d = d.detach().double().cpu()
        em = float((a.detach().double().cpu() - d).abs().max())
        er = float((r.detach().double().cpu() - d).abs().max())
        bound = 2.0 * er + ulp32(float(d.abs().max()))
        assert em <= bound, "%s, tensor %d: |mine - f64| %.3g > 2 * |reference - f64| %.3g + ulp = %.3g" % (
            what, i, em, er, bound)
        worst_m, worst_r, worst_q = max(worst_m, em), max(worst_r, er), max(worst_q, em / bound)
    return worst_m, worst_r, worst_q


def state_bound(steps, history_max):
    """Bound on a moment estimate against the reference's: every step is one convex combination of the old value and
    a term no larger than `history_max`, each rounding within an ulp of its result on either side -- two rounding
    histories of `steps` steps with up to two roundings per step."""
    return 2 * 2 * steps * 2.0 ** -24 * history_max
