"""The Adam / AMSGrad / RAdam kernels (csrc/adam.hip: ssa_adam_advance, ssa_adam_step) on the CPU EMULATION of the
kernel sources (tools/emu; test infrastructure, the product never loads it), through the C ABI with CPU tensors as
device memory: the golden trajectories of the reference's get_optimizer (tests/golden/adam_golden.json), longer
tensors and an unaligned view against torch.optim.Adam / the restated RAdam within the bound of adam_util, and the
skip rule of fp16 training (an overflowed step leaves p, m, v, vmax AND t untouched).  The same properties are
checked on the device through FusedAdam / FusedRAdam in tests/test_adam_gpu.py."""
import ctypes

import pytest
import torch

from adam_util import (ADAM, AMSGRAD, RADAM, BETAS, EPS, case_id, case_mode, check_bound, golden, grad_scale, poly_lr,
                       references, state_bound)

MODES = [(ADAM, "adam"), (AMSGRAD, "amsgrad"), (RADAM, "radam")]


@pytest.fixture(scope="module")
def L():
    from emu_util import emu_lib
    return emu_lib()


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class Emu:
    """The raw C ABI on CPU tensors: parameters, moment estimates and the 16-byte step records."""

    def __init__(self, L, params, mode, wd):
        self.L, self.p, self.mode, self.wd = L, params, mode, wd
        self.m = [torch.zeros(p.numel()) for p in params]
        self.v = [torch.zeros(p.numel()) for p in params]
        self.x = [torch.zeros(p.numel()) for p in params]
        self.rec = torch.zeros((len(params), 4), dtype=torch.int32)

    def step(self, grads, lr, amp=None):
        idx = [i for i, g in enumerate(grads) if g is not None]
        pick = lambda ts: _ptrs([ts[i] for i in idx])                               # noqa: E731
        R = (ctypes.c_void_p * len(idx))(*[self.rec.data_ptr() + 16 * i for i in idx])
        N = (ctypes.c_int64 * len(idx))(*[self.p[i].numel() for i in idx])
        amp_ptr = amp.data_ptr() if amp is not None else None
        assert self.L.ssa_adam_advance(R, len(idx), self.mode, BETAS[0], BETAS[1], amp_ptr, None) == 0
        assert self.L.ssa_adam_step(pick(self.p), pick(grads), pick(self.m), pick(self.v),
                                    pick(self.x) if self.mode == AMSGRAD else None, R, N, len(idx), self.mode, lr, None,
                                    BETAS[0], BETAS[1], EPS, self.wd, amp_ptr, None) == 0

    def tensors(self):
        return self.p + self.m + self.v + self.x + [self.rec]


@pytest.mark.parametrize("case", golden(), ids=case_id)
def test_golden_trajectories(L, case):
    """Every golden case, every step, every tensor within the bound; the moment estimates and the step count after the
    last step; for RAdam both branches taken (5 un-rectified steps, then 7 rectified ones)."""
    mode, wd = case_mode(case), case["case"]["weight_decay"]
    init = [torch.tensor(p, dtype=torch.float32) for p in case["init"]]
    emu = Emu(L, [t.clone() for t in init], mode, wd)
    ref32, ref64 = references(mode, init, wd)
    rect = []
    assert len(case["traj"]) >= 12
    for step, want in enumerate(case["traj"]):
        grads = [torch.tensor(g, dtype=torch.float32) for g in case["grads"][step]]
        lr = case["lrs"][step]
        emu.step(grads, lr)
        ref32.step(grads, lr)
        ref64.step(grads, lr)
        gold = [torch.tensor(w, dtype=torch.float32) for w in want]
        # the references of this test reproduce the recorded trajectory of the real reference (an ulp of slack for
        # a torch build whose CPU kernels contract multiply-adds differently from the one that recorded it)
        for r, w in zip(ref32.p, gold):
            assert float((r.detach().flatten() - w).abs().max()) <= 2.0 ** -23 * float(w.abs().max()), (step, "fp32")
        for r, w in zip(ref64.p, gold):
            assert float((r.detach().flatten() - w.double()).abs().max()) <= 1e-5, (step, "f64")
        got = check_bound(emu.p, gold, [r.flatten() for r in ref64.p], "%s step %d" % (case_id(case), step))
        print("%s step %2d lr %.5f: max |emu - f64| %.3g, max |golden - f64| %.3g, worst ratio to the bound %.2f" % (
            (case_id(case), step, lr) + got))
        rect.append(int(emu.rec[0, 1]))
        assert emu.rec[:, 0].tolist() == [step + 1] * 4
    if mode == RADAM:
        assert rect == [0] * 5 + [1] * 7, rect
        assert ref64.rectified == [False] * 5 + [True] * 7
    steps = len(case["traj"])
    gmax = max(abs(x) for gs in case["grads"] for g in gs for x in g) + wd * 2.0
    for i, st in enumerate(case["state"]):
        assert float(st["step"]) == steps
        for name, mine, hist in (("exp_avg", emu.m, gmax), ("exp_avg_sq", emu.v, gmax * gmax)) + (
                (("max_exp_avg_sq", emu.x, gmax * gmax),) if mode == AMSGRAD else ()):
            err = float((mine[i] - torch.tensor(st[name], dtype=torch.float32)).abs().max())
            assert err <= state_bound(steps, hist), (name, i, err)


@pytest.mark.parametrize("mode,name", MODES)
def test_longer_tensors_and_an_unaligned_view(L, mode, name):
    """Sizes around the 4096-element chunk, a tensor of many chunks, an unaligned view (scalar path), a parameter
    without a gradient until step 3 (its own t) -- 16 steps, the learning rate changing every step."""
    sizes, steps, wd = (7, 4096, 4097, 100003, 33), 16, 1e-4
    g = torch.Generator().manual_seed(21)
    init = [torch.randn(n, generator=g) for n in sizes] + [torch.randn(1001, generator=g)[1:], torch.randn(50, generator=g)]
    mine = [t.clone() for t in init[:-2]] + [torch.cat([torch.zeros(1), init[-2]])[1:], init[-1].clone()]
    assert mine[-2].data_ptr() % 16 == 4
    emu = Emu(L, mine, mode, wd)
    ref32, ref64 = references(mode, init, wd)
    for step in range(steps):
        grads = [torch.randn(t.shape, generator=g) * grad_scale(step) for t in init]
        if step < 3:
            grads[-1] = None
        lr = poly_lr(1e-2, step, steps)
        for o in (emu, ref32, ref64):
            o.step(grads, lr)
        got = check_bound(emu.p, ref32.p, ref64.p, "%s step %d" % (name, step))
        print("%s step %2d lr %.5f: max |emu - f64| %.3g, max |reference - f64| %.3g, worst ratio to the bound %.2f" % (
            (name, step, lr) + got))
    assert emu.rec[:, 0].tolist() == [steps] * (len(init) - 1) + [steps - 3]
    if mode == RADAM:
        assert emu.rec[:, 1].tolist() == [1] * len(init)


@pytest.mark.parametrize("mode,name", MODES)
@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_an_overflowed_step_never_happened(L, mode, name, bad):
    """One bad element in one gradient: p, m, v, vmax and the step records stay bit-identical and the scale halves; the
    next clean step equals the step of a twin that never saw the overflow, at the halved scale."""
    sizes = (7, 4096, 4097, 100003, 33)
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(n, generator=g) for n in sizes]
    runs = [Emu(L, [t.clone() for t in init], mode, 1e-4) for _ in range(2)]
    states = [torch.tensor([512.0, 0.0, 0.0, 1.0 / 512.0]) for _ in range(2)]

    def scaled_step(k, true, lr):
        S = float(states[k][0])
        grads = [t * S for t in true]
        assert L.ssa_amp_check_grads(_ptrs(grads), (ctypes.c_int64 * len(grads))(*[t.numel() for t in grads]),
                                     len(grads), states[k].data_ptr(), None) == 0
        runs[k].step(grads, lr, states[k])
        assert L.ssa_amp_update(states[k].data_ptr(), 2000, 2.0, 0.5, 1.0, 2.0 ** 24, None) == 0

    for step in range(6 if mode == RADAM else 3):            # (RAdam: into the rectified branch)
        true = [torch.randn(n, generator=g) for n in sizes]
        for k in range(2):
            scaled_step(k, true, 1e-2)
    assert all(torch.equal(a, b) for a, b in zip(runs[0].tensors(), runs[1].tensors()))
    before = [t.clone() for t in runs[0].tensors()]
    true = [torch.randn(n, generator=g) for n in sizes]
    true[3][77777] = bad                                     # in the scalar tail of a later chunk of the fourth tensor
    scaled_step(0, true, 1e-2)
    assert all(torch.equal(a, b) for a, b in zip(runs[0].tensors(), before)), "a skipped step changed something"
    assert states[0].tolist()[:3] == [256.0, 0.0, 0.0]
    states[1].copy_(torch.tensor([256.0, 0.0, 0.0, 1.0 / 256.0]))
    true = [torch.randn(n, generator=g) for n in sizes]
    for k in range(2):
        scaled_step(k, true, 5e-3)
    assert all(torch.equal(a, b) for a, b in zip(runs[0].tensors(), runs[1].tensors()))
    assert int(runs[0].rec[0, 0]) == (7 if mode == RADAM else 4)


def test_scaled_steps_equal_the_unscaled_recursion(L):
    """With a scaler the gradients are multiplied by 1 / S on the way in: S a power of two, so the scaled run is
    bit-identical to the plain one."""
    g = torch.Generator().manual_seed(6)
    init = [torch.randn(n, generator=g) for n in (33, 4097)]
    for mode, _ in MODES:
        a, b = (Emu(L, [t.clone() for t in init], mode, 1e-4) for _ in range(2))
        state = torch.tensor([1024.0, 0.0, 0.0, 1.0 / 1024.0])
        for step in range(7):
            true = [torch.randn(t.shape, generator=g) for t in init]
            a.step(true, 1e-2)
            b.step([t * 1024.0 for t in true], 1e-2, state)
        assert all(torch.equal(x, y) for x, y in zip(a.tensors(), b.tensors()))


def test_invalid_arguments_are_refused(L):
    p, rec = [torch.zeros(8)], torch.zeros((1, 4), dtype=torch.int32)
    R = (ctypes.c_void_p * 1)(rec.data_ptr())
    N = (ctypes.c_int64 * 1)(8)
    ok = (_ptrs(p), _ptrs(p), _ptrs(p), _ptrs(p), None, R, N, 1, 0, 1e-3, None, 0.9, 0.999, 1e-8, 0.0, None, None)
    assert L.ssa_adam_step(*ok) == 0

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a
    assert L.ssa_adam_step(*with_(8, 3)) == -1               # mode
    assert L.ssa_adam_step(*with_(8, 1)) == -1               # AMSGrad without max_exp_avg_sq
    assert L.ssa_adam_step(*with_(11, 1.0)) == -1            # beta1
    assert L.ssa_adam_step(*with_(12, -0.1)) == -1           # beta2
    assert L.ssa_adam_step(*with_(13, -1e-8)) == -1          # eps
    assert L.ssa_adam_step(*with_(14, -1.0)) == -1           # weight decay
    assert L.ssa_adam_step(*with_(2, None)) == -1            # exp_avg
    assert L.ssa_adam_step(*with_(5, (ctypes.c_void_p * 1)(rec.data_ptr() + 4))) == -1       # misaligned record
    assert L.ssa_adam_advance(None, 1, 0, 0.9, 0.999, None, None) == -1
    assert L.ssa_adam_advance(R, 1, 5, 0.9, 0.999, None, None) == -1
    assert L.ssa_adam_advance(R, 1, 0, 0.9, 1.0, None, None) == -1
    assert torch.equal(rec, torch.zeros((1, 4), dtype=torch.int32))
