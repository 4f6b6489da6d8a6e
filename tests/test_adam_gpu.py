"""ssa_adam_advance / ssa_adam_step through semseg_amd.loss.optimizer.FusedAdam / FusedRAdam on the device:
parity with torch.optim.Adam(foreach=False), the restated RAdam and the reference's golden trajectories within the
bound of adam_util (measured against float64 runs of the same trajectory), the learning rate from the device
scalar, version counters, the step captured in a graph (the step count and RAdam's branch live on the device), the
loss scaler's skip rule, and semseg_amd.graph_training with both optimizers.

Measured on an MI355X (profiles/adam_gpu_tests.log): worst ratio to the bound 0.48 (parity), 0.43 (golden)."""
import math

import pytest
import torch

from adam_util import (ADAM, AMSGRAD, RADAM, SHAPES, case_id, case_mode, check_bound, golden, grad_scale, references)
from util import ACT_DTYPE

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = (1, 3, 7, 19, 4095, 4096, 4097, 720 * 512 * 9, 100003) + tuple(range(5, 5 + 120))   # > 2 x 56 tensors: 3 launches
KINDS = [(ADAM, "adam"), (AMSGRAD, "amsgrad"), (RADAM, "radam")]


def _make(mode, params, lr=1e-2, wd=1e-4):
    from semseg_amd.loss.optimizer import FusedAdam, FusedRAdam
    if mode == RADAM:
        return FusedRAdam(params, lr=lr, weight_decay=wd)
    return FusedAdam(params, lr=lr, weight_decay=wd, amsgrad=mode == AMSGRAD)


def _state_names(mode):
    return ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if mode == AMSGRAD else ())


def _everything(opt, params, mode):
    """Parameters, every state tensor and the step counts: what two runs of the same kernels must agree on bit for bit."""
    out = [p.detach() for p in params]
    for p in params:
        out += [opt.state[p][k] for k in _state_names(mode) if k in opt.state.get(p, {})]
    return out, opt.step_counts()


def _same(a, b):
    return a[1] == b[1] and len(a[0]) == len(b[0]) and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


@pytest.mark.parametrize("mode,name", KINDS)
def test_parity_with_torch_and_the_restated_radam(mode, name):
    """More tensors than one launch holds, an unaligned view, a parameter that never gets a gradient and one that gets
    its first at step 3 (its bias correction starts at t = 1 then); four learning rates."""
    g = torch.Generator().manual_seed(11)
    init = [torch.randn(n, generator=g) for n in SIZES]
    base = torch.randn(1001, generator=g)
    init += [base[1:], torch.randn(300, generator=g)]        # the unaligned view; the late parameter
    mine = [t.clone().to(DEV).requires_grad_(True) for t in init[:-2]]
    mine.append(base.clone().to(DEV)[1:].requires_grad_(True))
    assert mine[-1].data_ptr() % 16 == 4
    mine.append(init[-1].clone().to(DEV).requires_grad_(True))
    idle = torch.ones(8, device=DEV, requires_grad=True)
    opt = _make(mode, mine + [idle])
    ref32, ref64 = references(mode, init, 1e-4, DEV)
    lrs = (1e-2, 1e-2, 5e-3, 2e-3, 1e-3, 1e-3, 5e-3)
    for step, lr in enumerate(lrs):
        grads = [torch.randn(t.shape, generator=g).to(DEV) * grad_scale(step) for t in init]
        if step < 3:
            grads[-1] = None
        for p, gr in zip(mine, grads):
            p.grad = gr
        opt.param_groups[0]["lr"] = lr
        opt.step()
        ref32.step(grads, lr)
        ref64.step(grads, lr)
        torch.cuda.synchronize()
        got = check_bound(mine, ref32.p, ref64.p, "%s step %d" % (name, step))
        print("%s step %d lr %.4f: max |fused - f64| %.3g, max |reference - f64| %.3g, worst ratio to the bound %.2f" % (
            (name, step, lr) + got))
    assert torch.equal(idle, torch.ones(8, device=DEV)) and not opt.state.get(idle)
    assert opt.step_counts() == [len(lrs)] * (len(mine) - 1) + [len(lrs) - 3, 0]


@pytest.mark.parametrize("case", golden(), ids=case_id)
def test_golden_trajectories_on_the_device(case):
    mode, wd = case_mode(case), case["case"]["weight_decay"]
    init = [torch.tensor(p, dtype=torch.float32).reshape(s) for p, s in zip(case["init"], SHAPES)]
    mine = [t.clone().to(DEV).requires_grad_(True) for t in init]
    opt = _make(mode, mine, lr=case["case"]["lr"], wd=wd)
    _, ref64 = references(mode, init, wd)
    rect = []
    for step, want in enumerate(case["traj"]):
        grads = [torch.tensor(g, dtype=torch.float32).reshape(s) for g, s in zip(case["grads"][step], SHAPES)]
        for p, gr in zip(mine, grads):
            p.grad = gr.to(DEV)
        opt.param_groups[0]["lr"] = case["lrs"][step]
        opt.step()
        ref64.step(grads, case["lrs"][step])
        gold = [torch.tensor(w, dtype=torch.float32).reshape(s) for w, s in zip(want, SHAPES)]
        got = check_bound(mine, gold, ref64.p, "%s step %d" % (case_id(case), step))
        print("%s step %2d: max |fused - f64| %.3g, max |golden - f64| %.3g, worst ratio to the bound %.2f" % (
            (case_id(case), step) + got))
        rect.append(int(opt._rec[mine[0].device][0, 1]))
    assert opt.step_counts() == [12] * 4
    if mode == RADAM:
        assert rect == [0] * 5 + [1] * 7, rect               # both branches, taken on the device


@pytest.mark.parametrize("mode,name", KINDS)
def test_lr_from_the_device_scalar_and_version_counters(mode, name):
    """sync_lr() is what a captured step relies on; autograd and the packed-filter cache rely on ._version."""
    p = torch.zeros(1000, device=DEV, requires_grad=True)
    opt = _make(mode, [p], lr=1.0, wd=0.0)
    p.grad = torch.ones_like(p)
    v0 = p._version
    opt.step()
    assert p._version > v0
    sv = {k: opt.state[p][k]._version for k in _state_names(mode)}
    first = float(p.detach()[0])
    assert first < 0 and torch.equal(p.detach(), torch.full_like(p, first))
    opt.param_groups[0]["lr"] = 0.25
    opt.sync_lr()
    assert float(opt._lr_dev[0][0]) == 0.25
    opt.param_groups[0]["lr"] = 1.0                          # the kernel must read the scalar, not this
    opt._lr_dev[0][1] = 1.0                                  # (and step() must not refresh it)
    opt.step()
    second = float(p.detach()[0]) - first
    assert all(opt.state[p][k]._version > v for k, v in sv.items())
    assert abs(second / first - 0.25) < 1e-3, (first, second)   # (g = 1 twice: m / sqrt(v) is 1 at both steps)


def test_step_refreshes_packed_filters():
    """A conv after FusedAdam.step() must see the updated weights (the check of
    test_optim_gpu.py::test_fused_sgd_step_refreshes_packed_filters)."""
    from semseg_amd import ops
    from semseg_amd.nn import Conv2d
    torch.manual_seed(0)
    conv = Conv2d(16, 16, kernel_size=3, padding=1, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(conv.weight.sign() * 0.5)
    x = torch.randn(1, 8, 8, 16, device=DEV).to(ACT_DTYPE)
    B = ops.HipBackend()
    B.begin_step(x.device)
    y0 = B.conv2d(x, conv.weight, None, 1, 1, 1).detach().float()
    opt = _make(ADAM, conv.parameters(), lr=0.5, wd=0.0)     # first Adam step: p -= lr * sign(g) -> 0 (to eps)
    conv.weight.grad = conv.weight.detach().clone()
    opt.step()
    B.begin_step(x.device)
    y1 = B.conv2d(x, conv.weight, None, 1, 1, 1).detach().float()
    assert float(y0.abs().max()) > 0.1 and float(y1.abs().max()) < 1e-4


@pytest.mark.parametrize("mode,name", KINDS)
def test_captured_step_counts_and_branches_on_the_device(mode, name):
    """One eager step, then the step captured and replayed 8 times with fresh gradients in static buffers and the LR
    changed through sync_lr(): bit for bit the 9 eager steps of a twin; the device step count reads 9 (RAdam crosses
    step 6 inside the replays)."""
    N = 8
    g = torch.Generator().manual_seed(4)
    init = [torch.randn(n, generator=g) for n in (7, 4096, 4097, 100003, 33) + tuple(range(5, 65))]
    grads = [[torch.randn(t.shape, generator=g).to(DEV) * grad_scale(s) for t in init] for s in range(N + 1)]
    lrs = [1e-2 * math.pow(1 - s / (N + 2), 2.0) for s in range(N + 1)]
    twin = [t.clone().to(DEV).requires_grad_(True) for t in init]
    ot = _make(mode, twin)
    for s in range(N + 1):
        for p, gr in zip(twin, grads[s]):
            p.grad = gr
        ot.param_groups[0]["lr"] = lrs[s]
        ot.step()
    mine = [t.clone().to(DEV).requires_grad_(True) for t in init]
    om = _make(mode, mine)
    static = [gr.clone() for gr in grads[0]]
    for p, gr in zip(mine, static):
        p.grad = gr
    om.param_groups[0]["lr"] = lrs[0]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        om.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        om.step()
    assert om.step_counts() == [1] * len(init)               # a capture runs nothing
    rect = []
    for s in range(1, N + 1):
        for st, gr in zip(static, grads[s]):
            st.copy_(gr)
        om.param_groups[0]["lr"] = lrs[s]
        om.sync_lr()
        graph.replay()
        rect.append(int(om._rec[mine[0].device][0, 1]))
    torch.cuda.synchronize()
    assert om.step_counts() == [N + 1] * len(init)
    assert _same(_everything(om, mine, mode), _everything(ot, twin, mode))
    if mode == RADAM:
        assert rect == [0] * 4 + [1] * 4, rect


@pytest.mark.parametrize("mode,name", KINDS)
def test_loss_scaler_on_the_device(mode, name):
    """Un-scaled updates equal the plain recursion (S a power of two: bit for bit); an overflow skips everything
    including t and halves the scale; the next clean step is the one of a twin that never saw the overflow."""
    from semseg_amd.amp import LossScaler
    g = torch.Generator().manual_seed(3)
    init = [torch.randn(n, generator=g) for n in (7, 4096, 4097, 100003, 33)]
    mine = [t.clone().to(DEV).requires_grad_(True) for t in init]
    twin = [t.clone().to(DEV).requires_grad_(True) for t in init]
    om, ot = _make(mode, mine), _make(mode, twin)
    om.loss_scaler = LossScaler(torch.device(DEV), init_scale=1024.0, growth_interval=2000)
    clean = 6 if mode == RADAM else 3
    for step in range(clean):
        S = om.loss_scaler.loss_scale()
        for p, q in zip(mine, twin):
            gr = torch.randn(p.shape, generator=g)
            q.grad = gr.to(DEV)
            p.grad = (gr * S).to(DEV)                        # what backward of loss * S leaves
        om.step()
        ot.step()
    torch.cuda.synchronize()
    assert _same(_everything(om, mine, mode), _everything(ot, twin, mode))
    for bad in (float("inf"), float("-inf"), float("nan")):
        S = om.loss_scaler.loss_scale()
        for p in mine:
            p.grad = torch.randn(p.shape, generator=g).to(DEV) * S
        mine[3].grad[77777] = bad
        om.step()
        torch.cuda.synchronize()
        assert _same(_everything(om, mine, mode), _everything(ot, twin, mode)), "a skipped step changed something"
        st = om.loss_scaler.state.cpu().tolist()
        assert st[0] == S / 2 and st[1] == 0.0 and st[2] == 0.0, st
    assert om.step_counts() == [clean] * len(init)
    S = om.loss_scaler.loss_scale()
    assert S == 128.0
    for p, q in zip(mine, twin):
        gr = torch.randn(p.shape, generator=g)
        q.grad = gr.to(DEV)
        p.grad = (gr * S).to(DEV)
    om.step()
    ot.step()
    torch.cuda.synchronize()
    assert _same(_everything(om, mine, mode), _everything(ot, twin, mode))
    assert om.step_counts() == [clean + 1] * len(init)
    sd = om.state_dict()
    assert sd["loss_scaler"]["loss_scale"] == 128.0 and sd["loss_scaler"]["skipped_steps"] == 3


class _Tiny(torch.nn.Module):
    """Dict input -> scalar loss on plain torch ops (no atomics: eager and replay run the same arithmetic)."""

    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(16, 32)
        self.b = torch.nn.Linear(32, 4)

    def forward(self, inputs):
        return (self.b(torch.tanh(self.a(inputs["x"]))) - inputs["y"]).square().mean()


@pytest.mark.parametrize("mode,name", KINDS)
def test_graph_training_equals_the_eager_loop_bit_for_bit(mode, name):
    """The reference's loop under the proxies against the same loop run eagerly, 9 iterations, a scheduler in between:
    after EVERY iteration -- the first one, whose capture took two warm-up passes, included -- parameters, moment
    estimates and step counts are identical (the warm-up left no trace; t counts loop iterations)."""
    import semseg_amd
    N = 9
    torch.manual_seed(0)
    eager, graphed = _Tiny().to(DEV).train(), _Tiny().to(DEV).train()
    graphed.load_state_dict(eager.state_dict())
    g = torch.Generator().manual_seed(8)
    batches = [{"x": torch.randn(8, 16, generator=g).to(DEV), "y": torch.randn(8, 4, generator=g).to(DEV)} for _ in range(N)]
    oe, og = _make(mode, eager.parameters()), _make(mode, graphed.parameters())
    sched = lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda e: math.pow(1 - e / (N + 2), 2.0))   # noqa: E731
    se, sg = sched(oe), sched(og)
    gnet, goptim = semseg_amd.graph_training(graphed, og)
    for it, inputs in enumerate(batches):
        losses = []
        for net, optim, sch in ((eager, oe, se), (gnet, goptim, sg)):
            optim.zero_grad()
            loss = net(inputs).mean()
            losses.append(float(loss.detach()))
            loss.backward()
            optim.step()
            sch.step()
        torch.cuda.synchronize()
        assert losses[0] == losses[1], (it, losses)
        assert og.step_counts() == [it + 1] * 4, (it, og.step_counts())
        assert _same(_everything(og, list(graphed.parameters()), mode), _everything(oe, list(eager.parameters()), mode)), it
    assert gnet._stepper.replays == N and not gnet._stepper.eager_only


@pytest.mark.parametrize("mode,name", [(AMSGRAD, "amsgrad"), (RADAM, "radam")])
def test_graph_training_of_hrnet_mscale(mode, name):
    """HRNet-OCR-MScale as tests/test_graphed_step_gpu.py builds it, three iterations under the proxies: the first loss
    is the eager loop's (it does not depend on the optimizer; that test's 2e-3), every loss is finite, every
    parameter's device step count is 3.  Weights are NOT compared: BatchNorm's atomic sums differ in the last bits
    between eager and replay, and Adam's normalised update turns a last-bit difference of a near-zero gradient into a
    full +-lr step -- such a comparison would test the atomics."""
    import semseg_amd
    import __graft_entry__ as ge
    from test_graphed_step_gpu import _build, _reference_loop
    batches = []
    for i in range(3):
        images, gts = ge._synth(1, 256, 256, 40 + i, DEV)
        batches.append({"images": images, "gts": gts})
    net, _ = _build()
    init = {k: v.clone() for k, v in net.state_dict().items()}
    eager = _reference_loop(net, _make(mode, net.parameters(), lr=1e-4), batches[:1])
    del net
    net2, _ = _build()
    net2.load_state_dict(init)
    opt = _make(mode, net2.parameters(), lr=1e-4)
    gnet, goptim = semseg_amd.graph_training(net2, opt)
    graphed = _reference_loop(gnet, goptim, batches)
    print(name, "eager", eager, "graphed", graphed)
    assert abs(eager[0] - graphed[0]) <= 2e-3 * abs(eager[0]), (eager, graphed)
    assert all(math.isfinite(v) for v in graphed)
    assert gnet._stepper.replays == 3 and not gnet._stepper.eager_only
    counts = opt.step_counts()
    assert len(counts) == len(list(net2.parameters())) and set(counts) == {3}, sorted(set(counts))
