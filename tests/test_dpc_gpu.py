"""The Dense Prediction Cell on the HIP kernels (csrc/conv_dil.hip through ops.dil_conv_bn_act):

  * the cell alone, op by op, against the oracle -- the scheme and the bounds of tests/test_deeper_gpu.py / test_deepv3_gpu.py
    unchanged (the measured storage noise floor of tests/bf16_emu_backend.py bounds the HIP path op by op; gradients by
    the cosine rules of the train-step tests), 256 -> 64 channels at 48 x 52, in training and in evaluation mode;
  * one training step of DeepV3Plus(19, 'resnet-50', use_dpc=True) at 384 x 416 (48 x 52 at stride 8: every rate pair has
    off-centre taps inside the map) on the golden batch of the real reference: the oracle run is held to the golden's
    loss, the HIP run to the oracle by the end-to-end rules;
  * a captured step (hipGraph) replayed on two inputs against the eager steps;
  * the new route at dil_h == dil_w against the existing conv route, element for element within the one-rounding bound
    of tests/test_deeper_gpu.py::test_conv5x5_through_ops_against_the_generic_route."""
import os

import pytest
import torch

from util import ACT_DTYPE
import dpc_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"            # (the emulation run of the suite swaps it: tests/conftest.py)
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIN, C, H, W, B = 256, 64, 48, 52, 2


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _cos(a, b):
    return float((a * b).sum() / (a.norm() * b.norm() + 1e-30))


def _traced(backend, sink):
    """bf16_emu_backend.traced for the one op of the cell: every TOP-LEVEL dil_conv_bn_act call reports its outputs
    (BackendBase maps a list over single calls, the HIP backend runs it as one: the same tensors in the same order)."""
    depth = [0]
    inner = type(backend).dil_conv_bn_act

    class Traced(type(backend)):
        def dil_conv_bn_act(self, *a, **k):
            depth[0] += 1
            try:
                y = inner(self, *a, **k)
            finally:
                depth[0] -= 1
            if depth[0] == 0:
                for t in (y if isinstance(y, (list, tuple)) else (y,)):
                    sink(t)
            return y
    backend.__class__ = Traced
    return backend


def _cell_run(backend, sd, x, gy, train, device="cpu", hip=False):
    from semseg_amd import ops
    from semseg_amd.network.deepv3 import DPC
    prev = ops._BACKEND
    ops._set_backend_for_tests(backend)
    try:
        cell = DPC(CIN, C, output_stride=8)
        cell.load_state_dict(sd)
        cell = cell.to(device).train(train)
        xin = x.to(device).to(ACT_DTYPE if hip else x.dtype).detach().clone().requires_grad_(train)
        backend.begin_step(xin.device) if hasattr(backend, "begin_step") else None
        if not train:
            with torch.no_grad():
                return cell(xin).float().cpu(), None
        out = cell(xin)
        backend.end_forward() if hasattr(backend, "end_forward") else None
        out.backward(gy.to(device).to(out.dtype))
        if hip:
            torch.cuda.synchronize()
        grads = {n: p.grad.detach().float().cpu() for n, p in cell.named_parameters()}
        grads["<input>"] = xin.grad.detach().float().cpu()
        return out.detach().float().cpu(), grads
    finally:
        ops._set_backend_for_tests(prev)


@pytest.fixture(scope="module")
def cell_setup():
    from oracle.model import seeded_state_dict
    sd = seeded_state_dict(R.module_shapes(CIN, C), seed=21)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(B, H, W, CIN, generator=g).to(ACT_DTYPE).float()
    gy = torch.randn(B, H, W, 5 * C, generator=g).to(ACT_DTYPE).float()
    R.assert_taps_inside(H, W, 8)
    return sd, x, gy


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
def test_dpc_cell_op_by_op(cell_setup, train):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    sd, x, gy = cell_setup
    ref_log, emu_err, hip_err = [], [], []
    ref, gr = _cell_run(_traced(OracleBackend(), lambda y: ref_log.append(y.detach())), sd, x, gy, train)
    emu, ge = _cell_run(_traced(Bf16EmuBackend(), lambda y: emu_err.append(_rel(y.detach(), ref_log[len(emu_err)]))), sd, x, gy, train)
    hip, gh = _cell_run(_traced(ops.HipBackend(), lambda y: hip_err.append(_rel(y.detach().float().cpu(), ref_log[len(hip_err)]))),
                        sd, x, gy, train, device=DEV, hip=True)
    assert len(ref_log) == len(emu_err) == len(hip_err) == 5
    for i, n in enumerate(R.NAMES):
        print("DPC %s layer %s: hip %.5f emu %.5f" % ("train" if train else "eval", n, hip_err[i], emu_err[i]))
    bad = [(R.NAMES[i], hip_err[i], emu_err[i]) for i in range(5) if not hip_err[i] <= 1.5 * emu_err[i] + 5e-3]
    assert not bad, bad
    assert tuple(hip.shape) == (B, H, W, 5 * C) and torch.isfinite(hip).all()
    print("DPC output rel err hip %.5f emu %.5f" % (_rel(hip, ref), _rel(emu, ref)))
    assert _rel(hip, ref) <= 1.5 * _rel(emu, ref) + 5e-3
    if not train:
        return
    assert sorted(gh) == sorted(gr) and all(torch.isfinite(g).all() for g in gh.values())
    vh, ve = sorted(_cos(gh[n], gr[n]) for n in gr), sorted(_cos(ge[n], gr[n]) for n in gr)
    print("grad cosine vs oracle: hip min %.4f p10 %.4f median %.4f | emu min %.4f p10 %.4f median %.4f (n=%d)" % (
        vh[0], vh[len(vh) // 10], vh[len(vh) // 2], ve[0], ve[len(ve) // 10], ve[len(ve) // 2], len(vh)))
    assert vh[len(vh) // 2] >= ve[len(ve) // 2] - 0.10 and vh[len(vh) // 10] >= ve[len(ve) // 10] - 0.15
    for n, r in gr.items():
        ce, ch = _cos(ge[n], r), _cos(gh[n], r)
        assert not (ce >= 0.5 and ch < 0.5 * ce), (n, ch, ce)


# ---- the network
def _shapes():
    out = []
    with open(os.path.join(G, "keys_deepv3_dpc.txt")) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


def _build(sd):
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network.deepv3 import DeepV3Plus
    cfg.MODEL.BNFUNC = None
    cfg.MODEL.N_SCALES = None
    net = DeepV3Plus(19, trunk="resnet-50", criterion=CrossEntropyLoss2d(ignore_index=255), use_dpc=True)
    net.load_state_dict(sd)
    return net


def _net_run(backend, sd, images, gts, device="cpu"):
    from semseg_amd import ops
    prev = ops._BACKEND
    ops._set_backend_for_tests(backend)
    try:
        net = _build(sd).to(device).train()
        loss = net({"images": images.to(device), "gts": gts.to(device)})
        loss.backward()
        if device != "cpu":
            torch.cuda.synchronize()
        return float(loss.detach()), {n: p.grad.detach().float().cpu() for n, p in net.named_parameters()}
    finally:
        ops._set_backend_for_tests(prev)


@pytest.fixture(scope="module")
def net_setup():
    from oracle.model import seeded_state_dict
    gold = torch.load(os.path.join(G, "dpc_golden.pt"), map_location="cpu", weights_only=False)["net"]
    Bn, Hn, Wn, seed = gold["batch"]
    assert (Bn, Hn, Wn) == (2, 384, 416)
    images, gts = R.synth_batch(Bn, Hn, Wn, seed=seed)
    return gold, seeded_state_dict(_shapes(), seed=gold["seed"]), images, gts


def test_deepv3_dpc_train_step(net_setup):
    """The golden's weights and batch, undamped.  The oracle run reproduces the reference's loss (1e-5) and gradient
    norms; the HIP run is held to it by test_deepv3_gpu's / test_e2e_gpu's rules, with the emulated-storage run as the
    noise floor."""
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    gold, sd, images, gts = net_setup
    lr, gr = _net_run(OracleBackend(), sd, images, gts)
    assert abs(lr - float(gold["train_loss"])) <= 1e-5 * abs(float(gold["train_loss"])) + 1e-5, (lr, float(gold["train_loss"]))
    le, ge = _net_run(Bf16EmuBackend(), sd, images, gts)
    lh, gh = _net_run(ops.HipBackend(), sd, images, gts, device=DEV)
    print("deepv3+dpc train loss hip %.6f emu %.6f oracle %.6f golden %.6f" % (lh, le, lr, float(gold["train_loss"])))
    assert abs(lh - lr) <= 2e-3 * abs(lr) + 2 * abs(le - lr)

    def cosines(g):
        return sorted(_cos(g[n], r) for n, r in gr.items() if float(r.norm()) > 1e-10)
    vh, ve = cosines(gh), cosines(ge)
    print("grad cosine vs oracle: hip min %.4f p10 %.4f median %.4f | emu min %.4f p10 %.4f median %.4f (n=%d)" % (
        vh[0], vh[len(vh) // 10], vh[len(vh) // 2], ve[0], ve[len(ve) // 10], ve[len(ve) // 2], len(vh)))
    for n in ("aspp.a.0.weight", "aspp.b.0.weight", "aspp.c.0.weight", "aspp.d.0.weight", "aspp.e.0.weight"):
        print("  %s: hip %.4f emu %.4f" % (n, _cos(gh[n], gr[n]), _cos(ge[n], gr[n])))
    assert all(torch.isfinite(g).all() for g in gh.values())
    assert vh[len(vh) // 2] >= ve[len(ve) // 2] - 0.10 and vh[len(vh) // 10] >= ve[len(ve) // 10] - 0.15
    for n, r in gr.items():
        if float(r.norm()) > 1e-10:
            ce, ch = _cos(ge[n], r), _cos(gh[n], r)
            assert not (ce >= 0.5 and ch < 0.5 * ce), (n, ch, ce)


def test_deepv3_dpc_captured_steps_match_eager(net_setup):
    """Two updates on two different inputs through semseg_amd.graph_training (the second a replay of the captured
    hipGraph with new data) against two eager updates from the same state: the bounds of
    tests/test_deeper_gpu.py::test_mscale_deeper_w38_captured_step_matches_eager.  1 x 384 x 416."""
    import semseg_amd
    from semseg_amd.loss.optimizer import FusedSGD
    gold, sd, images, gts = net_setup
    batches = [{"images": images[i:i + 1].to(DEV), "gts": gts[i:i + 1].to(DEV)} for i in range(2)]

    def steps(graphed):
        net = _build(sd).to(DEV).train()
        optim = FusedSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
        run, opt = (semseg_amd.graph_training(net, optim) if graphed else (net, optim))
        losses = []
        for b in batches:
            opt.zero_grad()
            loss = run(b).mean()
            losses.append(loss.detach().clone())
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        if graphed:
            assert run._stepper.replays == 2 and not run._stepper.eager_only, "the steps were not captured"
        return [float(v) for v in losses], {n: p.detach().float().cpu() for n, p in net.named_parameters()}, \
            {n: b.detach().float().cpu() for n, b in net.named_buffers()}
    le, pe, be = steps(False)
    lg, pg, bg = steps(True)
    print("deepv3+dpc eager losses %s captured %s" % (le, lg))
    assert le[0] != le[1]
    for a, b in zip(le, lg):
        assert a == a and abs(a - b) <= 2e-3 * abs(a), (le, lg)
    init = {n: v.float() for n, v in sd.items()}
    for n in ("aspp.a.0.weight", "aspp.c.0.weight", "aspp.e.0.weight"):
        assert float((pe[n] - init[n]).abs().max()) > 0, n                 # the steps moved the cell's filters
    for n in pe:
        assert float((pe[n] - pg[n]).abs().max()) < 1e-3 * float(pe[n].abs().max()), n
    for n in be:
        assert torch.allclose(be[n], bg[n], rtol=1e-3, atol=1e-4), n


# ---- route against route
def _spacing(v):
    """Distance between neighbouring numbers of the storage format at |v| (float64; the smallest normal's below it)."""
    bits, emin = (7, -126) if ACT_DTYPE == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** emin)))
    return 2.0 ** (e - bits)


def test_square_dilation_against_the_existing_route():
    """1 x 48 x 52 x 256 -> 256, dilation (6, 6): ops.dil_conv_bn_act (csrc/conv_dil.hip) against ops.conv_bn_act (the
    route every square-dilated conv has, and keeps) on the same weights, forward, data gradient and weight gradient.
    The BatchNorm is an evaluation-mode identity (mean 0, variance 1, eps 0, gamma 1, beta 0, no ReLU), so that each
    route's result IS its conv's stored output and the incoming gradient reaches both convs unchanged.

    Bound, per element, as in test_conv5x5_through_ops_against_the_generic_route: both routes add the same K products
    of the same 16-bit operands in fp32, in different orders, and round the sum ONCE to the storage format: one spacing
    of the format at the larger result plus the distance of two fp32 sums, 8 sqrt(K) 2^-24 S (four standard deviations of
    a random walk of K roundings per route), S = the sum of |products| from the EXISTING route run on |operands|
    (x 1.01 for its own rounding).  The weight gradient is fp32 on both routes: the second term alone, K = pixels."""
    from semseg_amd import nn as snn, ops
    bk = ops.HipBackend()
    hb = bk.hb
    g = torch.Generator().manual_seed(91)
    Ci, Co, Hh, Ww, d = 256, 256, 48, 52, 6
    x0 = torch.randn((1, Hh, Ww, Ci), generator=g).to(ACT_DTYPE).to(DEV)
    w0 = (torch.randn((Co, Ci, 3, 3), generator=g) * (2.0 / (9 * Ci)) ** 0.5).to(ACT_DTYPE).float()
    dy = torch.randn((1, Hh, Ww, Co), generator=g).to(ACT_DTYPE).to(DEV)
    prev = ops._BACKEND
    ops._set_backend_for_tests(bk)
    res = {}
    try:
        for route in ("dil", "generic", "mag"):         # mag: |operands| on the existing route
            hb.clear_pack_cache()
            mag = route == "mag"
            cls = snn.DilConv2d if route == "dil" else snn.Conv2d
            conv = cls(Ci, Co, kernel_size=3, padding=d, dilation=d, bias=False).to(DEV)
            with torch.no_grad():
                conv.weight.copy_((w0.abs() if mag else w0).to(DEV))
            bn = snn.BatchNorm2d(Co, eps=0.0).to(DEV).eval()
            x = (x0.abs() if mag else x0).clone().requires_grad_(True)
            bk.begin_step(x.device)
            before = hb.lib().ssa_launch_count(0)
            if route == "dil":
                y = bk.dil_conv_bn_act(conv, bn, x, relu=False)
            else:
                y = bk.conv_bn_act(conv, bn, x, relu=False)
            bk.end_forward()
            y.backward(dy.abs() if mag else dy)
            torch.cuda.synchronize()
            assert hb.lib().ssa_launch_count(0) > before
            res[route] = (y.detach().double().cpu(), x.grad.double().cpu(), conv.weight.grad.double().cpu())
    finally:
        ops._set_backend_for_tests(prev)
        hb.clear_pack_cache()
    for i, (what, K, stored) in enumerate((("y", 9 * Ci, True), ("dx", 9 * Co, True), ("dw", Hh * Ww, False))):
        a, b, S = res["dil"][i], res["generic"][i], res["mag"][i] * 1.01
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        bound = 8.0 * K ** 0.5 * 2.0 ** -24 * S
        if stored:
            bound = bound + _spacing(torch.maximum(a.abs(), b.abs()))
        err = (a - b).abs()
        print("square dilation %s: %d of %d elements differ between the routes; largest difference / bound %.3f" % (
            what, int((err > 0).sum()), err.numel(), float((err / bound.clamp(min=1e-300)).max())))
        assert not bool((~(err <= bound)).any()), (what, int((~(err <= bound)).sum()))
