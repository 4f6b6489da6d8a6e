"""DeepLabV3+ on the SE-ResNeXt-50 trunk (--arch deepv3.DeepV3PlusSRNX50) on the HIP kernels against the oracle, on the
golden inputs generated from the real reference: the scheme and the bounds of tests/test_x71_gpu.py unchanged (the
measured bf16 storage noise floor of tests/bf16_emu_backend.py bounds the HIP path op by op), plus each fused op -- the
grouped conv kernels against their composition on the device, the SE gate against its fp32 formula on the device -- at two
or three shapes, and a captured step against an eager one."""
import os

import pytest
import torch

from util import ACT_DTYPE, check_close, check_close_robust

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _shapes():
    out = []
    with open(os.path.join(G, "keys_srnx50.txt")) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _build(sd):
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    cfg.MODEL.SRNX_CHECKPOINT = ""
    cfg.MODEL.BNFUNC = None
    net = get_model("deepv3.DeepV3PlusSRNX50", 19, CrossEntropyLoss2d(ignore_index=255))
    net.load_state_dict(sd)
    return net


def _run(backend, sd, images, gts, train, device="cpu"):
    from semseg_amd import ops
    prev = ops._BACKEND
    ops._set_backend_for_tests(backend)
    try:
        net = _build(sd).to(device).train(train)
        inputs = {"images": images.to(device), "gts": gts.to(device)}
        if not train:
            with torch.no_grad():
                return net(inputs)["pred"].float().cpu()
        loss = net(inputs)
        loss.backward()
        if device != "cpu":
            torch.cuda.synchronize()
        return float(loss.detach()), {n: p.grad.detach().float().cpu() for n, p in net.named_parameters()}
    finally:
        ops._set_backend_for_tests(prev)


# bf16_emu_backend.TRACED plus the operators of this trunk.  Only the OUTERMOST call reports: the CPU backends run the
# three as BackendBase's compositions on traced primitives, the HIP backend as single operators.
TRACED = ("image_to_nhwc", "conv2d", "conv_bn_act", "batch_norm_act", "sum_act", "bilinear", "max_pool3x3s2_ceil",
          "global_avg_pool", "grouped_conv_bn_act", "se_gate_add_act")


def traced(backend, sink):
    counter, depth = [0], [0]

    class Traced(type(backend)):
        pass

    def mk(name):
        f = getattr(type(backend), name)

        def g(self, *a, **k):
            depth[0] += 1
            try:
                y = f(self, *a, **k)
            finally:
                depth[0] -= 1
            if depth[0] == 0:
                for t in (y if isinstance(y, (list, tuple)) else (y,)):
                    sink(counter[0], name, t)
                    counter[0] += 1
            return y
        return g
    for name in TRACED:
        setattr(Traced, name, mk(name))
    backend.__class__ = Traced
    return backend


@pytest.fixture(scope="module")
def setup():
    from oracle.model import seeded_state_dict
    gold = torch.load(os.path.join(G, "srnx50_golden.pt"), map_location="cpu", weights_only=False)
    gold["gts"] = gold["gts"].long()
    sd = seeded_state_dict(_shapes(), seed=gold["seed"])
    n = 0
    for k in list(sd):                  # near-identity residual blocks (test_wrn38_gpu's damping): bn3 of each bottleneck
        if k.startswith("backbone.layer") and k.endswith(".bn3.weight"):
            sd[k] = sd[k] * 0.2
            n += 1
    assert n == 16
    sd["aspp.img_conv.1.weight"] = sd["aspp.img_conv.1.weight"] * 0.05      # BatchNorm over B = 2 samples: see test_deepv3_gpu
    return gold, sd


def test_srnx_eval_op_by_op(setup):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    gold, sd = setup
    images, gts = gold["images"], gold["gts"]
    prev = ops._BACKEND
    ops._set_backend_for_tests(OracleBackend())
    try:                                # calibrate the running statistics on this batch
        cal = _build(sd).train()
        for m in cal.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.momentum = 1.0
        with torch.no_grad():
            cal({"images": images, "gts": gts})
        sd = {k: v.clone() for k, v in cal.state_dict().items()}
        del cal
    finally:
        ops._set_backend_for_tests(prev)
    ref_log, emu_err, hip_err, names = [], [], [], []
    ref = _run(traced(OracleBackend(), lambda i, n, y: (ref_log.append(y.detach()), names.append(n))), sd, images,
               gts, False)
    emu = _run(traced(Bf16EmuBackend(), lambda i, n, y: emu_err.append(_rel(y.detach(), ref_log[i]))), sd, images,
               gts, False)
    hip = _run(traced(ops.HipBackend(), lambda i, n, y: hip_err.append(_rel(y.detach().float().cpu(), ref_log[i]))),
               sd, images, gts, False, device="cuda")
    assert len(ref_log) == len(emu_err) == len(hip_err) > 80
    assert names.count("se_gate_add_act") == 16 and names.count("grouped_conv_bn_act") == 16
    assert names.count("max_pool3x3s2_ceil") == 1
    bad = [(i, names[i], tuple(ref_log[i].shape), hip_err[i], emu_err[i]) for i in range(len(hip_err))
           if not hip_err[i] <= 1.5 * emu_err[i] + 5e-3]
    worst = max(range(len(hip_err)), key=lambda i: hip_err[i] - 1.5 * emu_err[i])
    print("ops traced %d; largest excess at op %d (%s): hip %.4f emu %.4f; pred rel err hip %.4f emu %.4f" % (
        len(hip_err), worst, names[worst], hip_err[worst], emu_err[worst], _rel(hip, ref), _rel(emu, ref)))
    assert not bad, bad[:5]
    assert torch.isfinite(hip).all() and _rel(hip, ref) <= 1.5 * _rel(emu, ref) + 5e-3
    ah = (hip.argmax(1) == ref.argmax(1)).float().mean().item()
    ae = (emu.argmax(1) == ref.argmax(1)).float().mean().item()
    print("argmax agreement with the oracle: hip %.4f emu %.4f" % (ah, ae))
    assert ah >= ae - 0.02


def test_srnx_train_step(setup):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    gold, sd = setup
    images, gts = gold["images"], gold["gts"]
    lr, gr = _run(OracleBackend(), sd, images, gts, True)
    le, ge = _run(Bf16EmuBackend(), sd, images, gts, True)
    lh, gh = _run(ops.HipBackend(), sd, images, gts, True, device="cuda")
    print("srnx50 train loss hip %.6f emu %.6f oracle %.6f" % (lh, le, lr))
    assert abs(lh - lr) <= 2e-3 * abs(lr) + 2 * abs(le - lr)

    def cosines(g):
        return sorted(float((g[n] * r).sum() / (g[n].norm() * r.norm() + 1e-30)) for n, r in gr.items()
                      if float(r.norm()) > 1e-10)
    vh, ve = cosines(gh), cosines(ge)
    print("grad cosine vs oracle: hip min %.4f p10 %.4f median %.4f | emu min %.4f p10 %.4f median %.4f (n=%d)" % (
        vh[0], vh[len(vh) // 10], vh[len(vh) // 2], ve[0], ve[len(ve) // 10], ve[len(ve) // 2], len(vh)))
    assert all(torch.isfinite(g).all() for g in gh.values())
    assert vh[len(vh) // 2] >= ve[len(ve) // 2] - 0.10 and vh[len(vh) // 10] >= ve[len(ve) // 10] - 0.15
    for n, r in gr.items():
        if float(r.norm()) > 1e-10:
            ce = float((ge[n] * r).sum() / (ge[n].norm() * r.norm() + 1e-30))
            ch = float((gh[n] * r).sum() / (gh[n].norm() * r.norm() + 1e-30))
            assert not (ce >= 0.5 and ch < 0.5 * ce), (n, ch, ce)


@pytest.mark.parametrize("shape,groups,stride,dil", [((2, 19, 23, 128), 32, 1, 1), ((2, 13, 17, 256), 32, 2, 1),
                                                     ((1, 11, 9, 1024), 32, 1, 4)], ids=["c128", "c256s2", "c1024d4"])
def test_grouped_conv_bn_act_fused_against_composition(shape, groups, stride, dil):
    """ops.grouped_conv_bn_act on the device: the grouped kernels (statistics in the epilogue) against BackendBase's
    composition on the same device (the weight on the block diagonal of a dense filter through the dense conv kernels) --
    z, dx, the weight gradient and the BatchNorm's gradients and running statistics.  The filter is representable in the
    storage format (both forms round it to 16 bits).  Bounds: util.check_close's."""
    from semseg_amd import ops
    from semseg_amd.nn import BatchNorm2d
    B = ops.HipBackend()
    C = shape[3]
    g = torch.Generator().manual_seed(920)
    x0 = (torch.randn(shape, generator=g) * 1.5).to(ACT_DTYPE).cuda()
    Ho, Wo = (shape[1] - 1) // stride + 1, (shape[2] - 1) // stride + 1
    wz = torch.randn((shape[0], Ho, Wo, C), generator=g).to(ACT_DTYPE).cuda()
    w0 = (torch.randn(C, C // groups, 3, 3, generator=g) * (2.0 / (9 * C // groups)) ** 0.5).to(ACT_DTYPE).float()
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.2
    prev = ops._BACKEND
    ops._set_backend_for_tests(B)
    res = {}
    try:
        for mode in ("fused", "composed"):
            conv = torch.nn.Conv2d(C, C, 3, stride, dil, dil, groups, bias=False).cuda()
            bn = BatchNorm2d(C).cuda().train()
            with torch.no_grad():
                conv.weight.copy_(w0)
                bn.weight.copy_(gamma)
                bn.bias.copy_(beta)
            x = x0.clone().requires_grad_(True)
            B.begin_step(x.device)
            if mode == "fused":
                assert B.hb.gconv_supported(x, conv.weight, stride, dil, groups)
                z = B.hb.GConv3x3Fn.apply(x, conv.weight, stride, dil, groups, True)
                z = B.batch_norm_act(z, bn, None, True)
            else:
                y = ops.BackendBase.grouped_conv(B, x, conv.weight, stride, dil, groups)
                z = B.batch_norm_act(y, bn, None, True)
            B.end_forward()
            z.backward(wz)
            torch.cuda.synchronize()
            res[mode] = dict(z=z.detach().float().cpu(), dx=x.grad.float().cpu(), dw=conv.weight.grad.float().cpu(),
                             dg=bn.weight.grad.float().cpu(), db=bn.bias.grad.float().cpu(), rm=bn.running_mean.cpu(),
                             rv=bn.running_var.cpu(), nbt=int(bn.num_batches_tracked))
    finally:
        ops._set_backend_for_tests(prev)
    f, c = res["fused"], res["composed"]
    assert f["nbt"] == c["nbt"] == 1
    assert tuple(f["dw"].shape) == (C, C // groups, 3, 3) and float(f["dw"].abs().max()) > 0
    check_close("grouped z", f["z"], c["z"])
    check_close_robust("grouped dx", f["dx"], c["dx"])
    check_close("grouped dW", f["dw"], c["dw"])
    check_close("grouped dgamma", f["dg"], c["dg"])
    check_close("grouped dbeta", f["db"], c["db"])
    check_close("grouped running mean", f["rm"], c["rm"], 1e-5, 1e-5)
    check_close("grouped running var", f["rv"], c["rv"], 1e-5, 1e-5)


@pytest.mark.parametrize("shape,relu", [((2, 19, 23, 256), True), ((1, 12, 16, 2048), True), ((2, 7, 9, 512), False)],
                         ids=["c256", "c2048", "c512-norelu"])
def test_se_gate_against_fp32_formula(shape, relu):
    """ops.se_gate_add_act on the device (ssa_se_*) against the gate's formula written out with torch's fp32 operators and
    autograd on the same device and the same 16-bit inputs -- z, dy, dresidual and the four parameter gradients.  NOT the
    composition of BackendBase.se_gate_add_act on HipBackend: that one stores the means, h and s in 16 bits, which the
    kernels (fp32 throughout) are not meant to reproduce; the fp32 formula is the tighter reference.  Bounds:
    util.check_close's (one rounding of the 16-bit outputs plus accumulation-order noise)."""
    from semseg_amd import ops
    from semseg_amd.network.seresnext import SEModule
    B = ops.HipBackend()
    C = shape[3]
    g = torch.Generator().manual_seed(930)
    y0 = (torch.randn(shape, generator=g) + 0.3).to(ACT_DTYPE).cuda()
    r0 = torch.randn(shape, generator=g).to(ACT_DTYPE).cuda()
    wz = torch.randn(shape, generator=g).to(ACT_DTYPE).cuda()
    torch.manual_seed(931)
    se = SEModule(C, 16).cuda()
    with torch.no_grad():
        se.fc2.weight.mul_(4.0)                         # gates spread over (0.2, 0.8) instead of huddling at 1/2
    prev = ops._BACKEND
    ops._set_backend_for_tests(B)
    try:
        y, r = y0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
        B.begin_step(y.device)
        z = B.se_gate_add_act(se, y, r, relu=relu)
        B.end_forward()
        z.backward(wz)
        torch.cuda.synchronize()
        got = [z.detach().float().cpu(), y.grad.float().cpu(), r.grad.float().cpu()] + [p.grad.float().cpu() for p in se.parameters()]
    finally:
        ops._set_backend_for_tests(prev)
    y2, r2 = y0.float().requires_grad_(True), r0.float().requires_grad_(True)
    p2 = [p.detach().clone().requires_grad_(True) for p in se.parameters()]
    mean = y2.mean(dim=(1, 2))
    h = torch.relu(mean @ p2[0][:, :, 0, 0].t() + p2[1])
    s = torch.sigmoid(h @ p2[2][:, :, 0, 0].t() + p2[3])
    z2 = s[:, None, None, :] * y2 + r2
    z2 = torch.relu(z2) if relu else z2
    z2.backward(wz.float())
    want = [z2.detach().cpu(), y2.grad.cpu(), r2.grad.cpu()] + [p.grad.cpu() for p in p2]
    print("gates in (%.3f, %.3f)" % (float(s.min()), float(s.max())))
    assert float(s.max() - s.min()) > 0.2
    names = ("z", "dy", "dresidual", "dfc1.weight", "dfc1.bias", "dfc2.weight", "dfc2.bias")
    for name, a, b in zip(names, got, want):
        assert tuple(a.shape) == tuple(b.shape), name
        (check_close_robust if name in ("dy", "dresidual") else check_close)("se " + name, a, b)


def test_srnx_captured_step_matches_eager(setup):
    """The pattern of tests/test_graphed_step_gpu.py at 1 x 96 x 128: one update of DeepV3PlusSRNX50 through
    semseg_amd.graph_training (a replayed hipGraph) and one eager update from the same state give the same loss and the
    same parameters."""
    import semseg_amd
    from semseg_amd.loss.optimizer import FusedSGD
    gold, sd = setup
    batch = {"images": gold["images"][:1].cuda(), "gts": gold["gts"][:1].cuda()}

    def one_step(graphed):
        net = _build(sd).cuda().train()
        optim = FusedSGD(net.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
        run, opt = (semseg_amd.graph_training(net, optim) if graphed else (net, optim))
        opt.zero_grad()
        loss = run(batch).mean()
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        if graphed:
            assert run._stepper.replays == 1 and not run._stepper.eager_only, "the step was not captured"
        return float(loss.detach()), {n: p.detach().float().cpu() for n, p in net.named_parameters()}, \
            {n: b.detach().float().cpu() for n, b in net.named_buffers()}
    le, pe, be = one_step(False)
    lg, pg, bg = one_step(True)
    print("srnx50 eager loss %.6f captured %.6f" % (le, lg))
    assert abs(le - lg) <= 2e-3 * abs(le)
    init = {n: v.float() for n, v in sd.items()}
    assert max(float((pe[n] - init[n]).abs().max()) for n in pe) > 0        # the step moved the parameters
    for n in pe:        # (test_graphed_step_gpu's bound: what may differ is the order of the atomics inside the BatchNorm sums)
        assert float((pe[n] - pg[n]).abs().max()) < 1e-3 * float(pe[n].abs().max()), n
    for n in be:
        assert torch.allclose(be[n], bg[n], rtol=1e-3, atol=1e-4), n
