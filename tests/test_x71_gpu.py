"""DeepLabV3+ on the Xception-71 trunk (--arch deepv3.DeepV3PlusX71) on the HIP kernels against the oracle, on the golden
inputs generated from the real reference: the scheme and the bounds of tests/test_wrn38_gpu.py unchanged (the measured
bf16 storage noise floor of tests/bf16_emu_backend.py bounds the HIP path op by op), plus the separable-conv op against
its composition on the device, the inference epilogue against the two launches, and a captured step against an eager one."""
import os

import pytest
import torch

from util import ACT_DTYPE, check_close, check_close_robust

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _shapes():
    out = []
    with open(os.path.join(G, "keys_x71.txt")) as f:
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
    cfg.MODEL.X71_CHECKPOINT = ""
    cfg.MODEL.BNFUNC = None
    net = get_model("deepv3.DeepV3PlusX71", 19, CrossEntropyLoss2d(ignore_index=255))
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


def _last_norms():
    """State-dict keys of the last BatchNorm weight of each block's `rep` (the one the skip is added behind)."""
    from semseg_amd.network.xception import Block, xception71
    trunk = xception71(pretrained=False)
    return ["backbone.%s.rep.%d.weight" % (name, len(m.rep) - 1) for name, m in trunk.named_children() if isinstance(m, Block)]


@pytest.fixture(scope="module")
def setup():
    from oracle.model import seeded_state_dict
    gold = torch.load(os.path.join(G, "x71_golden.pt"), map_location="cpu", weights_only=False)
    gold["gts"] = gold["gts"].long()
    sd = seeded_state_dict(_shapes(), seed=gold["seed"])
    n = 0
    for k in _last_norms():             # near-identity residual blocks (test_wrn38_gpu's damping): the last BatchNorm of each block
        sd[k] = sd[k] * 0.2
        n += 1
    assert n == 20
    sd["aspp.img_conv.1.weight"] = sd["aspp.img_conv.1.weight"] * 0.05      # BatchNorm over B = 2 samples: see test_deepv3_gpu
    return gold, sd


def test_x71_eval_op_by_op(setup):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend, traced
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


def test_x71_train_step(setup):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    gold, sd = setup
    images, gts = gold["images"], gold["gts"]
    lr, gr = _run(OracleBackend(), sd, images, gts, True)
    le, ge = _run(Bf16EmuBackend(), sd, images, gts, True)
    lh, gh = _run(ops.HipBackend(), sd, images, gts, True, device="cuda")
    print("x71 train loss hip %.6f emu %.6f oracle %.6f" % (lh, le, lr))
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


def _sep_pair(C, Cout, stride, dil, g):
    from semseg_amd.nn import BatchNorm2d
    from semseg_amd.network.xception import SeparableConv2d
    sep, bn = SeparableConv2d(C, Cout, 3, stride, dil).cuda(), BatchNorm2d(Cout).cuda()
    with torch.no_grad():
        # representable in the storage format: the dense conv kernels round their filter to 16 bits when they pack it, the
        # depthwise kernels read the fp32 parameter -- with such a filter the two forms compute the same function (with an
        # arbitrary fp32 filter the outputs differ by a rounding almost everywhere, about 0.1 % of the ReLU masks fall on the
        # other side, and behind the 1x1 conv and the 3x3 stencil each of those moves 72 x 9 elements of dx: measured 4.4 %
        # of the elements past check_close_robust's bound, BOTH forms equally far, 1.4 %, from a float64 computation)
        sep.conv1.weight.copy_((torch.randn(C, 1, 3, 3, generator=g) * 0.4).to(ACT_DTYPE).float())
        sep.pointwise.weight.copy_(torch.randn(Cout, C, 1, 1, generator=g) * (2.0 / C) ** 0.5)
        for m in (sep.bn, bn):
            m.weight.copy_(torch.rand(m.num_features, generator=g) + 0.5)
            m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.2)
    return sep, bn


@pytest.mark.parametrize("stride,dil", [(1, 2), (2, 1)], ids=["s1d2", "s2"])
def test_separable_conv_bn_act_fused_against_composition(stride, dil):
    """ops.separable_conv_bn_act on the device: the depthwise kernels (statistics in the epilogue, one backward pass for dx
    and dW) against BackendBase's composition on the same device (the depthwise weight on the diagonal of a dense filter
    through the dense conv kernels, ssa_bn_stats) -- z, dx, the weight gradients of both convs, the running statistics of
    both BatchNorms.  Bounds: util.check_close's, one bf16 rounding of the output plus accumulation-order noise."""
    from semseg_amd import ops
    B = ops.HipBackend()
    shape, Cout = (2, 19, 23, 72), 96
    C = shape[3]
    g = torch.Generator().manual_seed(910)
    x0 = (torch.randn(shape, generator=g) * 1.5).to(ACT_DTYPE).cuda()
    Ho, Wo = (shape[1] - 1) // stride + 1, (shape[2] - 1) // stride + 1
    r0 = torch.randn((2, Ho, Wo, Cout), generator=g).to(ACT_DTYPE).cuda()
    wz = torch.randn((2, Ho, Wo, Cout), generator=g).to(ACT_DTYPE).cuda()
    state = g.get_state()
    prev = ops._BACKEND
    ops._set_backend_for_tests(B)
    res, calls = {}, {}
    try:
        for mode in ("fused", "composed"):
            g.set_state(state)
            sep, bn = _sep_pair(C, Cout, stride, dil, g)
            sep.train()
            bn.train()
            x, r = x0.clone().requires_grad_(True), r0.clone().requires_grad_(True)
            B.begin_step(x.device)
            before = B.hb.lib().ssa_launch_count(0)
            if mode == "fused":
                z = B.separable_conv_bn_act(sep, bn, x, residual=r, relu=True)
            else:
                y = ops.BackendBase.depthwise_conv(B, x, sep.conv1.weight, stride, dil)
                z = B.conv_bn_act(sep.pointwise, bn, B.batch_norm_act(y, sep.bn), r, True)
            B.end_forward()
            z.backward(wz)
            torch.cuda.synchronize()
            calls[mode] = B.hb.lib().ssa_launch_count(0) - before
            res[mode] = dict(z=z.detach().float().cpu(), dx=x.grad.float().cpu(), dr=r.grad.float().cpu(),
                             dw=sep.conv1.weight.grad.float().cpu(), dpw=sep.pointwise.weight.grad.float().cpu(),
                             rm1=sep.bn.running_mean.cpu(), rv1=sep.bn.running_var.cpu(), rm2=bn.running_mean.cpu(),
                             rv2=bn.running_var.cpu(), nbt=(int(sep.bn.num_batches_tracked), int(bn.num_batches_tracked)))
    finally:
        ops._set_backend_for_tests(prev)
    f, c = res["fused"], res["composed"]
    assert f["nbt"] == c["nbt"] == (1, 1)
    assert tuple(f["dw"].shape) == (C, 1, 3, 3) and float(f["dw"].abs().max()) > 0
    check_close("separable z", f["z"], c["z"])
    check_close_robust("separable dx", f["dx"], c["dx"])
    check_close_robust("separable dresidual", f["dr"], c["dr"])
    check_close("separable depthwise dW", f["dw"], c["dw"])
    check_close("separable pointwise dW", f["dpw"], c["dpw"])
    for k in ("rm1", "rv1", "rm2", "rv2"):
        check_close("separable running statistics " + k, f[k], c[k], 1e-5, 1e-5)
    print("launches: fused %d, composed %d" % (calls["fused"], calls["composed"]))
    assert calls["fused"] < calls["composed"]


@pytest.mark.parametrize("stride,dil", [(1, 2), (2, 1)], ids=["s1d2", "s2"])
def test_separable_eval_epilogue_same_bits(stride, dil, monkeypatch):
    """eval(): the inner BatchNorm as the depthwise kernel's epilogue (SSA_FUSE_EVAL_BN on, the default) against the two
    launches (off): the same bits, from one launch instead of two."""
    from semseg_amd import ops
    B = ops.HipBackend()
    g = torch.Generator().manual_seed(911)
    x = (torch.randn((2, 19, 23, 72), generator=g) * 1.5).to(ACT_DTYPE).cuda()
    sep, bn = _sep_pair(72, 96, stride, dil, g)
    with torch.no_grad():
        for m in (sep.bn, bn):
            m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
            m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    sep.eval()
    bn.eval()
    prev = ops._BACKEND
    ops._set_backend_for_tests(B)
    out, calls = {}, {}
    try:
        for fuse in (True, False):
            monkeypatch.setattr(B.hb, "_FUSE_EVAL_BN", fuse)
            for warm in (False, True):          # the second forward finds the layers' coefficient tables registered
                B.begin_step(x.device)
                with torch.no_grad():
                    before = B.hb.lib().ssa_launch_count(0)
                    inner = B.depthwise_conv_bn(sep, x)
                    calls[fuse] = B.hb.lib().ssa_launch_count(0) - before
                    z = B.separable_conv_bn_act(sep, bn, x, relu=True)
                torch.cuda.synchronize()
            out[fuse] = (inner.cpu(), z.cpu())
    finally:
        ops._set_backend_for_tests(prev)
    assert float(out[True][0].float().abs().max()) > 0
    assert torch.equal(out[True][0].view(torch.int16), out[False][0].view(torch.int16))
    assert torch.equal(out[True][1].view(torch.int16), out[False][1].view(torch.int16))
    # depthwise conv -> inner BatchNorm: ONE launch with the epilogue (this is what proves that the epilogue form ran and
    # the two settings did not take the same path), conv + apply without
    print("launches of depthwise_conv_bn: epilogue %d, two passes %d" % (calls[True], calls[False]))
    assert calls[True] == 1 and calls[False] >= 2


def test_x71_captured_step_matches_eager(setup):
    """The pattern of tests/test_graphed_step_gpu.py at 1 x 96 x 128: one update of DeepV3PlusX71 through
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
    print("x71 eager loss %.6f captured %.6f" % (le, lg))
    assert abs(le - lg) <= 2e-3 * abs(le)
    init = {n: v.float() for n, v in sd.items()}
    assert max(float((pe[n] - init[n]).abs().max()) for n in pe) > 0        # the step moved the parameters
    for n in pe:        # (test_graphed_step_gpu's bound: what may differ is the order of the atomics inside the BatchNorm sums)
        assert float((pe[n] - pg[n]).abs().max()) < 1e-3 * float(pe[n].abs().max()), n
    for n in be:
        assert torch.allclose(be[n], bg[n], rtol=1e-3, atol=1e-4), n
