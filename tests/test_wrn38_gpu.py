"""DeepLabV3+ on the WiderResNet-38 trunk (scripts/train_cityscapes_deepv3.yml, --arch deepv3.DeepV3PlusW38) on the HIP
kernels against the oracle, on the golden inputs generated from the real reference: the scheme and the bounds of
tests/test_deepv3_gpu.py (the measured bf16 storage noise floor of tests/bf16_emu_backend.py bounds the HIP path op by
op), plus the fused pre-activation op against its composition on the device and a captured step against an eager one."""
import os

import pytest
import torch

from util import ACT_DTYPE, check_close, check_close_robust

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _shapes():
    out = []
    with open(os.path.join(G, "keys_wrn38.txt")) as f:
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
    cfg.MODEL.WRN38_CHECKPOINT = ""
    cfg.MODEL.BNFUNC = None
    net = get_model("deepv3.DeepV3PlusW38", 19, CrossEntropyLoss2d(ignore_index=255))
    net.load_state_dict(sd)
    for m in net.modules():             # the mask draws of two backends are not the same stream
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
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


@pytest.fixture(scope="module")
def setup():
    from oracle.model import seeded_state_dict
    gold = torch.load(os.path.join(G, "wrn38_golden.pt"), map_location="cpu", weights_only=False)
    sd = seeded_state_dict(_shapes(), seed=gold["seed"])
    n = 0
    for k in sd:        # near-identity residual blocks (test_deepv3_gpu's bn3 damping): the last BatchNorm of each block
        last = ("mod6." in k or "mod7." in k) and k.endswith("convs.bn3.0.weight") or \
            not ("mod6." in k or "mod7." in k) and k.endswith("convs.bn2.0.weight")
        if last:
            sd[k] = sd[k] * 0.2
            n += 1
    assert n == 17
    sd["aspp.img_conv.1.weight"] = sd["aspp.img_conv.1.weight"] * 0.05      # BatchNorm over B = 2 samples: see test_deepv3_gpu
    return gold, sd


def test_wrn38_eval_op_by_op(setup):
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


def test_wrn38_train_step(setup):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    gold, sd = setup
    images, gts = gold["images"], gold["gts"]
    lr, gr = _run(OracleBackend(), sd, images, gts, True)
    le, ge = _run(Bf16EmuBackend(), sd, images, gts, True)
    lh, gh = _run(ops.HipBackend(), sd, images, gts, True, device="cuda")
    print("wrn38 train loss hip %.6f emu %.6f oracle %.6f" % (lh, le, lr))
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


@pytest.mark.parametrize("shortcut", [True, False], ids=["dadd", "last-use"])
def test_add_bn_act_fused_against_composition(shortcut):
    """ops.add_bn_act on the device: the fused Function (ssa_add_bn_stats + ssa_bn_apply_train; ssa_bn_bwd_reduce +
    ssa_bn_bwd_apply_add) against BackendBase's composition of today's ops (sum_act, batch_norm_act) -- s bit for bit, z,
    the gradients of both operands and of gamma / beta, the running statistics.  `dadd`: s also feeds a shortcut, so a
    gradient arrives at it; `last-use`: it does not (the plain ssa_bn_bwd_apply).  Bounds: util.check_close's, one bf16
    rounding of the output plus accumulation-order noise (the composition rounds the gradient sum twice)."""
    from semseg_amd import ops
    from semseg_amd.nn import BatchNorm2d
    B = ops.HipBackend()
    g = torch.Generator().manual_seed(900)
    shape = (2, 19, 23, 72)
    a0 = (torch.randn(shape, generator=g) * 1.5).to(ACT_DTYPE).cuda()
    b0 = (torch.randn(shape, generator=g) + 0.3).to(ACT_DTYPE).cuda()
    wz = torch.randn(shape, generator=g).to(ACT_DTYPE).cuda()
    ws = torch.randn(shape, generator=g).to(ACT_DTYPE).cuda()
    gamma, beta = torch.rand(72, generator=g) + 0.5, torch.randn(72, generator=g) * 0.2
    prev = ops._BACKEND
    ops._set_backend_for_tests(B)
    res = {}
    calls = {}
    try:
        for mode in ("fused", "composed"):
            bn = BatchNorm2d(72).cuda().train()
            with torch.no_grad():
                bn.weight.copy_(gamma)
                bn.bias.copy_(beta)
            a, b = a0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            B.begin_step(a.device)
            before = B.hb.lib().ssa_launch_count(0)
            s, z = B.add_bn_act(a, b, bn) if mode == "fused" else ops.BackendBase.add_bn_act(B, a, b, bn)
            B.end_forward()
            # the loss is linear in z and s: its gradients are the weights
            torch.autograd.backward([z] + ([s] if shortcut else []), [wz] + ([ws] if shortcut else []))
            torch.cuda.synchronize()
            calls[mode] = B.hb.lib().ssa_launch_count(0) - before
            res[mode] = dict(s=s.detach().cpu(), z=z.detach().float().cpu(), da=a.grad.float().cpu(), db=b.grad.float().cpu(),
                             dg=bn.weight.grad.float().cpu(), dbeta=bn.bias.grad.float().cpu(),
                             rm=bn.running_mean.cpu(), rv=bn.running_var.cpu(), nbt=int(bn.num_batches_tracked))
    finally:
        ops._set_backend_for_tests(prev)
    f, c = res["fused"], res["composed"]
    assert torch.equal(f["s"], c["s"])
    assert f["nbt"] == c["nbt"] == 1
    check_close("add_bn_act z", f["z"], c["z"])
    check_close_robust("add_bn_act da", f["da"], c["da"])
    check_close_robust("add_bn_act db", f["db"], c["db"])
    check_close("add_bn_act dgamma", f["dg"], c["dg"], 2e-3, 2e-3)
    check_close("add_bn_act dbeta", f["dbeta"], c["dbeta"], 2e-3, 2e-3)
    check_close("add_bn_act running_mean", f["rm"], c["rm"], 1e-5, 1e-5)
    check_close("add_bn_act running_var", f["rv"], c["rv"], 1e-5, 1e-5)
    assert torch.equal(f["da"], f["db"])
    print("launches: fused %d, composed %d" % (calls["fused"], calls["composed"]))
    assert calls["fused"] < calls["composed"]


def test_wrn38_captured_step_matches_eager(setup):
    """The pattern of tests/test_graphed_step_gpu.py at 1 x 96 x 128: one update of DeepV3PlusW38 through
    semseg_amd.graph_training (a replayed hipGraph: the fused Functions take their buffers from the step's arenas) and one
    eager update from the same state give the same loss and the same parameters."""
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
    print("wrn38 eager loss %.6f captured %.6f" % (le, lg))
    assert abs(le - lg) <= 2e-3 * abs(le)
    init = {n: v.float() for n, v in sd.items()}
    assert max(float((pe[n] - init[n]).abs().max()) for n in pe) > 0        # the step moved the parameters
    for n in pe:        # (test_graphed_step_gpu's bound: what may differ is the order of the atomics inside the BatchNorm sums)
        assert float((pe[n] - pg[n]).abs().max()) < 1e-3 * float(pe[n].abs().max()), n
    for n in be:
        assert torch.allclose(be[n], bg[n], rtol=1e-3, atol=1e-4), n
