"""The Deeper (Panoptic-DeepLab style) decoders on the HIP kernels against the oracle, on the golden inputs generated from
the real reference: the scheme and the bounds of tests/test_x71_gpu.py unchanged (the measured storage noise floor of
tests/bf16_emu_backend.py bounds the HIP path op by op) -- evaluation op by op for deeper.DeeperX71, one training step
of mscale.DeeperW38 (two-scale loss), a captured step against an eager one for mscale.DeeperW38 -- plus the 5x5 conv and
its data gradient through `ops` on csrc/conv_halo5.hip against the implicit-GEMM route at a size the policy sends to the
new kernel, and a captured step of deeper.DeeperX71 at 1 x 512 x 512, where both 5x5 convs run on it inside the network
(the golden batch, 2 x 96 x 128, keeps them below the policy: there the networks run them on the generic route)."""
import os

import pytest
import torch

from util import ACT_DTYPE

pytestmark = pytest.mark.gpu

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEMS = {"deeper.DeeperX71": "deeper_x71", "mscale.DeeperW38": "mscale_deeper_w38"}


def _shapes(arch):
    out = []
    with open(os.path.join(G, "keys_%s.txt" % STEMS[arch])) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _build(arch, sd):
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    cfg.MODEL.X71_CHECKPOINT = ""
    cfg.MODEL.WRN38_CHECKPOINT = ""
    cfg.MODEL.BNFUNC = None
    cfg.MODEL.N_SCALES = None
    net = get_model(arch, 19, CrossEntropyLoss2d(ignore_index=255))
    net.load_state_dict(sd)
    for m in net.modules():             # the mask draws of two backends are not the same stream
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0
    return net


def _run(arch, backend, sd, images, gts, train, device="cpu"):
    from semseg_amd import ops
    prev = ops._BACKEND
    ops._set_backend_for_tests(backend)
    try:
        net = _build(arch, sd).to(device).train(train)
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


def _setup(arch):
    """Golden inputs and the seeded state with test_x71_gpu's / test_wrn38_gpu's damping: the last BatchNorm of each residual
    block x 0.2 (near-identity blocks), the image-pooling BatchNorm (over B = 2 samples) x 0.05."""
    from oracle.model import seeded_state_dict
    gold = torch.load(os.path.join(G, "%s_golden.pt" % STEMS[arch]), map_location="cpu", weights_only=False)
    gold["gts"] = gold["gts"].long()
    sd = seeded_state_dict(_shapes(arch), seed=gold["seed"])
    n = 0
    if arch == "deeper.DeeperX71":
        from semseg_amd.network.xception import Block, xception71
        trunk = xception71(pretrained=False)
        for name, m in trunk.named_children():
            if isinstance(m, Block):
                k = "trunk.%s.rep.%d.weight" % (name, len(m.rep) - 1)
                sd[k] = sd[k] * 0.2
                n += 1
        assert n == 20
    else:
        for k in sd:
            deep = "mod6." in k or "mod7." in k
            if k.startswith("backbone.") and (deep and k.endswith("convs.bn3.0.weight") or not deep and k.endswith("convs.bn2.0.weight")):
                sd[k] = sd[k] * 0.2
                n += 1
        assert n == 17
    sd["aspp.img_conv.1.weight"] = sd["aspp.img_conv.1.weight"] * 0.05
    return gold, sd


@pytest.fixture(scope="module")
def setup_x71():
    return _setup("deeper.DeeperX71")


@pytest.fixture(scope="module")
def setup_w38():
    from semseg_amd.config import cfg
    before = cfg.LOSS.SUPERVISED_MSCALE_WT
    cfg.LOSS.SUPERVISED_MSCALE_WT = 0.05
    yield _setup("mscale.DeeperW38")
    cfg.LOSS.SUPERVISED_MSCALE_WT = before


def test_deeper_x71_eval_op_by_op(setup_x71):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend, traced
    arch = "deeper.DeeperX71"
    gold, sd = setup_x71
    images, gts = gold["images"], gold["gts"]
    prev = ops._BACKEND
    ops._set_backend_for_tests(OracleBackend())
    try:                                # calibrate the running statistics on this batch
        cal = _build(arch, sd).train()
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
    ref = _run(arch, traced(OracleBackend(), lambda i, n, y: (ref_log.append(y.detach()), names.append(n))), sd, images,
               gts, False)
    emu = _run(arch, traced(Bf16EmuBackend(), lambda i, n, y: emu_err.append(_rel(y.detach(), ref_log[i]))), sd, images,
               gts, False)
    hip = _run(arch, traced(ops.HipBackend(), lambda i, n, y: hip_err.append(_rel(y.detach().float().cpu(), ref_log[i]))),
               sd, images, gts, False, device="cuda")
    assert len(ref_log) == len(emu_err) == len(hip_err) > 80
    bad = [(i, names[i], tuple(ref_log[i].shape), hip_err[i], emu_err[i]) for i in range(len(hip_err))
           if not hip_err[i] <= 1.5 * emu_err[i] + 5e-3]
    worst = max(range(len(hip_err)), key=lambda i: hip_err[i] - 1.5 * emu_err[i])
    print("ops traced %d; largest excess at op %d (%s): hip %.4f emu %.4f; pred rel err hip %.4f emu %.4f" % (
        len(hip_err), worst, names[worst], hip_err[worst], emu_err[worst], _rel(hip, ref), _rel(emu, ref)))
    assert not bad, bad[:5]
    assert tuple(hip.shape) == (2, 19, 96, 128)
    assert torch.isfinite(hip).all() and _rel(hip, ref) <= 1.5 * _rel(emu, ref) + 5e-3
    ah = (hip.argmax(1) == ref.argmax(1)).float().mean().item()
    ae = (emu.argmax(1) == ref.argmax(1)).float().mean().item()
    print("argmax agreement with the oracle: hip %.4f emu %.4f" % (ah, ae))
    assert ah >= ae - 0.02


def test_mscale_deeper_w38_train_step(setup_w38):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    arch = "mscale.DeeperW38"
    gold, sd = setup_w38
    images, gts = gold["images"], gold["gts"]
    lr, gr = _run(arch, OracleBackend(), sd, images, gts, True)
    le, ge = _run(arch, Bf16EmuBackend(), sd, images, gts, True)
    lh, gh = _run(arch, ops.HipBackend(), sd, images, gts, True, device="cuda")
    print("mscale.DeeperW38 train loss hip %.6f emu %.6f oracle %.6f" % (lh, le, lr))
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


def test_mscale_deeper_w38_captured_step_matches_eager(setup_w38):
    """The pattern of tests/test_graphed_step_gpu.py at 1 x 96 x 128: one update of mscale.DeeperW38 through
    semseg_amd.graph_training (a replayed hipGraph) and one eager update from the same state give the same loss and the
    same parameters."""
    import semseg_amd
    from semseg_amd.loss.optimizer import FusedSGD
    arch = "mscale.DeeperW38"
    gold, sd = setup_w38
    batch = {"images": gold["images"][:1].cuda(), "gts": gold["gts"][:1].cuda()}

    def one_step(graphed):
        net = _build(arch, sd).cuda().train()
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
    print("mscale.DeeperW38 eager loss %.6f captured %.6f" % (le, lg))
    assert abs(le - lg) <= 2e-3 * abs(le)
    init = {n: v.float() for n, v in sd.items()}
    assert max(float((pe[n] - init[n]).abs().max()) for n in pe) > 0        # the step moved the parameters
    for n in pe:        # (test_graphed_step_gpu's bound: what may differ is the order of the atomics inside the BatchNorm sums)
        assert float((pe[n] - pg[n]).abs().max()) < 1e-3 * float(pe[n].abs().max()), n
    for n in be:
        assert torch.allclose(be[n], bg[n], rtol=1e-3, atol=1e-4), n


def test_deeper_x71_captured_step_above_the_policy_threshold(monkeypatch):
    """deeper.DeeperX71 at 1 x 512 x 512: conv_up2 at 128 x 128 and conv_up3 at 256 x 256, so both 5x5 convs and both data
    gradients run on ssa_conv2d_halo5 INSIDE the network -- its BatchNorm sums go to the training apply, and the launches
    are part of the replayed graph.  One captured update against one eager update from the same state, the bounds of the
    test above; the policy's answers are recorded to show the route was taken."""
    import semseg_amd
    from semseg_amd import hip_backend as hb
    from semseg_amd.loss.optimizer import FusedSGD
    from oracle.model import seeded_state_dict
    arch = "deeper.DeeperX71"
    sd = seeded_state_dict(_shapes(arch), seed=5)
    g = torch.Generator().manual_seed(31)
    gts = torch.randint(0, 19, (1, 16, 16), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)
    batch = {"images": torch.randn(1, 3, 512, 512, generator=g).cuda(), "gts": gts.cuda()}
    real = hb.halo5_supported
    answers = []
    monkeypatch.setattr(hb, "halo5_supported", lambda d: (answers.append((d.Cin, d.Cout, d.H, bool(real(d)))), answers[-1][3])[1])

    def one_step(graphed):
        net = _build(arch, sd).cuda().train()
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
    assert sorted(answers) == [(256, 288, 256, True), (256, 320, 128, True), (288, 256, 256, True), (320, 256, 128, True)]
    lg, pg, bg = one_step(True)
    assert answers and all(a[3] for a in answers)
    print("deeper.DeeperX71 at 512 x 512: eager loss %.6f captured %.6f" % (le, lg))
    assert le == le and abs(le - lg) <= 2e-3 * abs(le)
    init = {n: v.float() for n, v in sd.items()}
    assert float((pe["conv_up3.conv.weight"] - init["conv_up3.conv.weight"]).abs().max()) > 0
    assert float((pe["conv_up2.conv.weight"] - init["conv_up2.conv.weight"]).abs().max()) > 0
    for n in pe:
        assert float((pe[n] - pg[n]).abs().max()) < 1e-3 * float(pe[n].abs().max()), n
    for n in be:
        assert torch.allclose(be[n], bg[n], rtol=1e-3, atol=1e-4), n


def _spacing(v):
    """Distance between neighbouring numbers of the storage format at |v| (float64; the smallest normal's below it)."""
    bits, emin = (7, -126) if ACT_DTYPE == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(v.abs().clamp(min=2.0 ** emin)))
    return 2.0 ** (e - bits)


def test_conv5x5_through_ops_against_the_generic_route(monkeypatch):
    """1 x 128 x 128 x 320 -> 256 (conv_up2's channels at exactly the policy's 16384 pixels): ops.conv2d and its backward
    with the library's policy (forward and data gradient on ssa_conv2d_halo5) against the same calls with the policy
    answering no (ssa_conv2d_igemm, what the parent commit ran).

    Bound, per element: both routes add the same K = 25 * Cin (forward) or 25 * Cout (gradient) products of the same 16-bit
    operands in fp32, in different orders, and round the sum ONCE to the storage format.  So the two stored results differ
    by at most one spacing of the storage format at the larger of them, plus the distance of the two fp32 sums.  That
    distance is rounding noise: each of the K additions of a route rounds a partial sum no larger than S = sum of the
    |products| by at most 2^-24 of it, the errors are of either sign and add like a random walk, sqrt(K) 2^-24 S per route
    at one standard deviation; allowed are four of them per route, 8 sqrt(K) 2^-24 S -- at this shape (K = 8000, S about 80)
    3.4e-3, under half a bf16 spacing at |y| = 1, where a missing k-step of one tap (16 of the 8000 terms) moves y by
    about 0.06.  S comes from the GENERIC route run on |x| and |w| (its 16-bit rounding covered by the factor 1.01), never
    from the kernel under test."""
    from semseg_amd import ops
    B = ops.HipBackend()
    hb = B.hb
    g = torch.Generator().manual_seed(77)
    Cin, Cout, H, W = 320, 256, 128, 128
    x0 = torch.randn((1, H, W, Cin), generator=g).to(ACT_DTYPE).cuda()
    w0 = (torch.randn((Cout, Cin, 5, 5), generator=g) * (2.0 / (25 * Cin)) ** 0.5).to(ACT_DTYPE).float()
    dy = torch.randn((1, H, W, Cout), generator=g).to(ACT_DTYPE).cuda()
    real = hb.halo5_supported
    answers = []
    prev = ops._BACKEND
    ops._set_backend_for_tests(B)
    res = {}
    try:
        for route in ("halo5", "generic", "mag"):       # mag: |operands| on the generic route
            hb.clear_pack_cache()
            del answers[:]
            if route != "halo5":
                monkeypatch.setattr(hb, "halo5_supported", lambda d: (answers.append(False), False)[1])
            else:
                monkeypatch.setattr(hb, "halo5_supported", lambda d: (answers.append(real(d)), answers[-1])[1])
            mag = route == "mag"
            w = torch.nn.Parameter((w0.abs() if mag else w0).cuda())
            x = (x0.abs() if mag else x0).clone().requires_grad_(True)
            B.begin_step(x.device)
            before = hb.lib().ssa_launch_count(0)
            y = B.conv2d(x, w, None, 1, 2, 1, False)
            B.end_forward()
            y.backward(dy.abs() if mag else dy)
            torch.cuda.synchronize()
            assert len(answers) == 2 and all(a == (route == "halo5") for a in answers), (route, answers)
            assert hb.lib().ssa_launch_count(0) > before
            res[route] = (y.detach().double().cpu(), x.grad.double().cpu(), w.grad.double().cpu())
    finally:
        ops._set_backend_for_tests(prev)
        hb.clear_pack_cache()
    for i, (what, K) in enumerate((("y", 25 * Cin), ("dx", 25 * Cout))):
        a, b, S = res["halo5"][i], res["generic"][i], res["mag"][i] * 1.01
        assert bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
        bound = _spacing(torch.maximum(a.abs(), b.abs())) + 8.0 * K ** 0.5 * 2.0 ** -24 * S
        err = (a - b).abs()
        n_diff = int((err > 0).sum())
        print("conv5x5 %s: %d of %d elements differ between the routes; largest |difference| / spacing %.3f; largest "
              "difference / bound %.3f; largest difference where the results are below 2^-6: %.3g (noise allowed there %.3g)" % (
                  what, n_diff, err.numel(), float((err / _spacing(torch.maximum(a.abs(), b.abs()))).max()),
                  float((err / bound).max()), float(err[torch.maximum(a.abs(), b.abs()) < 2.0 ** -6].max()),
                  float(8.0 * K ** 0.5 * 2.0 ** -24 * S.max())))
        assert not bool((~(err <= bound)).any()), (what, int((~(err <= bound)).sum()))
    # (the weight gradient is the generic kernel's on both routes)
    assert bool(torch.isfinite(res["halo5"][2]).all()) and float(res["halo5"][2].abs().max()) > 0
