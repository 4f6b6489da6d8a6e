"""End-to-end parity on the GPU: the product network (semseg_amd.network.ocrnet
on the HIP kernels, bf16 storage / fp32 accumulate) against the oracle (CPU fp32
restatement pinned to the reference) on identical seeded weights and inputs.

Stated tolerance.  north_star asks for logits within 1e-3 relative; that is not
reachable with bf16 activations (one rounding = 2^-9 per stored tensor, ~450
stored tensors deep, and two BatchNorms of the OCR head amplify relative
perturbations 3-6x on any weights) -- nor by the reference's own apex-O1 fp16
path.  The tolerance used here is therefore RELATIVE TO THE bf16 STORAGE NOISE
FLOOR, which is measured, not guessed: tests/bf16_emu_backend.py runs the
oracle's fp32 CPU operators with every stored tensor rounded to bf16 (same
weights, same inputs).  With
    e_hip[i] = |hip_i - oracle_i| / |oracle_i|   (L2 over the tensor, op i of ~1400)
    e_emu[i] = |emu_i - oracle_i| / |oracle_i|
the tests assert
  * op by op (eval):  e_hip[i] <= 1.5 * e_emu[i] + 5e-3 for EVERY tensor the operator surface returns -- a
    wrong kernel at any of the network's real shapes shows up as a jump at its
    index that the emulation does not have;
  * outputs (eval):   same rule for pred / pred_05x / pred_10x / attn_05x, and
    argmax agreement with the oracle >= the emulation's agreement - 2 %;
  * train loss:       |loss - oracle| <= 2e-3 * |oracle| + 2 * |emu - oracle|;
  * gradients:        cosine(hip, oracle) per parameter; its distribution over the
    955 parameters must match the emulation's (median and 10th percentile no
    more than 0.05 lower; measured on MI355X: hip 0.839/0.790, emu 0.856/0.814),
    and no single parameter may collapse: wherever the emulation reaches 0.5,
    cosine(hip) >= 0.5 * cosine(emu) and the gradient norm is within
    [0.6, 1.6] of the oracle's (a wrong wgrad/dgrad kernel at some shape gives
    cosine ~ 0 or a wrong scale for exactly the parameters it touches; a
    per-parameter margin tighter than this is inside the run-to-run spread of
    the emulation itself);
  * BN running statistics: within 3e-2 relative.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _synth(B, H, W, seed, C=19, ign=255):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, H, W, generator=g)
    bs = 32
    blocks = torch.randint(0, C, (B, (H + bs - 1) // bs, (W + bs - 1) // bs), generator=g)
    gts = blocks.repeat_interleave(bs, 1).repeat_interleave(bs, 2)[:, :H, :W].clone()
    gts[torch.rand(B, H, W, generator=g) < 0.1] = ign
    return images, gts.long()


def parity_state_dict(shapes, seed=0):
    """seeded_state_dict with the last BN of every residual block scaled by 0.2
    (the 'zero-init-residual' regime trained ResNets live in): with gamma ~ 1
    on 100+ stacked residual blocks a random network is chaotic and nothing
    can be compared through it."""
    from oracle.model import seeded_state_dict
    sd = seeded_state_dict(shapes, seed=seed)
    for k in sd:
        if (k.endswith("bn2.weight") and "branches" in k) or (k.endswith("bn3.weight") and "layer1" in k):
            sd[k] = sd[k] * 0.2
    return sd


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-30))


def _run(backend, sd, images, gts, train, device="cpu", C=19, ign=255):
    from semseg_amd import ops
    from semseg_amd.config import cfg
    from semseg_amd.loss import RMILoss
    from semseg_amd.network import ocrnet
    prev = ops._BACKEND
    ops._set_backend_for_tests(backend)
    saved_nc = cfg.DATASET.NUM_CLASSES
    try:
        cfg.LOSS.SUPERVISED_MSCALE_WT = 0.05
        cfg.MODEL.N_SCALES = None
        cfg.MODEL.BNFUNC = None
        cfg.DATASET.NUM_CLASSES = C             # the OCR head's width (network/ocrnet.py reads it from the config)
        net = ocrnet.HRNet_Mscale(C, RMILoss(num_classes=C, ignore_index=ign))
        net.load_state_dict(sd)
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout2d):
                m.p = 0.0
        net = net.to(device).train(train)
        inputs = {"images": images.to(device), "gts": gts.to(device)}
        if not train:
            with torch.no_grad():
                out = net(inputs)
            return {k: v.float().cpu() for k, v in out.items()}
        # fp16 storage (tests/test_amp_fp16_gpu.py runs this file with SSA_ACT_DTYPE=fp16): backward on loss * S with
        # apex's initial scale, on the HIP path and in the storage emulation alike; gradients compared un-scaled
        from util import ACT_DTYPE
        S = 65536.0 if (ACT_DTYPE == torch.float16 and type(backend).__name__ != "OracleBackend") else 1.0
        if S != 1.0:
            print("loss scale %d (%s)" % (S, type(backend).__name__))
            if device != "cpu":
                from semseg_amd import hip_backend
                hip_backend.enable_fp16_training()      # (the scaler's un-scaling is done by hand below)
        loss = net(inputs)
        (loss * S).backward()
        if device != "cpu":
            torch.cuda.synchronize()
        grads = {n: p.grad.detach().float().cpu() / S for n, p in net.named_parameters() if p.grad is not None}
        stats = {k: v.detach().float().cpu() for k, v in net.state_dict().items() if "running_" in k}
        return float(loss.detach()), grads, stats
    finally:
        cfg.DATASET.NUM_CLASSES = saved_nc
        ops._set_backend_for_tests(prev)


@pytest.fixture(scope="module")
def setup():
    from semseg_amd.config import cfg
    from semseg_amd.loss import RMILoss
    from semseg_amd.network import ocrnet
    from oracle.model import Net
    cfg.LOSS.SUPERVISED_MSCALE_WT = 0.05
    cfg.MODEL.N_SCALES = None
    cfg.MODEL.BNFUNC = None
    net = ocrnet.HRNet_Mscale(19, RMILoss(num_classes=19, ignore_index=255))
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = parity_state_dict(shapes, seed=0)
    images, gts = _synth(2, 256, 256, seed=77)
    # calibrate BN running stats on this input (momentum 1.0, oracle, CPU)
    with torch.no_grad():
        Net(sd, 19, training=True, bn_momentum=1.0, criterion="ce").two_scale_forward(images, gts)
    return sd, images, gts


def test_eval_op_by_op(setup):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend, traced
    sd, images, gts = setup
    ref_log, emu_err, hip_err, names = [], [], [], []
    ref = _run(traced(OracleBackend(), lambda i, n, y: (ref_log.append(y.detach()), names.append(n))),
               sd, images, gts, False)
    emu = _run(traced(Bf16EmuBackend(), lambda i, n, y: emu_err.append(_rel(y.detach(), ref_log[i]))),
               sd, images, gts, False)
    hip = _run(traced(ops.HipBackend(), lambda i, n, y: hip_err.append(_rel(y.detach().float().cpu(), ref_log[i]))),
               sd, images, gts, False, device="cuda")
    assert len(ref_log) == len(emu_err) == len(hip_err) > 400        # tensors returned by the (grouped) public ops
    worst = max(range(len(hip_err)), key=lambda i: hip_err[i] - 1.5 * emu_err[i])
    print("ops traced %d; largest excess at op %d (%s %s): hip %.4f emu %.4f" % (
        len(hip_err), worst, names[worst], tuple(ref_log[worst].shape), hip_err[worst], emu_err[worst]))
    for i in range(0, len(hip_err), 100):
        print("  op %4d %-14s hip %.4f emu %.4f" % (i, names[i], hip_err[i], emu_err[i]))
    bad = [(i, names[i], tuple(ref_log[i].shape), hip_err[i], emu_err[i]) for i in range(len(hip_err))
           if not hip_err[i] <= 1.5 * emu_err[i] + 5e-3]
    assert not bad, bad[:5]
    for k in ("pred_05x", "pred_10x", "attn_05x", "pred"):
        eh, ee = _rel(hip[k], ref[k]), _rel(emu[k], ref[k])
        print("eval %-9s rel err hip %.4f emu %.4f" % (k, eh, ee))
        assert torch.isfinite(hip[k]).all()
        assert eh <= 1.5 * ee + 5e-3, k
    from util import ACT_DTYPE
    if ACT_DTYPE == torch.float16:
        # the reference's own storage format: an order of magnitude closer to the fp32 oracle than bf16 (~0.17)
        eh = _rel(hip["pred"], ref["pred"])
        print("fp16 storage: eval pred rel err %.4f (emulation %.4f)" % (eh, _rel(emu["pred"], ref["pred"])))
        assert eh <= 0.03, eh
    ah = (hip["pred"].argmax(1) == ref["pred"].argmax(1)).float().mean().item()
    ae = (emu["pred"].argmax(1) == ref["pred"].argmax(1)).float().mean().item()
    print("argmax agreement with the oracle: hip %.4f emu %.4f" % (ah, ae))
    assert ah >= ae - 0.02


def test_train_step(setup):
    _check_train_step(*setup)


@pytest.fixture(scope="module")
def setup65():
    """Mapillary's head: 65 classes, ignore label 65 (= C), B = 2 at test_train_step's 256 x 256 (at 128 x 128 the
    random network's gradient cosines are noisier than the margins of test_train_step's bounds, on both paths)."""
    from semseg_amd.config import cfg
    from semseg_amd.loss import RMILoss
    from semseg_amd.network import ocrnet
    from oracle.model import Net
    cfg.LOSS.SUPERVISED_MSCALE_WT = 0.05
    cfg.MODEL.N_SCALES = None
    cfg.MODEL.BNFUNC = None
    saved_nc = cfg.DATASET.NUM_CLASSES
    cfg.DATASET.NUM_CLASSES = 65
    try:
        net = ocrnet.HRNet_Mscale(65, RMILoss(num_classes=65, ignore_index=65))
    finally:
        cfg.DATASET.NUM_CLASSES = saved_nc
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    sd = parity_state_dict(shapes, seed=0)
    images, gts = _synth(2, 256, 256, seed=65, C=65, ign=65)
    with torch.no_grad():
        Net(sd, 65, training=True, bn_momentum=1.0, criterion="ce", ignore_index=65).two_scale_forward(images, gts)
    return sd, images, gts


def test_training_65_classes(setup65):
    """One HRNet_Mscale(65, RMILoss(num_classes=65, ignore_index=65)) training step against the oracle with
    test_train_step's assertions: the RMI pool in three class chunks and the 65-wide classifier convs' data and weight
    gradients (output channels padded to 72)."""
    sd, images, gts = setup65
    assert int((gts == 65).sum()) > 0
    _check_train_step(sd, images, gts, C=65, ign=65)


def _check_train_step(sd, images, gts, C=19, ign=255):
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    lr, gr, sr = _run(OracleBackend(), sd, images, gts, True, C=C, ign=ign)
    le, ge, se = _run(Bf16EmuBackend(), sd, images, gts, True, C=C, ign=ign)
    lh, gh, sh = _run(ops.HipBackend(), sd, images, gts, True, device="cuda", C=C, ign=ign)
    print("train loss hip %.6f emu %.6f oracle %.6f" % (lh, le, lr))
    assert abs(lh - lr) <= 2e-3 * abs(lr) + 2 * abs(le - lr)

    def cosines(g):
        out = {}
        for name, r in gr.items():
            if float(r.norm()) < 1e-10:
                continue
            assert torch.isfinite(g[name]).all(), name
            out[name] = float((g[name] * r).sum() / (g[name].norm() * r.norm() + 1e-30))
        return out
    ch, ce = cosines(gh), cosines(ge)
    vh, ve = sorted(ch.values()), sorted(ce.values())
    print("grad cosine vs oracle: hip min %.4f p10 %.4f median %.4f | emu min %.4f p10 %.4f median %.4f (n=%d)" % (
        vh[0], vh[len(vh) // 10], vh[len(vh) // 2], ve[0], ve[len(ve) // 10], ve[len(ve) // 2], len(vh)))
    nr = {k: float(gh[k].norm() / (gr[k].norm() + 1e-30)) for k in ch}
    bad = [(k, ch[k], ce[k], nr[k]) for k in ch
           if ce[k] >= 0.5 and (ch[k] < 0.5 * ce[k] or not 0.6 <= nr[k] <= 1.6)]
    for k in sorted(ch, key=lambda k: ch[k] - ce[k])[:6]:
        print("  largest deficit %-60s hip %.4f emu %.4f norm ratio %.3f" % (k, ch[k], ce[k], nr[k]))
    assert not bad, bad[:5]
    assert vh[len(vh) // 2] >= ve[len(ve) // 2] - 0.05
    assert vh[len(vh) // 10] >= ve[len(ve) // 10] - 0.05
    # running statistics: 3 % of the largest entry, or twice what bf16 STORAGE alone does to the same statistic (the
    # object-context BatchNorms see 2 x 19 region vectors per channel: their variance moves 2.3 % under the CPU bf16
    # emulation, 1.7-3.8 % on the device depending on the kernel versions -- the same statistic tops both lists)
    rel = {k: float((sh[k] - sr[k]).abs().max() / (sr[k].abs().max() + 1e-12)) for k in sr}
    rel_e = {k: float((se[k] - sr[k]).abs().max() / (sr[k].abs().max() + 1e-12)) for k in sr}
    top = sorted(rel.items(), key=lambda kv: -kv[1])[:5]
    print("running stats worst rel %.4g (emu %.4g); the five worst: %s" % (top[0][1], max(rel_e.values()), [(k, round(v, 4), round(rel_e[k], 4)) for k, v in top]))
    # (round 6: the bound on the largest entry sat INSIDE the range the comment above states -- 3 % against 1.7-3.8 % --,
    # and the first kernel change that moved a rounding anywhere upstream tripped it: f_up's variance 3.03 % with 1 ulp
    # different BatchNorm scales, identical with the new conv kernels switched on or off.  4.5 % clears the stated range;
    # a wrong statistic -- a miscounted pixel, a missed pass -- is off by 10 % or more.)
    over = [(k, v, rel_e[k]) for k, v in rel.items() if v > max(4.5e-2, 2.0 * rel_e[k])]
    assert not over, over[:5]


def test_eval_nscale(setup):
    """Hierarchical multi-scale inference {0.5, 1.0, 2.0} (network/ocrnet.py:185-262, BASELINE
    configs[2]); the three scale passes run on concurrent streams on the HIP path."""
    from semseg_amd import ops
    from semseg_amd.config import cfg
    from oracle_backend import OracleBackend
    from bf16_emu_backend import Bf16EmuBackend
    from semseg_amd.loss import RMILoss as _RMI
    from semseg_amd.network import ocrnet as _ocrnet
    from test_parity_eval_gpu import _image, calibrate_eval_bn
    sd, _, gts = setup
    # A photograph-like (1/f) image and BatchNorm buffers calibrated over exactly the three passes under test
    # (tests/test_parity_eval_gpu.py::calibrate_eval_bn): with white noise and the fixture's two-scale statistics the
    # three passes sit at different activation levels and the attention logits are ill-conditioned (round-4 review).
    images = _image(128, 192, 78)
    gts = gts[:1, :128, :192].contiguous()
    cfg.MODEL.N_SCALES = [0.5, 1.0, 2.0]
    try:
        cal = _ocrnet.HRNet_Mscale(19, _RMI(num_classes=19, ignore_index=255))
        cal.load_state_dict(sd)
        sd = {k: v.clone() for k, v in calibrate_eval_bn(cal, images, "cpu").state_dict().items()}
    finally:
        cfg.MODEL.N_SCALES = None

    def run(backend, device):
        from semseg_amd.loss import RMILoss
        from semseg_amd.network import ocrnet
        prev = ops._BACKEND
        ops._set_backend_for_tests(backend)
        try:
            cfg.MODEL.N_SCALES = [0.5, 1.0, 2.0]
            net = ocrnet.HRNet_Mscale(19, RMILoss(num_classes=19, ignore_index=255))
            net.load_state_dict(sd)
            net = net.to(device).eval()
            with torch.no_grad():
                o = net({"images": images.to(device), "gts": gts.to(device)})
            return {k: v.float().cpu() for k, v in o.items()}
        finally:
            cfg.MODEL.N_SCALES = None
            ops._set_backend_for_tests(prev)

    ref, emu, hip = run(OracleBackend(), "cpu"), run(Bf16EmuBackend(), "cpu"), run(ops.HipBackend(), "cuda")
    assert set(hip) == set(ref) and "pred_2.0x" in hip and "attn_0.5x" in hip
    # The outputs of this random-weight network carry the storage noise amplified ~100x (a 1e-6 perturbation of the image
    # moves `pred` by 1.3e-4, tests/test_parity_eval_gpu.py), so the error of ONE output is itself a random variable:
    # in two noisy runs (the CPU emulation and the device, which round the same tensors but sum in different orders) the
    # same output comes out 0.145 in one and 0.238 in the other while the NEXT output shows the reverse.  What is stable
    # is the level of a KIND of output (attention maps; predictions) and the level over all outputs, so those are bounded:
    #   * every output <= 1.5 x the largest emulation error among the outputs of its kind + 5e-3,
    #   * the mean over all outputs <= 1.25 x the emulation's mean + 5e-3
    # (a kernel that is wrong at some shape puts its outputs at O(1): both bounds fail by a wide margin; op-level
    # accuracy is the teacher-forced tests' job).  Same rule for both storage builds.
    ee_all = {k: _rel(emu[k], ref[k]) for k in ref}
    eh_all = {k: _rel(hip[k], ref[k]) for k in ref}
    kind = lambda k: "attn" if k.startswith("attn") else "pred"      # noqa: E731
    worst = {kd: max(v for k, v in ee_all.items() if kind(k) == kd) for kd in ("attn", "pred")}
    for k in sorted(ref):
        print("nscale %-10s rel err hip %.4f emu %.4f" % (k, eh_all[k], ee_all[k]))
        assert torch.isfinite(hip[k]).all() and hip[k].shape == ref[k].shape
    from util import ACT_DTYPE
    for k in sorted(ref):
        bound = 1.5 * worst[kind(k)] + 5e-3
        assert eh_all[k] <= bound, (k, eh_all[k], ee_all[k], bound)
        if ACT_DTYPE == torch.float16:
            # fp16 storage (the reference's own format) sits an order of magnitude closer to the oracle: at ~1e-2 the
            # amplified noise no longer decides an output's error, so EVERY output is held to its own emulation
            # error (the per-output bound of round 3, asked back by the round-5 review) and to an absolute level
            assert eh_all[k] <= 1.5 * ee_all[k] + 1e-2, (k, eh_all[k], ee_all[k])
            assert eh_all[k] <= 0.06, (k, eh_all[k])
    mh, me = sum(eh_all.values()) / len(eh_all), sum(ee_all.values()) / len(ee_all)
    print("nscale mean over the outputs: hip %.4f emu %.4f" % (mh, me))
    assert mh <= 1.25 * me + 5e-3, (mh, me)


def test_smoke_entry():
    """`__graft_entry__.smoke()` -- what the driver runs before the bench -- is part of the suite (advisor, round 5):
    one 2 x 3 x 128 x 256 training step on the HIP path against the oracle (loss 5e-3, classifier-gradient cosine 0.99)."""
    import importlib
    import os
    import sys
    from util import ACT_DTYPE
    if ACT_DTYPE == torch.float16:
        pytest.skip("smoke() is the default (bf16) build's entry; fp16 training goes through the loss scaler "
                    "(tests/test_amp_fp16_gpu.py)")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from semseg_amd.config import cfg
    saved = (cfg.LOSS.SUPERVISED_MSCALE_WT, cfg.MODEL.N_SCALES)
    try:
        importlib.import_module("__graft_entry__").smoke()
    finally:
        cfg.LOSS.SUPERVISED_MSCALE_WT, cfg.MODEL.N_SCALES = saved
