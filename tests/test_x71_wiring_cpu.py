"""Module wiring of DeepLabV3+ on the Xception-71 trunk (semseg_amd.network.xception, deepv3.DeepV3PlusX71) checked on
CPU against golden vectors from the REAL reference (tests/golden/make_golden_x71.py), with the oracle's operators behind
the ops interface -- `depthwise_conv` / `separable_conv_bn_act` run as BackendBase's compositions there (the depthwise
weight on the diagonal of a dense filter)."""
import os

import pytest
import torch

from util import check_close

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DW_SET = {(64, 1, 1), (128, 1, 1), (128, 2, 1), (256, 1, 1), (728, 1, 1), (728, 2, 1), (728, 1, 2), (1024, 1, 1),
          (1024, 1, 4), (1536, 1, 4)}


@pytest.fixture()
def oracle_ops():
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    prev = ops._BACKEND
    ops._set_backend_for_tests(OracleBackend())
    yield
    ops._set_backend_for_tests(prev)


def _shapes():
    out = []
    with open(os.path.join(G, "keys_x71.txt")) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


@pytest.fixture(scope="module")
def gold():
    g = torch.load(os.path.join(G, "x71_golden.pt"), map_location="cpu", weights_only=False)
    g.update(torch.load(os.path.join(G, "x71_golden_calib.pt"), map_location="cpu", weights_only=False))
    g["gts"] = g["gts"].long()
    return g


@pytest.fixture(scope="module")
def seeded(gold):
    from oracle.model import seeded_state_dict
    return seeded_state_dict(_shapes(), seed=gold["seed"])


def _net(train, sd):
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    cfg.MODEL.X71_CHECKPOINT = ""
    net = get_model("deepv3.DeepV3PlusX71", 19, CrossEntropyLoss2d(ignore_index=255))
    net.load_state_dict(sd)
    assert not any(isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)) for m in net.modules())
    return net.train(train)


def test_x71_state_dict_is_the_references():
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    from semseg_amd.network.utils import get_trunk
    from semseg_amd.network.xception import SeparableConv2d
    net = get_model("deepv3.DeepV3PlusX71", 19, CrossEntropyLoss2d(ignore_index=255))
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == _shapes()
    keys = set(net.state_dict())
    assert len(keys) == 825
    for k in ("backbone.block1.rep.0.conv1.weight", "backbone.block1.rep.0.bn.weight", "backbone.block1.rep.0.pointwise.weight",
              "backbone.block1.rep.1.weight", "backbone.block1.skip.weight", "backbone.block1.skipbn.running_var",
              "backbone.block4.rep.1.conv1.weight", "backbone.block20.rep.8.bias", "backbone.conv3.conv1.weight"):
        assert k in keys, k
    assert sum(p.numel() for p in net.parameters()) == 54632240
    assert sum(p.numel() for p in net.backbone.parameters()) == 37798448
    trunk, s2, s4, high = get_trunk("xception71")
    assert (s2, s4, high) == (64, 128, 2048)
    seps = [m for m in net.modules() if isinstance(m, SeparableConv2d)]
    assert len(seps) == 62
    assert {(m.conv1.in_channels, m.conv1.stride[0], m.conv1.dilation[0]) for m in seps} == DW_SET
    with pytest.raises(ValueError, match="xception71"):
        get_trunk("resnet-101")
    with pytest.raises(AssertionError):
        get_trunk("xception71", output_stride=16)


@pytest.mark.parametrize("stride,dil", [(1, 1), (1, 4), (2, 1)])
def test_depthwise_composition_is_the_grouped_conv(oracle_ops, stride, dil):
    """BackendBase.depthwise_conv (the weight on the diagonal of a dense filter) against F.conv2d(groups = C), float64:
    forward, input gradient and weight gradient; the off-diagonal products are exact zeros, so only the summation order
    of 9 terms may differ."""
    from semseg_amd import ops
    C = 16
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 9, 11, C, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(C, 1, 3, 3, generator=g, dtype=torch.float64, requires_grad=True)
    y = ops.backend().depthwise_conv(x, w, stride, dil)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    gx, gw = torch.autograd.grad(y, (x, w), dy)
    x2, w2 = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
    y2 = torch.nn.functional.conv2d(x2.permute(0, 3, 1, 2), w2, None, stride, dil, dil, C).permute(0, 2, 3, 1)
    gx2, gw2 = torch.autograd.grad(y2, (x2, w2), dy)
    for name, a, b in (("y", y, y2), ("dx", gx, gx2), ("dw", gw, gw2)):
        assert tuple(a.shape) == tuple(b.shape), name
        err = float((a - b).detach().abs().max())
        assert err <= 1e-13 * max(1.0, float(b.detach().abs().max())), (name, err)


def test_x71_block_skip_sees_the_relu_input(oracle_ops):
    """The reference's in-place leading ReLU rewrites the block input: an identity block (4..19) computes
    rep'(relu(x)) + relu(x), not rep'(relu(x)) + x.  Checked on our Block against the layers of `rep` applied one by one
    with torch's own ops."""
    from semseg_amd.network.xception import Block
    F = torch.nn.functional
    torch.manual_seed(3)
    blk = Block(24, 24, reps=3, stride=1, dilation=2, start_with_relu=True, grow_first=True).double().eval()
    for m in blk.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.5)
            m.running_var.uniform_(0.5, 2.0)
            m.weight.data.normal_(1, 0.2)
            m.bias.data.normal_(0, 0.2)
    assert blk.skip is None and isinstance(blk.rep[0], torch.nn.ReLU) and len(blk.rep) == 9
    x = torch.randn(2, 7, 9, 24, dtype=torch.float64)
    assert float(x.min()) < -0.5
    with torch.no_grad():
        out = blk(x)

        def bn(m, t):
            return F.batch_norm(t, m.running_mean, m.running_var, m.weight, m.bias, False, 0.1, m.eps)
        r = torch.relu(x).permute(0, 3, 1, 2)
        t = r
        for i in (1, 4, 7):
            sep, norm = blk.rep[i], blk.rep[i + 1]
            t = torch.relu(t) if i > 1 else t
            t = F.conv2d(t, sep.conv1.weight, None, 1, 2, 2, 24)
            t = F.conv2d(bn(sep.bn, t), sep.pointwise.weight)
            t = bn(norm, t)
        want, wrong = (t + r).permute(0, 2, 3, 1), (t + x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
    assert float((out - want).abs().max()) < 1e-12
    assert float((out - wrong).abs().max()) > 0.5


def test_x71_train_step_and_eval(oracle_ops, gold, seeded):
    """Train loss to 1e-5 and eval logits to 2e-3 / 5e-3 of the reference's (test_deepv3_wiring's tolerances);
    num_batches_tracked == 1 after one step; running-statistics samples to rtol 1e-4 / atol 1e-5.

    Sampled gradients against the reference's, per parameter: the relative distance over the golden sample,
    |g[idx] - gold[idx]| / |gold[idx]|, and the relative difference of the gradient norms.  The bound is measured in the
    test (the WiderResNet-38 test's rule): the same two distances between this module's own fp32 and fp64 runs on
    OracleBackend, per parameter; 4x the largest is allowed (the reference sums in place and in another order, so its fp32
    noise is another draw of the same size).
    The 62 `<SeparableConv2d>.bn.bias` have NO gradient: a constant added in front of the pointwise conv is a constant per
    output channel, which the training-mode BatchNorm behind it removes.  Their fp64 gradients are ~1e-17 of the largest
    (asserted: exactly these 62 names fall below 1e-8 of it), so a relative distance is a ratio of two noises; for them the
    same rule is applied to the ABSOLUTE distances (floor = this module's fp32 noise on these parameters, 4x allowed).
    Measured (random weights, batch 2 x 96 x 128; the trunk's last 56 blocks normalise over 384 samples): over the 352
    parameters with a gradient the floor is 4.07e-2 on the samples and 4.5e-3 on the norms (bounds 1.63e-1 and 1.8e-2) and
    the reference's gradients lie within 3.46e-2 and 4.84e-3; over the 62 null gradients the absolute floor is 1.29e-6 /
    3.2e-6 (bounds 5.2e-6 / 1.28e-5) and the reference's lie within 2.32e-6 / 7.81e-7."""
    net = _net(True, seeded)
    loss = net({"images": gold["images"], "gts": gold["gts"]})
    loss.backward()
    print("x71 train loss %.7f, the reference's %.7f" % (float(loss.detach()), float(gold["train_loss"])))
    check_close("x71 train loss", loss.detach().view(1), gold["train_loss"].view(1), 1e-5, 1e-5)
    sd = net.state_dict()
    for k in ("backbone.bn1.num_batches_tracked", "backbone.block1.rep.0.bn.num_batches_tracked",
              "backbone.block12.rep.5.num_batches_tracked", "backbone.block20.skipbn.num_batches_tracked",
              "backbone.conv5.bn.num_batches_tracked", "aspp.features.0.1.num_batches_tracked"):
        assert int(sd[k]) == 1, k
    worst = max(float((sd[k].flatten()[:4] - v).abs().max()) for k, v in gold["running_sample"].items())
    print("x71 running statistics: largest absolute distance from the reference's samples %.3g" % worst)
    for k, v in gold["running_sample"].items():
        assert torch.allclose(sd[k].flatten()[:4], v, rtol=1e-4, atol=1e-5), k
    assert all(p.grad is not None for p in net.parameters())
    g32 = {n: p.grad.clone() for n, p in net.named_parameters()}
    assert set(g32) == set(gold["grads"])
    del net

    net = _net(True, seeded).double()
    loss64 = net({"images": gold["images"].double(), "gts": gold["gts"]})
    loss64.backward()
    g64 = {n: p.grad for n, p in net.named_parameters()}
    top = max(float(g.norm()) for g in g64.values())
    null = sorted(n for n, g in g64.items() if float(g.norm()) <= 1e-8 * top)
    assert null == sorted(n for n in g64 if n.endswith(".bn.bias")) and len(null) == 62, null[:4]
    floor = {False: [0.0, 0.0], True: [0.0, 0.0]}
    dist = {}
    for n, g in g64.items():
        idx, vals, norm = gold["grads"][n]
        z = n in null
        a32, a64 = g32[n].flatten()[idx].double(), g.flatten()[idx]
        n32, n64 = float(g32[n].double().norm()), float(g.norm())
        ds, dn = float((a32 - a64).norm()), abs(n32 - n64)
        rs, rn = float((a32 - vals.double()).norm()), abs(n32 - float(norm))
        if not z:       # relative to the value; a null gradient's distances stay absolute
            ds, dn, rs, rn = ds / float(a64.norm()), dn / n64, rs / float(vals.double().norm()), rn / float(norm)
        floor[z] = [max(floor[z][0], ds), max(floor[z][1], dn)]
        dist[n] = (z, rs, rn)
    for z, what in ((False, "relative"), (True, "null gradients, absolute")):
        print("x71 gradients (%s): fp32-vs-fp64 floor %.3g (samples) %.3g (norms); against the reference %.3g / %.3g over %d "
              "parameters" % (what, floor[z][0], floor[z][1], max(d[1] for d in dist.values() if d[0] == z),
                              max(d[2] for d in dist.values() if d[0] == z), sum(1 for d in dist.values() if d[0] == z)))
    for n, (z, rs, rn) in dist.items():
        assert rs <= 4 * floor[z][0], (n, rs, floor[z][0])
        assert rn <= 4 * floor[z][1], (n, rn, floor[z][1])
    del net

    net = _net(False, seeded)
    net.load_state_dict(gold["calib_buffers"], strict=False)
    with torch.no_grad():
        o = net({"images": gold["images"]})
    assert tuple(o["pred"].shape) == (2, 19, 96, 128)
    check_close("x71 eval pred", o["pred"][:, :, ::8, ::8], gold["eval_pred"], 2e-3, 5e-3)


def test_x71_checkpoint_round_trip(tmp_path):
    """cfg.MODEL.X71_CHECKPOINT: checkpoint['model_dict'] saved from a DataParallel wrapper -- `module.` stripped, laid
    over the current state dict, loaded with strict=False: a key the trunk does not have is ignored and a key the file
    lacks keeps its initial value.  The synthetic file holds one distinct scalar per key, expanded to the key's shape."""
    from semseg_amd.config import cfg
    from semseg_amd.network.xception import xception71
    assert cfg.MODEL.X71_CHECKPOINT == ""
    ref = xception71()                                      # default: random init, no file needed
    sd, vals = {}, {}
    for i, (k, v) in enumerate(ref.state_dict().items()):
        vals[k] = (i + 1) if v.dtype == torch.long else 0.25 + i / 1024.0
        sd["module." + k] = torch.full((1,) * v.dim(), vals[k], dtype=v.dtype).expand(v.shape)
    sd["module.last_linear.weight"] = torch.zeros(1, 1).expand(1000, 2048)
    missing = "block7.rep.4.pointwise.weight"
    del sd["module." + missing]
    path = str(tmp_path / "aligned_xception71.pth")
    torch.save({"model_dict": sd, "epoch": 0}, path)
    assert os.path.getsize(path) < 2 << 20
    cfg.MODEL.X71_CHECKPOINT = path
    try:
        net = xception71(pretrained=True)
        for k, v in net.state_dict().items():
            if k == missing:
                assert float(v.std()) > 0 and not bool((v == vals[k]).all())
            else:
                assert bool((v == vals[k]).all()), k
        untouched = xception71(pretrained=False)
        assert float(untouched.state_dict()["conv1.weight"].std()) > 0
    finally:
        cfg.MODEL.X71_CHECKPOINT = ""
