"""Module wiring of the Dense Prediction Cell (semseg_amd.network.deepv3.DPC / dpc_conv, get_aspp(dpc=True)) and of the heads
that take `use_dpc=True`, checked on CPU against golden vectors from the REAL reference
(tests/golden/make_golden_dpc.py): the float64 restatement tests/dpc_ref.py, the module on the oracle's operators behind
the ops interface (BackendBase.dil_conv_bn_act), the state-dict keys of DeepV3Plus(use_dpc=True).

Comparison rules are those of tests/test_deeper_wiring_cpu.py / tests/test_srnx_wiring_cpu.py: outputs by check_close at
2e-3 / 5e-3, running statistics at rtol 1e-4 / atol 1e-5, train loss at 1e-5, gradients per tensor by relative distance
and relative difference of the norms, bounded by 4x the largest such distance between the module's own fp32 and fp64 runs."""
import os

import pytest
import torch

from util import check_close
import dpc_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture()
def oracle_ops():
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    prev = ops._BACKEND
    ops._set_backend_for_tests(OracleBackend())
    yield
    ops._set_backend_for_tests(prev)


@pytest.fixture(scope="module")
def gold():
    g = torch.load(os.path.join(G, "dpc_golden.pt"), map_location="cpu", weights_only=False)
    g["calib"] = torch.load(os.path.join(G, "dpc_golden_calib.pt"), map_location="cpu", weights_only=False)
    return g


def _read_keys(name):
    out = []
    with open(os.path.join(G, "keys_%s.txt" % name)) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


def _seeded(stride, rec, dtype=torch.float64):
    from oracle.model import seeded_state_dict
    _, cin, red, _, _ = R.MODULE_CASES[stride]
    sd = seeded_state_dict(R.module_shapes(cin, red), seed=rec["seed"])
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _ref_train(stride, rec, swap_axes=False):
    sd = _seeded(stride, rec)
    for k, v in sd.items():
        if v.is_floating_point() and "running" not in k:
            v.requires_grad_(True)
    x, gy = R.module_inputs(stride)
    x.requires_grad_(True)
    out, stats = R.dpc(x, sd, stride, True, swap_axes)
    (out * gy).sum().backward()
    return out.detach(), x.grad, {k: v.grad for k, v in sd.items() if v.requires_grad}, stats


@pytest.mark.parametrize("stride", [16, 8])
def test_dpc_ref_reproduces_the_reference_module(gold, stride):
    """tests/dpc_ref.py (float64, tap by tap) against the real module: train output, input gradient, every parameter
    gradient, the running statistics after the pass, and the eval output on the calibrated buffers."""
    rec = gold["module"][stride]
    B, cin, red, H, W = R.MODULE_CASES[stride]
    R.assert_taps_inside(H, W, stride)
    assert tuple(rec["out"].shape) == (B, 5 * red, H, W)
    out, dx, grads, stats = _ref_train(stride, rec)
    check_close("dpc_ref os%d out" % stride, out, rec["out"], 2e-3, 5e-3)
    check_close("dpc_ref os%d dx" % stride, dx, rec["dx"], 2e-3, 5e-3)
    assert sorted(grads) == sorted(rec["grads"])
    for k, g in rec["grads"].items():
        check_close("dpc_ref os%d grad %s" % (stride, k), grads[k], g, 2e-3, 5e-3)
    assert sorted(stats) == sorted(rec["running"])
    for k, v in rec["running"].items():
        assert torch.allclose(stats[k].float(), v, rtol=1e-4, atol=1e-5), k
    sd = _seeded(stride, rec)
    sd.update({k: v.double() for k, v in rec["calib"].items()})
    with torch.no_grad():
        ev, none = R.dpc(R.module_inputs(stride)[0], sd, stride, False)
    assert not none
    check_close("dpc_ref os%d eval" % stride, ev[:, :, ::2, ::2], rec["eval_out"], 2e-3, 5e-3)


@pytest.mark.parametrize("stride", [16, 8])
def test_transposed_rate_pairs_do_not_reproduce_the_golden(gold, stride):
    """(dil_w, dil_h) in place of (dil_h, dil_w) in every conv of the cell misses the golden output by far more than the
    bound the true cell is held to: a transposed rate pair cannot pass."""
    rec = gold["module"][stride]
    out, _, _, _ = _ref_train(stride, rec, swap_axes=True)
    with pytest.raises(AssertionError):
        check_close("dpc_ref os%d out, axes swapped" % stride, out, rec["out"], 2e-3, 5e-3)
    err = (out - rec["out"].double()).abs()
    # not a near miss: beyond 100x the bound in the maximum, on the channels of every layer (the square-rate layer d
    # reads a, which differs)
    red = R.MODULE_CASES[stride][2]
    for i, n in enumerate(R.NAMES):
        worst = float(err[:, i * red:(i + 1) * red].max()) / float(rec["out"].abs().max())
        assert worst > 0.2, (n, worst)


def _cell(stride, rec, dtype):
    from semseg_amd.network.deepv3 import DPC
    _, cin, red, _, _ = R.MODULE_CASES[stride]
    cell = DPC(cin, red, output_stride=stride)
    assert [(k, tuple(v.shape)) for k, v in cell.state_dict().items()] == R.module_shapes(cin, red)
    cell.load_state_dict(_seeded(stride, rec, torch.float32))
    return cell.to(dtype)


def _cell_train(stride, rec, dtype):
    cell = _cell(stride, rec, dtype).train()
    x64, gy64 = R.module_inputs(stride)
    x = x64.to(dtype).requires_grad_(True)
    out = cell(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)           # the ops surface is NHWC
    (out * gy64.to(dtype)).sum().backward()
    grads = {n: p.grad for n, p in cell.named_parameters()}
    grads["<input>"] = x.grad
    return cell, out.detach(), grads


@pytest.mark.parametrize("stride", [16, 8])
def test_dpc_module_on_the_portable_backend(oracle_ops, gold, stride):
    """semseg_amd's DPC through BackendBase.dil_conv_bn_act (F.conv2d with the tuple padding / dilation) against the
    golden of the real module."""
    rec = gold["module"][stride]
    cell, out, g32 = _cell_train(stride, rec, torch.float32)
    check_close("DPC os%d out" % stride, out, rec["out"], 2e-3, 5e-3)
    sd = cell.state_dict()
    for n in R.NAMES:
        assert int(sd["%s.1.num_batches_tracked" % n]) == 1
    for k, v in rec["running"].items():
        assert torch.allclose(sd[k], v, rtol=1e-4, atol=1e-5), k
    _, _, g64 = _cell_train(stride, rec, torch.float64)
    want = dict(rec["grads"])
    want["<input>"] = rec["dx"]
    assert sorted(g32) == sorted(want)
    floor, dist = [0.0, 0.0], {}
    for n, g in g64.items():
        a32, ref = g32[n].double(), want[n].double()
        floor = [max(floor[0], float((a32 - g).norm() / g.norm())), max(floor[1], abs(float(a32.norm() - g.norm())) / float(g.norm()))]
        dist[n] = (float((a32 - ref).norm() / ref.norm()), abs(float(a32.norm() - ref.norm())) / float(ref.norm()))
    print("DPC os%d gradients: fp32-vs-fp64 floor %.3g (tensors) %.3g (norms); against the reference %.3g / %.3g over %d tensors"
          % (stride, floor[0], floor[1], max(d[0] for d in dist.values()), max(d[1] for d in dist.values()), len(dist)))
    for n, (rs, rn) in dist.items():
        assert rs <= 4 * floor[0], (n, rs, floor[0])
        assert rn <= 4 * floor[1], (n, rn, floor[1])
    ev = _cell(stride, rec, torch.float32)
    ev.load_state_dict(rec["calib"], strict=False)
    ev.eval()
    with torch.no_grad():
        o = ev(R.module_inputs(stride)[0].float().permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
    check_close("DPC os%d eval" % stride, o[:, :, ::2, ::2], rec["eval_out"], 2e-3, 5e-3)


def test_deepv3_dpc_state_dict_is_the_references():
    from semseg_amd.network.deepv3 import DPC, DeepV3Plus
    from semseg_amd import nn as snn
    net = DeepV3Plus(19, trunk="resnet-50", use_dpc=True)
    got = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    want = _read_keys("deepv3_dpc")
    assert len(got) == len(want) and got == want
    assert isinstance(net.aspp, DPC) and tuple(net.bot_aspp.weight.shape) == (256, 1280, 1, 1)
    rates = [tuple(getattr(net.aspp, n)[0].dilation) for n in R.NAMES]
    assert rates == [(2, 12), (36, 30), (12, 42), (2, 2), (12, 6)] == list(R.rates_for(8))
    for n in R.NAMES:
        conv, bn = getattr(net.aspp, n)[0], getattr(net.aspp, n)[1]
        assert isinstance(conv, snn.DilConv2d) and conv.padding == conv.dilation and conv.bias is None
        # the reference builds these with nn.BatchNorm2d, not Norm2d: local statistics even under --syncbn
        assert type(bn) is snn.BatchNorm2d and not bn.sync
    assert [n for n, _ in net.aspp.named_children()] == list(R.NAMES) + ["drop"]
    # without the flag nothing changed
    assert [k for k, _ in DeepV3Plus(19, trunk="resnet-50").state_dict().items()] == [k for k, _ in _read_keys("deepv3")]


def test_init_all_initialises_the_cell():
    """init_all=True: initialize_weights(self.aspp, ...) (network/deepv3.py:69-70) reaches the cell's convs (kaiming) and
    BatchNorms (1, 0), as network/mynn.py:27-39 does for any nn.Conv2d / nn.BatchNorm2d."""
    from semseg_amd.network.deepv3 import DeepV3Plus
    torch.manual_seed(0)
    net = DeepV3Plus(19, trunk="resnet-50", use_dpc=True, init_all=True)
    for n in R.NAMES:
        conv, bn = getattr(net.aspp, n)[0], getattr(net.aspp, n)[1]
        assert bool((bn.weight == 1).all()) and bool((bn.bias == 0).all())
        fan_in = conv.weight.shape[1] * 9
        assert abs(float(conv.weight.detach().std()) / (2.0 / fan_in) ** 0.5 - 1) < 0.05, n


def test_sibling_heads_take_use_dpc():
    from semseg_amd.config import cfg
    from semseg_amd.network.deepv3 import DPC
    from semseg_amd.network.mscale import MscaleV3Plus
    from semseg_amd.network.attnscale import ASDV3P, ASDV3P_Paired
    before = cfg.MODEL.N_SCALES
    try:
        cfg.MODEL.N_SCALES = [0.5, 1.0]
        for cls in (MscaleV3Plus, ASDV3P, ASDV3P_Paired):
            net = cls(19, trunk="resnet-50", use_dpc=True)
            assert isinstance(net.aspp, DPC) and net.bot_aspp.weight.shape[1] == 1280, cls.__name__
            assert not isinstance(cls(19, trunk="resnet-50").aspp, DPC)
    finally:
        cfg.MODEL.N_SCALES = before


def test_unsupported_arguments_raise():
    from semseg_amd.network.deepv3 import DPC, dpc_conv, get_aspp
    with pytest.raises(NotImplementedError, match="dropout"):
        DPC(64, 64, dropout=True)
    with pytest.raises(NotImplementedError, match="separable"):
        DPC(64, 64, separable=True)
    with pytest.raises(NotImplementedError, match="separable"):
        dpc_conv(64, 64, (1, 6), True)
    for stride in (4, 32):
        with pytest.raises(ValueError, match="output stride of %d" % stride):
            DPC(64, 64, output_stride=stride)
        with pytest.raises(ValueError, match="output stride"):
            get_aspp(64, 64, stride, dpc=True)
    cell, width = get_aspp(128, 64, 16, dpc=True)
    assert isinstance(cell, DPC) and width == 320


def test_portable_route_refuses_other_convs(oracle_ops):
    """dil_conv_bn_act is for 3x3, stride 1, padding = dilation, no bias: anything else is refused, not computed."""
    from semseg_amd import nn as snn, ops
    bn = snn.BatchNorm2d(8)
    x = torch.zeros(1, 6, 6, 8)
    for kw in (dict(kernel_size=3, padding=(1, 2), dilation=(2, 1)), dict(kernel_size=3, padding=1, stride=2),
               dict(kernel_size=1), dict(kernel_size=3, padding=1, bias=True)):
        kw.setdefault("bias", False)
        with pytest.raises(AssertionError):
            ops.backend().dil_conv_bn_act(snn.DilConv2d(8, 8, **kw), bn, x)


def _net(sd, dtype=torch.float32):
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network.deepv3 import DeepV3Plus
    cfg.MODEL.N_SCALES = None
    net = DeepV3Plus(19, trunk="resnet-50", criterion=CrossEntropyLoss2d(ignore_index=255), use_dpc=True)
    net.load_state_dict(sd)
    return net.to(dtype)


def test_deepv3_dpc_train_step_and_eval(oracle_ops, gold):
    """DeepV3Plus(use_dpc=True) on the golden's 2 x 384 x 416 batch (48 x 52 at stride 8): train loss to 1e-5, the
    running-statistics samples, the sampled gradients by the 4x-floor rule, and the eval logits on the calibrated buffers
    -- test_deeper_wiring_cpu's rules."""
    from oracle.model import seeded_state_dict
    rec, calib = gold["net"], gold["calib"]
    Bn, Hn, Wn, seed = rec["batch"]
    R.assert_taps_inside(Hn // 8, Wn // 8, 8)
    images, gts = R.synth_batch(Bn, Hn, Wn, seed=seed)
    sd = seeded_state_dict(_read_keys("deepv3_dpc"), seed=rec["seed"])
    net = _net(sd).train()
    loss = net({"images": images, "gts": gts})
    loss.backward()
    print("deepv3+dpc train loss %.7f, the reference's %.7f" % (float(loss.detach()), float(rec["train_loss"])))
    check_close("deepv3+dpc train loss", loss.detach().view(1), rec["train_loss"].view(1), 1e-5, 1e-5)
    st = net.state_dict()
    for n in R.NAMES:
        assert int(st["aspp.%s.1.num_batches_tracked" % n]) == 1
    for k, v in rec["running_sample"].items():
        assert torch.allclose(st[k].flatten()[:4], v, rtol=1e-4, atol=1e-5), k
    g32 = {n: p.grad.clone() for n, p in net.named_parameters()}
    assert set(g32) == set(rec["grads"])
    del net
    net = _net(sd, torch.float64).train()
    net({"images": images.double(), "gts": gts}).backward()
    floor, dist = [0.0, 0.0], {}
    for n, p in net.named_parameters():
        g = p.grad
        idx, vals, norm = rec["grads"][n]
        a32, a64 = g32[n].flatten()[idx].double(), g.flatten()[idx]
        n32, n64 = float(g32[n].double().norm()), float(g.norm())
        floor = [max(floor[0], float((a32 - a64).norm() / a64.norm())), max(floor[1], abs(n32 - n64) / n64)]
        dist[n] = (float((a32 - vals.double()).norm() / vals.double().norm()), abs(n32 - float(norm)) / float(norm))
    print("deepv3+dpc gradients: fp32-vs-fp64 floor %.3g (samples) %.3g (norms); against the reference %.3g / %.3g over %d "
          "parameters" % (floor[0], floor[1], max(d[0] for d in dist.values()), max(d[1] for d in dist.values()), len(dist)))
    for n, (rs, rn) in dist.items():
        assert rs <= 4 * floor[0], (n, rs, floor[0])
        assert rn <= 4 * floor[1], (n, rn, floor[1])
    del net
    net = _net(sd).eval()
    net.load_state_dict(calib["calib_buffers"], strict=False)
    with torch.no_grad():
        pred = net({"images": images})["pred"]
    assert tuple(pred.shape) == (Bn, 19, Hn, Wn)
    check_close("deepv3+dpc eval pred", pred[:, :, ::16, ::16], calib["eval_pred"], 2e-3, 5e-3)
