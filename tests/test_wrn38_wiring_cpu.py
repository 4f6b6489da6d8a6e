"""Module wiring of DeepLabV3+ on the WiderResNet-38 trunk (semseg_amd.network.wider_resnet, deepv3.DeepV3PlusW38)
checked on CPU against golden vectors from the REAL reference (tests/golden/make_golden_wrn38.py), with the oracle's
operators behind the ops interface -- `add_bn_act` runs as BackendBase's composition there."""
import os

import pytest
import torch

from util import check_close

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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
    with open(os.path.join(G, "keys_wrn38.txt")) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


@pytest.fixture(scope="module")
def gold():
    return torch.load(os.path.join(G, "wrn38_golden.pt"), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def seeded(gold):
    from oracle.model import seeded_state_dict
    return seeded_state_dict(_shapes(), seed=gold["seed"])


def _net(train, sd, drop=False):
    from semseg_amd.config import cfg
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    cfg.MODEL.WRN38_CHECKPOINT = ""
    net = get_model("deepv3.DeepV3PlusW38", 19, CrossEntropyLoss2d(ignore_index=255))
    net.load_state_dict(sd)
    drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout2d)]
    assert sorted(m.p for m in drops) == [0.3, 0.5]
    if not drop:
        for m in drops:
            m.p = 0.0
    return net.train(train)


def test_wrn38_state_dict_is_the_references():
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.network import get_model
    from semseg_amd.network.utils import get_trunk
    net = get_model("deepv3.DeepV3PlusW38", 19, CrossEntropyLoss2d(ignore_index=255))
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == _shapes()
    keys = set(net.state_dict())
    for k in ("backbone.mod1.conv1.weight", "backbone.mod2.block1.bn1.0.weight", "backbone.mod2.block1.convs.conv1.weight",
              "backbone.mod6.block1.convs.bn3.0.running_var", "backbone.mod4.block1.proj_conv.weight"):
        assert k in keys, k
    assert not any("bn_out" in k or "classifier" in k for k in keys)
    assert sum(p.numel() for p in net.parameters()) == 137103936 and sum(p.numel() for p in net.backbone.parameters()) == 105062720
    trunk, s2, s4, high = get_trunk("wrn38")
    assert (s2, s4, high) == (128, 256, 4096)
    init_all = get_model("deepv3.DeepV3PlusW38I", 19, None)
    assert sorted(init_all.state_dict()) == sorted(keys)


def test_wrn38_train_step_and_eval(oracle_ops, gold, seeded):
    """Train loss to 1e-5 and eval logits to 2e-3 / 5e-3 of the reference's (test_deepv3_wiring's tolerances);
    num_batches_tracked == 1 after one step.

    Sampled gradients against the reference's, per parameter: the relative distance over the golden sample,
    |g[idx] - gold[idx]| / |gold[idx]|, and the relative difference of the gradient norms.  The bound is measured in the
    test: the same two distances between this module's own fp32 and fp64 runs on OracleBackend, per parameter; 4x the
    largest is allowed (the reference sums in place and in another order, so its fp32 noise is another draw of the same
    size).  Measured floor (largest fp32-vs-fp64 distance over the 139 parameters, random weights, batch 2 x 96 x 128: mod6 /
    mod7 normalise over 384 samples): 1.46e-2 on the samples and 1.71e-3 on the norms, i.e. bounds of 5.8e-2 and 6.8e-3; the
    reference's gradients lie within 4.64e-2 and 2.52e-3."""
    net = _net(True, seeded)
    loss = net({"images": gold["images"], "gts": gold["gts"]})
    loss.backward()
    check_close("wrn38 train loss", loss.detach().view(1), gold["train_loss"].view(1), 1e-5, 1e-5)
    sd = net.state_dict()
    for k in ("backbone.mod2.block1.bn1.0.num_batches_tracked", "backbone.mod4.block3.bn1.0.num_batches_tracked",
              "backbone.mod7.block1.convs.bn3.0.num_batches_tracked", "aspp.features.0.1.num_batches_tracked"):
        assert int(sd[k]) == 1, k
    # (the loss is held to 1e-5 relative; a running mean is 0.1 x a batch mean of activations of order 1 that may itself
    # be near zero, so the same 1e-5 is the absolute allowance)
    worst = max(float((sd[k].flatten()[:4] - v).abs().max()) for k, v in gold["running_sample"].items())
    print("wrn38 running statistics: largest absolute distance from the reference's samples %.3g" % worst)
    for k, v in gold["running_sample"].items():
        assert torch.allclose(sd[k].flatten()[:4], v, rtol=1e-4, atol=1e-5), k
    g32 = {n: p.grad.clone() for n, p in net.named_parameters()}
    assert set(g32) == set(gold["grads"])
    del net

    net = _net(True, seeded).double()
    loss64 = net({"images": gold["images"].double(), "gts": gold["gts"]})
    loss64.backward()
    floor_s = floor_n = 0.0
    dist = {}
    for n, p in net.named_parameters():
        idx, vals, norm = gold["grads"][n]
        a32, a64 = g32[n].flatten()[idx].double(), p.grad.flatten()[idx]
        floor_s = max(floor_s, float((a32 - a64).norm() / a64.norm()))
        floor_n = max(floor_n, abs(float(g32[n].double().norm()) - float(p.grad.norm())) / float(p.grad.norm()))
        dist[n] = (float((a32 - vals.double()).norm() / vals.double().norm()),
                   abs(float(g32[n].double().norm()) - float(norm)) / float(norm))
    worst_s, worst_n = max(d[0] for d in dist.values()), max(d[1] for d in dist.values())
    print("wrn38 gradients: fp32-vs-fp64 floor %.3g (samples) %.3g (norms); against the reference %.3g / %.3g over %d parameters"
          % (floor_s, floor_n, worst_s, worst_n, len(dist)))
    for n, (ds, dn) in dist.items():
        assert ds <= 4 * floor_s, (n, ds, floor_s)
        assert dn <= 4 * floor_n, (n, dn, floor_n)
    del net

    net = _net(False, seeded)
    net.load_state_dict(gold["calib_buffers"], strict=False)
    with torch.no_grad():
        o = net({"images": gold["images"]})
    assert tuple(o["pred"].shape) == (2, 19, 96, 128)
    check_close("wrn38 eval pred", o["pred"][:, :, ::8, ::8], gold["eval_pred"], 2e-3, 5e-3)


def test_wrn38_dropout_masks(gold, seeded):
    """With p restored (0.3 in mod6, 0.5 in mod7) and a fixed seed: the BatchNorm + ReLU in front of the last conv of
    mod6 / mod7 is handed a per-(image, channel) multiplier that is 0 at about the drawn rate (within 4 sigma of the
    binomial) and 1 / keep elsewhere, and its output is the unmasked output with whole channels zeroed and the rest scaled
    by 1 / keep; no other BatchNorm of the network gets a mask."""
    from semseg_amd import ops
    from oracle_backend import OracleBackend
    seen = []

    class Recording(OracleBackend):
        def _batch_norm_act(self, x, bn, residual=None, relu=False, post=None):
            out = OracleBackend._batch_norm_act(self, x, bn, residual, relu, post)
            if post is not None:
                with torch.no_grad():
                    base = OracleBackend._batch_norm_act(self, x, bn, residual, relu, None)
                seen.append((bn, post.clone(), base, out.detach()))
            return out

    prev = ops._BACKEND
    ops._set_backend_for_tests(Recording())
    try:
        net = _net(True, seeded, drop=True)
        torch.manual_seed(7)
        with torch.no_grad():
            net({"images": gold["images"], "gts": gold["gts"]})
    finally:
        ops._set_backend_for_tests(prev)
    want = [(net.backbone.mod6.block1.convs.bn3[0], 0.3, 1024), (net.backbone.mod7.block1.convs.bn3[0], 0.5, 2048)]
    assert len(seen) == 2
    for (bn, post, base, out), (wbn, p, width) in zip(seen, want):
        assert bn is wbn and tuple(post.shape) == (2, width)
        keep = 1.0 - p
        dropped = post == 0
        assert bool(((post == 0) | ((post - 1.0 / keep).abs() < 1e-6)).all())
        rate, sigma = float(dropped.float().mean()), (p * keep / post.numel()) ** 0.5
        assert abs(rate - p) <= 4 * sigma, (rate, p, sigma)
        m = dropped[:, None, None, :].expand_as(out)
        assert float(out[m].abs().max()) == 0.0
        assert float(base.abs().max()) > 0
        assert torch.allclose(out[~m], base[~m] / keep, rtol=1e-6, atol=0)


def test_wrn38_checkpoint_round_trip(tmp_path):
    """cfg.MODEL.WRN38_CHECKPOINT: checkpoint['state_dict'] of the ImageNet classifier saved from a DataParallel wrapper --
    `module.` stripped, classifier.* and bn_out.* dropped, the rest loaded strictly (a missing key raises).  The synthetic
    file holds one distinct scalar per key, expanded to the key's shape (a few KB on disk)."""
    from semseg_amd.config import cfg
    from semseg_amd.network.wider_resnet import wrn38
    assert cfg.MODEL.WRN38_CHECKPOINT == ""
    ref = wrn38()                                           # default: random init, no file needed
    sd, vals = {}, {}
    for i, (k, v) in enumerate(ref.state_dict().items()):
        vals[k] = (i + 1) if v.dtype == torch.long else 0.25 + i / 1024.0
        sd["module." + k] = torch.full((1,) * v.dim(), vals[k], dtype=v.dtype).expand(v.shape)
    sd["module.bn_out.0.weight"] = torch.ones(4096)
    sd["module.bn_out.0.bias"] = torch.zeros(4096)
    sd["module.classifier.fc.weight"] = torch.zeros(1, 1).expand(1000, 4096)
    sd["module.classifier.fc.bias"] = torch.zeros(1000)
    path = str(tmp_path / "wider_resnet38.pth.tar")
    torch.save({"state_dict": sd, "epoch": 0}, path)
    assert os.path.getsize(path) < 2 << 20
    cfg.MODEL.WRN38_CHECKPOINT = path
    try:
        net = wrn38(pretrained=True)
        for k, v in net.state_dict().items():
            assert bool((v == vals[k]).all()), k
        del sd["module.mod3.block2.convs.conv1.weight"]
        torch.save({"state_dict": sd}, path)
        with pytest.raises(RuntimeError):
            wrn38(pretrained=True)
    finally:
        cfg.MODEL.WRN38_CHECKPOINT = ""
