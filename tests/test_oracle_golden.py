"""Pin the oracle (oracle/ops.py, oracle/model.py) against golden vectors that
tests/golden/make_golden.py produced by running the REAL reference
(/root/reference: loss/rmi.py, loss/utils.py, network/ocrnet.py) on CPU.
CPU-only; runs everywhere."""
import os

import pytest
import torch

from util import check_close

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    return torch.load(os.path.join(G, name), map_location="cpu", weights_only=False)


def _shapes():
    out = []
    with open(os.path.join(G, "keys.txt")) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            out.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    return out


def test_keys_inventory():
    shapes = _shapes()
    assert len(shapes) == 1903
    assert shapes[0][0] == "backbone.conv1.weight"
    assert shapes[-1][0] == "scale_attn.conv2.weight"


@pytest.mark.parametrize("do_rmi", [False, True])
def test_rmi_loss_matches_reference(do_rmi):
    from oracle import ops as O
    g = _load("rmi_golden.pt")
    lg = g["logits"].clone().requires_grad_(True)
    loss = O.rmi_loss(lg, g["gts"], 19, do_rmi=do_rmi)
    loss.backward()
    check_close("rmi loss", loss.view(1), g["loss_rmi%d" % do_rmi].view(1), 1e-6, 1e-6)
    check_close("rmi grad", lg.grad, g["grad_rmi%d" % do_rmi], 1e-5, 1e-5)


def test_cross_entropy_matches_reference():
    from oracle import ops as O
    g = _load("ce_golden.pt")
    lg = g["logits"].clone().requires_grad_(True)
    loss = O.cross_entropy(lg, g["gts"], 255)
    loss.backward()
    check_close("ce loss", loss.view(1), g["loss"].view(1), 1e-6, 1e-6)
    check_close("ce grad", lg.grad, g["grad"], 1e-6, 1e-6)


def _loss65_inputs():
    """tests/golden/make_golden_loss65.py's inputs(): the logits are regenerated from the seed, not stored."""
    g = torch.Generator().manual_seed(65)
    logits = torch.randn(2, 65, 15, 18, generator=g) * 2
    return logits


@pytest.mark.parametrize("which", ["bce", "bce_rmi", "ce"])
def test_losses_at_65_classes_match_reference(which):
    """Mapillary's class count and ignore label (65 = C): RMILoss(num_classes=65, ignore_index=65) with do_rmi False /
    True and CrossEntropyLoss2d(ignore_index=65) of the reference, at H % 4 == 3 -- the oracle the GPU loss tests
    compare against is the reference there too."""
    from oracle import ops as O
    g = _load("loss65_golden.pt")
    logits = _loss65_inputs()
    assert float(logits.double().sum()) == pytest.approx(float(g["logits_sum"]), abs=1e-9)
    assert float(logits.double().abs().sum()) == pytest.approx(float(g["logits_abs_sum"]), abs=1e-9)
    gts = g["gts"].long()
    assert int((gts == 65).sum()) > 0 and int(gts.max()) == 65
    lg = logits.clone().requires_grad_(True)
    if which == "ce":
        loss = O.cross_entropy(lg, gts, 65)
        key = "ce"
    else:
        loss = O.rmi_loss(lg, gts, 65, do_rmi=which == "bce_rmi")
        key = "rmi%d" % (which == "bce_rmi")
    loss.backward()
    check_close("loss65 " + which, loss.view(1), g["loss_" + key].view(1), 1e-6, 1e-6)
    check_close("loss65 grad " + which, lg.grad, g["grad_" + key], 1e-6, 1e-6)


@pytest.fixture(scope="module")
def gold():
    return _load("mscale_golden.pt")


def _oracle_net(training, **kw):
    from oracle.model import Net, seeded_state_dict
    sd = seeded_state_dict(_shapes(), seed=0)
    for k, v in sd.items():
        if v.is_floating_point() and not ("running_" in k):
            v.requires_grad_(training)
    used = set()
    return Net(sd, 19, training=training, used=used, **kw), sd, used


def test_mscale_train_step_matches_reference(gold):
    net, sd, used = _oracle_net(True, mscale_wt=0.05)
    loss = net.two_scale_forward(gold["images"], gold["gts"])
    loss.backward()
    assert used == set(sd.keys()), sorted(set(sd.keys()) ^ used)[:10]
    check_close("train loss", loss.detach().view(1), gold["train_loss"].view(1), 1e-5, 1e-5)
    worst = 0.0
    for name, (idx, vals, norm) in gold["grads"].items():
        gflat = sd[name].grad.flatten()
        rel = float((gflat.norm() - norm).abs() / (norm + 1e-12))
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
        assert torch.allclose(gflat[idx], vals, rtol=5e-3, atol=1e-6 + 2e-3 * float(vals.abs().max())), name
    print("worst grad-norm rel err", worst)
    bad = [k for k, v in gold["running_sample"].items()
           if not torch.allclose(sd[k].flatten()[:4], v, rtol=1e-3, atol=1e-5)]
    assert len(bad) <= 3, bad   # a few 4-sample BN layers are noise-dominated


def test_mscale_eval_matches_reference(gold):
    net, sd, _ = _oracle_net(False)
    for k, v in gold["calib_buffers"].items():
        sd[k].copy_(v)
    with torch.no_grad():
        o = net.two_scale_forward(gold["images"])
    for k, v in gold["eval"].items():
        check_close("eval " + k, o[k][:, :, ::8, ::8], v, 1e-4, 1e-4)
    with torch.no_grad():
        o = net.nscale_forward(gold["images"], [0.5, 1.0, 2.0])
    for k, v in gold["eval_nscale"].items():
        check_close("nscale " + k, o[k][:, :, ::8, ::8], v, 1e-4, 1e-4)


def test_deepv3_oracle_matches_reference():
    """DeepLabV3+/ResNet-50 (BASELINE configs[0]): oracle/deepv3.py vs the real
    reference's train loss, sampled gradients of all 161 parameters, BN running
    statistics and eval logits (tests/golden/make_golden_deepv3.py)."""
    import os
    from oracle.deepv3 import DeepV3PlusNet
    from oracle.model import seeded_state_dict
    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    gold = torch.load(os.path.join(G, "deepv3_golden.pt"), map_location="cpu", weights_only=False)
    shapes = []
    with open(os.path.join(G, "keys_deepv3.txt")) as f:
        for line in f:
            k, _, s = line.strip().partition(" ")
            shapes.append((k, tuple(int(v) for v in s.split(",")) if s else ()))
    sd = seeded_state_dict(shapes, seed=gold["seed"])
    for k, v in sd.items():
        if v.is_floating_point() and "running_" not in k:
            v.requires_grad_(True)
    loss = DeepV3PlusNet(sd, 19, training=True).forward(gold["images"], gold["gts"])
    loss.backward()
    assert abs(float(loss) - float(gold["train_loss"])) <= 1e-5 * abs(float(gold["train_loss"]))
    for name, (idx, vals, norm) in gold["grads"].items():
        g = sd[name].grad.flatten()
        assert torch.allclose(g[idx], vals, rtol=2e-3, atol=2e-6 * float(norm) + 1e-9), name
        assert abs(float(g.norm()) - float(norm)) <= 1e-3 * float(norm) + 1e-9, name
    for k, v in gold["running_sample"].items():
        assert torch.allclose(sd[k].detach().flatten()[:4], v, rtol=1e-4, atol=1e-6), k
    sd2 = seeded_state_dict(shapes, seed=gold["seed"])
    sd2.update(gold["calib_buffers"])
    with torch.no_grad():
        pred = DeepV3PlusNet(sd2, 19, training=False).forward(gold["images"])["pred"]
    ref = gold["eval_pred"]
    assert float((pred[:, :, ::8, ::8] - ref).abs().max()) <= 2e-4 * float(ref.abs().max())


def test_mscale_eval_four_scales_65_classes_matches_reference():
    """BASELINE configs[4]'s recipe chain (scripts/eval_mapillary.yml:13-18: n_scales 0.25,0.5,1.0,2.0, 65 classes):
    `nscale_forward` (network/ocrnet.py:185-262) performs two consecutive `s < 1.0` fusions; the oracle against the
    real reference's outputs (tests/golden/make_golden_nscale4.py), every key of the output dict (the fixture also holds the
    three-scale chain on the same 65-class weights; the 19-class three-scale chain is pinned above)."""
    from oracle.model import Net, seeded_state_dict
    g = _load("nscale4_golden.pt")
    assert g["num_classes"] == 65 and g["scales4"] == [0.25, 0.5, 1.0, 2.0]
    sd = seeded_state_dict(g["shapes"], seed=g["seed"])
    for k, v in g["calib_buffers"].items():
        sd[k].copy_(v)
    net = Net(sd, 65, training=False)

    def sample(v):
        st = 16 if v.shape[1] > 1 else 8
        return v[:, :, ::st, ::st]

    with torch.no_grad():
        o = net.nscale_forward(g["images"], g["scales4"])
    assert sorted(o) == sorted(g["eval_nscale4"]), (sorted(o), sorted(g["eval_nscale4"]))
    for k, v in g["eval_nscale4"].items():
        check_close("nscale4 " + k, sample(o[k]), v, 1e-4, 1e-4)
