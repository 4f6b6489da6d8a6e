"""Golden fixture for DeepLabV3+ on the SE-ResNeXt-50 trunk (--arch deepv3.DeepV3PlusSRNX50; network/deepv3.py:96-97,
network/SEresnext.py, network/utils.py:48-99) generated from the REAL reference.  Run in the build container:
    python tests/golden/make_golden_srnx.py
Writes srnx50_golden.pt (train loss, sampled parameter gradients plus norms, BN running-stat samples, sub-sampled eval
logits), srnx50_golden_calib.pt (the calibrated buffers the eval logits were computed on), keys_srnx50.txt and
keys_srnx101.txt (state_dict keys+shapes).

Two things about the reference are pinned here.  (1) network.SEresnext.initialize_pretrained_model downloads the ImageNet
file; it is replaced by a no-op BEFORE anything is built, so this generator never reaches for the network.  (2) get_trunk
returns s2_ch = 48 for the SE-ResNeXt trunks although layer1 delivers 256 channels, so the factory as shipped raises in
bot_fine on its first forward (asserted below); the fixture is taken with get_trunk wrapped to return 256, the value the
project's get_trunk returns, and the key lists hold that bot_fine shape ([48, 256, 1, 1])."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ref_bootstrap import bootstrap  # noqa: E402
from make_golden import synth_batch, sample_idx  # noqa: E402
from oracle.model import seeded_state_dict  # noqa: E402


def write_keys(net, name):
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, name), "w") as f:
        for k, s in shapes:
            f.write("%s %s\n" % (k, ",".join(map(str, s))))
    return shapes


def main():
    bootstrap(19)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import network.SEresnext as ref_srnx
    ref_srnx.initialize_pretrained_model = lambda model, num_classes, settings: None      # never downloads
    import network.deepv3 as deepv3
    from loss.utils import CrossEntropyLoss2d
    images, gts = synth_batch(2, 96, 128, seed=4321)

    shipped = deepv3.DeepV3PlusSRNX50(19, CrossEntropyLoss2d(ignore_index=255))
    assert tuple(shipped.bot_fine.weight.shape) == (48, 48, 1, 1)
    print("as shipped: keys", len(shipped.state_dict()), "params", sum(p.numel() for p in shipped.parameters()),
          "backbone", sum(p.numel() for p in shipped.backbone.parameters()))
    try:
        with torch.no_grad():
            shipped.eval()({"images": images})
        raise AssertionError("the shipped DeepV3PlusSRNX50 ran a forward")
    except RuntimeError as e:
        assert "to have 48 channels" in str(e) and "256" in str(e), str(e)
        print("as shipped:", str(e).splitlines()[0])
    del shipped

    ref_get_trunk = deepv3.get_trunk

    def get_trunk(trunk_name, output_stride=8):
        backbone, s2_ch, s4_ch, high = ref_get_trunk(trunk_name, output_stride=output_stride)
        return backbone, (256 if trunk_name.startswith("seresnext") else s2_ch), s4_ch, high
    deepv3.get_trunk = get_trunk

    net101 = deepv3.DeepV3PlusSRNX101(19, CrossEntropyLoss2d(ignore_index=255))
    k101 = write_keys(net101, "keys_srnx101.txt")
    print("srnx101 keys", len(k101), "params", sum(p.numel() for p in net101.parameters()))
    del net101

    net = deepv3.DeepV3PlusSRNX50(19, CrossEntropyLoss2d(ignore_index=255))
    shapes = write_keys(net, "keys_srnx50.txt")
    assert not any(isinstance(m, (torch.nn.Dropout, torch.nn.Dropout2d)) for m in net.modules())
    sd = seeded_state_dict(shapes, seed=3)
    net.load_state_dict(sd)
    gates = []
    for m in net.modules():
        if isinstance(m, ref_srnx.SEModule):
            m.sigmoid.register_forward_hook(lambda mod, inp, out: gates.append(out.detach().flatten()))
    gold = {"images": images, "gts": gts, "seed": 3}
    net.train()
    loss = net({"images": images, "gts": gts})
    loss.backward()
    assert len(gates) == 16
    lo, hi = min(float(g.min()) for g in gates), max(float(g.max()) for g in gates)
    print("gates: 16 blocks in (%.3f, %.3f), smallest per-block standard deviation %.3f" %
          (lo, hi, min(float(g.std()) for g in gates)))
    assert 0.05 < lo and hi < 0.95
    gold["train_loss"] = loss.detach()
    grads = {}
    for name, p in net.named_parameters():
        flat = p.grad.flatten()
        idx = sample_idx(flat.numel())
        grads[name] = (idx, flat[idx].clone(), flat.norm().clone())
        if ".se_module." in name:
            assert float(flat.norm()) > 0, name
    gold["grads"] = grads
    gold["running_sample"] = {k: v.flatten()[:4].clone() for k, v in net.state_dict().items()
                              if k.endswith("running_mean") or k.endswith("running_var")}
    # eval on BN statistics calibrated on this batch (momentum 1.0), as make_golden.py does
    net.load_state_dict(sd)
    net.train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    with torch.no_grad():
        net({"images": images, "gts": gts})
    for m in bns:
        m.momentum = 0.1
    calib = {k: v.clone() for k, v in net.state_dict().items() if k.endswith("running_mean") or k.endswith("running_var")}
    net.eval()
    with torch.no_grad():
        gold["eval_pred"] = net({"images": images})["pred"][:, :, ::8, ::8].clone()
    # two files, each below the repository's 1 MiB limit for a committed file; the labels as bytes (19 classes and 255)
    gold["gts"] = gts.to(torch.uint8)
    assert torch.equal(gold["gts"].long(), gts)
    torch.save(gold, os.path.join(HERE, "srnx50_golden.pt"))
    torch.save({"calib_buffers": calib}, os.path.join(HERE, "srnx50_golden_calib.pt"))
    for f in ("srnx50_golden.pt", "srnx50_golden_calib.pt", "keys_srnx50.txt", "keys_srnx101.txt"):
        assert os.path.getsize(os.path.join(HERE, f)) < 1 << 20, f
    print("train_loss", float(gold["train_loss"]), "keys", len(shapes), "params",
          sum(p.numel() for p in net.parameters()), "backbone", sum(p.numel() for p in net.backbone.parameters()))


if __name__ == "__main__":
    main()
