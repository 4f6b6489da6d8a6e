"""Golden fixtures for the Dense Prediction Cell (network/utils.py:249-311: dpc_conv, DPC, get_aspp(dpc=True)) and for
DeepLabV3+ with it (network/deepv3.py:44-93, DeepV3Plus(use_dpc=True)) generated from the REAL reference.  Run in the
build container:
    python tests/golden/make_golden_dpc.py
Writes
    dpc_golden.pt         "module": per output stride (16 and 8) the cell alone on small channel counts, in train() --
                          output, input gradient, every parameter gradient, the updated running statistics -- and its
                          eval() output (sub-sampled) on buffers calibrated on the same input;
                          "net": DeepV3Plus(19, trunk='resnet-50', use_dpc=True) on a 384 x 416 crop (48 x 52 at stride 8):
                          train loss, sampled parameter gradients, BN running-stat samples -- deepv3_golden.pt's record.
    dpc_golden_calib.pt   the network's calibrated buffers and sub-sampled eval logits
    keys_deepv3_dpc.txt   state_dict keys + shapes of the network
The inputs are not stored: tests/dpc_ref.py rebuilds them (module_inputs, synth_batch with the stored seed).  Every
feature map is asserted to have H > dil_h and W > dil_w for each of the five rate pairs: on a smaller map (the 12 x 16
of deepv3_golden.pt's 96 x 128 crop) the (36, 30) conv is a 1x1 conv and the golden is blind to its off-centre taps."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from ref_bootstrap import bootstrap  # noqa: E402
from make_golden import synth_batch, sample_idx  # noqa: E402
from oracle.model import seeded_state_dict  # noqa: E402
import dpc_ref  # noqa: E402

MODULE_SEED, NET_SEED = 11, 3


def module_record(utils, output_stride):
    B, cin, red, H, W = dpc_ref.MODULE_CASES[output_stride]
    dpc_ref.assert_taps_inside(H, W, output_stride)
    cell = utils.DPC(cin, red, output_stride=output_stride)
    shapes = [(k, tuple(v.shape)) for k, v in cell.state_dict().items()]
    assert shapes == dpc_ref.module_shapes(cin, red), shapes
    sd = seeded_state_dict(shapes, seed=MODULE_SEED + output_stride)
    cell.load_state_dict(sd)
    x64, gy64 = dpc_ref.module_inputs(output_stride)
    x = x64.float().requires_grad_(True)
    cell.train()
    out = cell(x)
    (out * gy64.float()).sum().backward()
    rec = {"seed": MODULE_SEED + output_stride, "out": out.detach().clone(), "dx": x.grad.clone(),
           "grads": {n: p.grad.clone() for n, p in cell.named_parameters()},
           "running": {k: v.clone() for k, v in cell.state_dict().items() if "running" in k}}
    # eval on statistics calibrated on this input (momentum 1.0), as the network record does
    cell.load_state_dict(sd)
    bns = [m for m in cell.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    with torch.no_grad():
        cell(x.detach())
    rec["calib"] = {k: v.clone() for k, v in cell.state_dict().items() if "running" in k}
    cell.eval()
    with torch.no_grad():
        rec["eval_out"] = cell(x.detach())[:, :, ::2, ::2].clone()
    return rec


def main():
    bootstrap(19)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import network.Resnet as Resnet
    Resnet.resnet50.__defaults__ = (False,)          # no checkpoint download
    import network.deepv3 as deepv3
    import network.utils as utils
    from loss.utils import CrossEntropyLoss2d
    gold = {"module": {s: module_record(utils, s) for s in (16, 8)}}

    net = deepv3.DeepV3Plus(19, trunk="resnet-50", criterion=CrossEntropyLoss2d(ignore_index=255), use_dpc=True)
    assert isinstance(net.aspp, utils.DPC)
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, "keys_deepv3_dpc.txt"), "w") as f:
        for k, s in shapes:
            f.write("%s %s\n" % (k, ",".join(map(str, s))))
    sd = seeded_state_dict(shapes, seed=NET_SEED)
    net.load_state_dict(sd)
    B, H, W, seed = dpc_ref.NET_BATCH
    dpc_ref.assert_taps_inside(H // 8, W // 8, 8)
    images, gts = synth_batch(B, H, W, seed=seed)
    i2, g2 = dpc_ref.synth_batch(B, H, W, seed=seed)
    assert torch.equal(images, i2) and torch.equal(gts, g2)
    rec = {"seed": NET_SEED, "batch": dpc_ref.NET_BATCH}
    net.train()
    loss = net({"images": images, "gts": gts})
    loss.backward()
    rec["train_loss"] = loss.detach()
    grads = {}
    for name, p in net.named_parameters():
        flat = p.grad.flatten()
        idx = sample_idx(flat.numel())
        grads[name] = (idx, flat[idx].clone(), flat.norm().clone())
    rec["grads"] = grads
    rec["running_sample"] = {k: v.flatten()[:4].clone() for k, v in net.state_dict().items()
                             if k.endswith("running_mean") or k.endswith("running_var")}
    gold["net"] = rec
    torch.save(gold, os.path.join(HERE, "dpc_golden.pt"))
    # eval on BN statistics calibrated on this batch (momentum 1.0), as make_golden_deepv3.py does
    net.load_state_dict(sd)
    net.train()
    bns = [m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = 1.0
    with torch.no_grad():
        net({"images": images, "gts": gts})
    for m in bns:
        m.momentum = 0.1
    calib = {"calib_buffers": {k: v.clone() for k, v in net.state_dict().items()
                               if k.endswith("running_mean") or k.endswith("running_var")}}
    net.eval()
    with torch.no_grad():
        calib["eval_pred"] = net({"images": images})["pred"][:, :, ::16, ::16].clone()
    torch.save(calib, os.path.join(HERE, "dpc_golden_calib.pt"))
    print("train_loss", float(rec["train_loss"]), "keys", len(shapes), "params", sum(p.numel() for p in net.parameters()))


if __name__ == "__main__":
    main()
