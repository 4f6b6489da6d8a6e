"""Golden fixtures for the Deeper (Panoptic-DeepLab style) decoders, generated from the REAL reference
(network/deeper.py:36-87, network/mscale.py:363-442).  Run in the build container:
    python tests/golden/make_golden_deeper.py
Two configurations, so that each trunk and each class is pinned once:
    deeper.DeeperX71   DeeperS8 on Xception-71, cross entropy              -> deeper_x71_golden.pt (+ _calib.pt)
    mscale.DeeperW38   MscaleDeeper on WiderResNet-38, two-scale training loss with SUPERVISED_MSCALE_WT = 0.05,
                       two-scale evaluation (cfg.MODEL.N_SCALES unset)     -> mscale_deeper_w38_golden.pt (+ _calib.pt)
Each holds the train loss, sampled parameter gradients plus norms, BN running-stat samples and sub-sampled eval
outputs; the _calib files the calibrated running statistics the eval outputs were computed on (a file of their own:
every committed file stays below 1 MiB).  keys_deeper_x71.txt / keys_mscale_deeper_w38.txt: state_dict keys + shapes.
Batch 2 x 96 x 128: both sides divide by 16, so the 0.5x pass of the two-scale forward still lands on the stride-8
grid (the x2 upsampling steps of the decoder need every level to be exactly half of the one below).  WiderResNet-38's
two Dropout2d probabilities are 0 for the train step (the mask draws of the two implementations differ)."""
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

# stem of the files, module, factory, SUPERVISED_MSCALE_WT
CONFIGS = (
    ("deeper_x71", "deeper", "DeeperX71", 0),
    ("mscale_deeper_w38", "mscale", "DeeperW38", 0.05),
)


def main():
    cfg = bootstrap(19)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import importlib
    import network.utils as ref_utils
    # (no ImageNet checkpoints in the container)
    ref_x71, ref_wrn38 = ref_utils.xception71, ref_utils.wrn38
    ref_utils.xception71 = lambda output_stride, BatchNorm, pretrained=True: ref_x71(
        output_stride=output_stride, BatchNorm=BatchNorm, pretrained=False)
    ref_utils.wrn38 = lambda pretrained=True: ref_wrn38(pretrained=False)
    from loss.utils import CrossEntropyLoss2d
    for stem, modname, factory, wt in CONFIGS:
        cfg.LOSS.SUPERVISED_MSCALE_WT = wt
        cfg.MODEL.N_SCALES = None
        mod = importlib.import_module("network." + modname)
        net = getattr(mod, factory)(19, CrossEntropyLoss2d(ignore_index=255))
        shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
        with open(os.path.join(HERE, "keys_%s.txt" % stem), "w") as f:
            for k, s in shapes:
                f.write("%s %s\n" % (k, ",".join(map(str, s))))
        for m in net.modules():
            if isinstance(m, torch.nn.Dropout2d):
                m.p = 0.0
        sd = seeded_state_dict(shapes, seed=3)
        net.load_state_dict(sd)
        images, gts = synth_batch(2, 96, 128, seed=4321)
        gold = {"images": images, "seed": 3, "wt": wt}
        net.train()
        loss = net({"images": images, "gts": gts})
        loss.backward()
        gold["train_loss"] = loss.detach()
        grads = {}
        for name, p in net.named_parameters():
            flat = p.grad.flatten()
            idx = sample_idx(flat.numel())
            grads[name] = (idx, flat[idx].clone(), flat.norm().clone())
        gold["grads"] = grads
        gold["running_sample"] = {k: v.flatten()[:4].clone() for k, v in net.state_dict().items()
                                  if k.endswith("running_mean") or k.endswith("running_var")}
        # eval on BN statistics calibrated on this batch (momentum 1.0), as make_golden.py does; under the two-scale
        # forward the statistics of the pass the reference runs LAST (the 1.0x one) are what stays
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
            o = net({"images": images, "gts": gts})
            gold["eval"] = {k: v[:, :, ::8, ::8].clone() for k, v in o.items()}
        gold["gts"] = gts.to(torch.uint8)                   # 19 classes and 255
        assert torch.equal(gold["gts"].long(), gts)
        torch.save(gold, os.path.join(HERE, "%s_golden.pt" % stem))
        torch.save({"calib_buffers": calib}, os.path.join(HERE, "%s_golden_calib.pt" % stem))
        print(stem, "train_loss", float(gold["train_loss"]), "keys", len(shapes), "params",
              sum(p.numel() for p in net.parameters()), "eval", sorted(gold["eval"]))


if __name__ == "__main__":
    main()
