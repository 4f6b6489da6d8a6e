"""Golden fixture for DeepLabV3+ on the WiderResNet-38 trunk (scripts/train_cityscapes_deepv3.yml:
--arch deepv3.DeepV3PlusW38; network/deepv3.py:108-109, network/wider_resnet.py:71-185,269-434) generated
from the REAL reference.  Run in the build container:
    python tests/golden/make_golden_wrn38.py
Writes wrn38_golden.pt (train loss, sampled parameter gradients plus norms, BN running-stat
samples, calibrated buffers, sub-sampled eval logits) and keys_wrn38.txt (state_dict keys+shapes).
The two Dropout2d probabilities (0.3 in mod6, 0.5 in mod7) are 0 for the train step: the mask draws of
the two implementations are not the same random stream."""
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


def main():
    bootstrap(19)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    import network.utils as ref_utils
    ref_wrn38 = ref_utils.wrn38
    ref_utils.wrn38 = lambda pretrained=True: ref_wrn38(pretrained=False)       # no ImageNet checkpoint in the container
    import network.deepv3 as deepv3
    from loss.utils import CrossEntropyLoss2d
    net = deepv3.DeepV3PlusW38(19, CrossEntropyLoss2d(ignore_index=255))
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, "keys_wrn38.txt"), "w") as f:
        for k, s in shapes:
            f.write("%s %s\n" % (k, ",".join(map(str, s))))
    sd = seeded_state_dict(shapes, seed=3)
    net.load_state_dict(sd)
    drops = [m for m in net.modules() if isinstance(m, torch.nn.Dropout2d)]
    assert sorted(m.p for m in drops) == [0.3, 0.5]
    for m in drops:
        m.p = 0.0
    images, gts = synth_batch(2, 96, 128, seed=4321)
    gold = {"images": images, "gts": gts, "seed": 3}
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
    gold["calib_buffers"] = {k: v.clone() for k, v in net.state_dict().items()
                             if k.endswith("running_mean") or k.endswith("running_var")}
    net.eval()
    with torch.no_grad():
        gold["eval_pred"] = net({"images": images})["pred"][:, :, ::8, ::8].clone()
    torch.save(gold, os.path.join(HERE, "wrn38_golden.pt"))
    print("train_loss", float(gold["train_loss"]), "keys", len(shapes), "params",
          sum(p.numel() for p in net.parameters()))


if __name__ == "__main__":
    main()
