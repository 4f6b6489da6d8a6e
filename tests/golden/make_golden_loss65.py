"""Generate tests/golden/loss65_golden.pt from the REAL reference at Mapillary's class count.

Run in the build container (where the reference checkout exists):
    python tests/golden/make_golden_loss65.py
RMILoss(num_classes=65, ignore_index=65) with do_rmi False and True (loss/rmi.py) and CrossEntropyLoss2d(ignore_index=65)
(loss/utils.py) on a small seeded input: 2 x 65 x 15 x 18 (H % 4 == 3: the last row lies in no pooling window), labels
in large blocks with scattered and banded ignore label 65 (= C: out of range).  Stored: the labels, the losses, the
logit gradients and a checksum of the logits; the logits themselves are regenerated from the seed (`inputs()`, repeated
in tests/test_oracle_golden.py)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from ref_bootstrap import bootstrap  # noqa: E402

C, IGN = 65, 65


def inputs():
    g = torch.Generator().manual_seed(65)
    logits = torch.randn(2, C, 15, 18, generator=g) * 2
    blocks = torch.randint(0, C, (2, 4, 5), generator=g)
    gts = blocks.repeat_interleave(4, 1).repeat_interleave(4, 2)[:, :15, :18].clone()
    gts[torch.rand(2, 15, 18, generator=g) < 0.1] = IGN
    gts[1, :, 7] = IGN
    return logits, gts.long()


def main():
    bootstrap(C)
    torch.set_num_threads(8)
    from loss.rmi import RMILoss
    from loss.utils import CrossEntropyLoss2d
    logits, gts = inputs()
    out = {"gts": gts.to(torch.uint8), "logits_sum": logits.double().sum(), "logits_abs_sum": logits.double().abs().sum()}
    crit = RMILoss(num_classes=C, ignore_index=IGN)
    for do_rmi in (False, True):
        lg = logits.clone().requires_grad_(True)
        loss = crit(lg, gts, do_rmi=do_rmi)
        loss.backward()
        out["loss_rmi%d" % do_rmi] = loss.detach()
        out["grad_rmi%d" % do_rmi] = lg.grad.clone()
    ce = CrossEntropyLoss2d(ignore_index=IGN)
    lg = logits.clone().requires_grad_(True)
    loss = ce(lg, gts)
    loss.backward()
    out["loss_ce"] = loss.detach()
    out["grad_ce"] = lg.grad.clone()
    torch.save(out, os.path.join(HERE, "loss65_golden.pt"))


if __name__ == "__main__":
    main()
