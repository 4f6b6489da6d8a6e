"""Generate tests/golden/relaxloss_golden.pt from the REAL reference: the label relaxation of --jointwtborder.

Run in the build container (where the reference checkout exists):
    python tests/golden/make_golden_relaxloss.py
For cases 1-7 of tests/relaxloss_cases.py: RelaxedBoundaryLossToTensor(ignore, C) (transforms/transforms.py:74-123) on
every label map of the batch under the case's cfg.BORDER_WINDOW / cfg.STRICTBORDERCLASS, then ImgWtLossSoftNLL
(loss/utils.py:150-231) under the case's cfg.BATCH_WEIGHTING and upper bound on the seeded logits, backward with the
case's upstream gradient.  Stored per case: the uint8 labels, the reference's multi-hot targets, calculate_weights as
torch.Tensor() makes them (per image, or the batch's for every image), the loss, the logit gradient and a checksum of the
logits (regenerated from the seed by relaxloss_cases.inputs()).

scikit-image is not installed where this was recorded: transforms/transforms.py imports three of its functions at module
level, none of which these cases reach (find_boundaries only in the reduced-border mode), so they are stubbed the way
make_golden_gblur.py does.  scipy.ndimage.interpolation.shift is LIVE SciPy's scipy.ndimage.shift (the old module path
is gone from current SciPy).  The criterion calls .cuda() on its class weights: torch.Tensor.cuda is the identity for
the run."""
import os
import sys

import numpy as np
import scipy
import scipy.ndimage
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import relaxloss_cases as K                       # noqa: E402
from ref_bootstrap import _mod, bootstrap         # noqa: E402


def reference_modules():
    cfg = bootstrap()
    tr = sys.modules["torchvision.transforms"]
    tr.Lambda = tr.Compose = None
    sk = _mod("skimage")
    sk.filters = _mod("skimage.filters", gaussian=None)
    sk.restoration = _mod("skimage.restoration", denoise_bilateral=None)
    sk.segmentation = _mod("skimage.segmentation", find_boundaries=None)
    try:
        import scipy.ndimage.interpolation  # noqa: F401
    except ImportError:
        _mod("scipy.ndimage.interpolation", shift=scipy.ndimage.shift)
    import transforms.transforms as T
    import loss.utils as U
    return cfg, T, U


def main():
    cfg, T, U = reference_modules()
    torch.set_num_threads(8)
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {"meta": {"scipy": scipy.__version__, "numpy": np.__version__, "torch": str(torch.__version__)}}
    for n in K.GOLDEN_CASES:
        k = K.CASES[n]
        cfg.DATASET.NUM_CLASSES = k["C"]
        cfg.BORDER_WINDOW = k["border"]
        cfg.STRICTBORDERCLASS = k["strict"]
        cfg.BATCH_WEIGHTING = k["batch"]
        cfg.REDUCE_BORDER_EPOCH = -1
        logits, labels = K.inputs(n)
        to_target = T.RelaxedBoundaryLossToTensor(k["ignore"], k["C"])
        target = torch.stack([to_target(labels[i].numpy().copy()) for i in range(labels.shape[0])])
        crit = U.ImgWtLossSoftNLL(classes=k["C"], ignore_index=k["ignore"], upper_bound=k["ub"])
        tnp = target.numpy()
        weights = torch.stack([torch.Tensor(crit.calculate_weights(tnp if k["batch"] else tnp[i]))
                               for i in range(tnp.shape[0])])
        lg = logits.clone().requires_grad_(True)
        loss = crit(lg, target.clone())
        (loss * k["up"]).backward()
        assert torch.isfinite(loss) and torch.isfinite(lg.grad).all(), n
        s, a = K.checksum(logits)
        out["case%d" % n] = {"labels": labels, "multihot": target, "weights": weights, "loss": loss.detach(),
                             "grad": lg.grad.clone(), "logits_sum": s, "logits_abs_sum": a}
        ign = int((target[:, :-1].sum(1) == 0).sum())
        print("case %d: loss %.6f  pixels without a class %d  widest set %d" % (
            n, float(loss.detach()), ign, int(target[:, :-1].sum(1).max())))
    torch.save(out, os.path.join(HERE, "relaxloss_golden.pt"))


if __name__ == "__main__":
    main()
