"""Generate tests/golden/evaltail_golden.pt from the REAL reference's evaluation tail.

Run in the build container (where the reference checkout exists):
    python tests/golden/make_golden_evaltail.py
utils/trnval_utils.eval_minibatch (with utils/misc.fast_hist and loss/utils.CrossEntropyLoss2d behind it) runs on the CPU
-- `Tensor.cuda` is made the identity and `torch.cuda.empty_cache` a no-op, as tests/ref_train_driver.py does -- on the
seeded batches and stub networks of tests/evaltail_ref.py (`CASES` below, repeated by tests/test_eval_tail_cpu.py).
Stored per case: only results -- the asset keys in order, predictions / pred_* / error mask as uint8, the histogram,
prob_mask, val_loss.avg; the inputs are regenerated from the seeds."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from ref_bootstrap import bootstrap  # noqa: E402
import evaltail_ref as R  # noqa: E402

# name: (classes, ignore label, cfg.MODEL.MSCALE, stub, batch (B, H, W, seed), args)
CASES = {
    "mscale19": (19, 255, True, ("MscaleStub", 3), (1, 24, 40, 19), dict(do_flip=True)),
    "mscale65": (65, 65, True, ("MscaleStub", 3), (2, 24, 40, 65), dict(do_flip=True)),
    "multi19": (19, 255, False, ("SeededStub", 100), (1, 24, 40, 21),
                dict(multi_scale_inference=True, extra_scales="0.5,2.0", do_flip=True)),
    "plain19": (19, 255, False, ("SeededStub", 7), (1, 24, 40, 22), dict()),
}


def build_case(name):
    C, ignore, mscale, (stub, seed), (B, H, W, bseed), kw = CASES[name]
    return C, ignore, mscale, getattr(R, stub)(C, seed), R.make_batch(B, H, W, C, ignore, seed=bseed), R.Args(**kw)


def main():
    cfg = bootstrap(19)
    torch.set_num_threads(8)
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.cuda.empty_cache = lambda: None
    from utils.trnval_utils import eval_minibatch
    from loss.utils import CrossEntropyLoss2d
    out = {}
    for name in CASES:
        C, ignore, mscale, net, data, args = build_case(name)
        cfg.DATASET.NUM_CLASSES, cfg.DATASET.IGNORE_LABEL, cfg.MODEL.MSCALE = C, ignore, mscale
        meter = R.Meter()
        assets, hist = eval_minibatch(data, net, CrossEntropyLoss2d(ignore_index=ignore), meter, True, args, 1)
        rec = {"keys": list(assets.keys()), "hist": torch.from_numpy(hist).long(), "loss": float(meter.avg),
               "count": int(meter.count), "prob_mask": assets["prob_mask"].clone()}
        for k, v in assets.items():
            if k == "prob_mask":
                continue
            if "attn_" in k:
                rec[k + ".shape"] = tuple(v.shape)
                continue
            assert v.dtype.kind == "i" and v.min() >= 0 and v.max() < 256
            rec[k] = torch.from_numpy(v.astype("uint8"))
        out[name] = rec
    torch.save(out, os.path.join(HERE, "evaltail_golden.pt"))
    print({k: v["keys"] for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "evaltail_golden.pt")))


if __name__ == "__main__":
    main()
