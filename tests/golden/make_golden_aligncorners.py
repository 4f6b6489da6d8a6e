"""Golden fixture for --align_corners (cfg.MODEL.ALIGN_CORNERS = True; config.py:127,293) generated from the REAL reference's
ocrnet.HRNet_Mscale.  Run in the build container:
    python tests/golden/make_golden_aligncorners.py
Writes aligncorners_golden.pt: the train loss, sampled parameter gradients plus norms, BN running-stat samples, and
sub-sampled eval outputs (two-scale and the 0.5 / 1.0 / 2.0 chain) on BN statistics calibrated on the batch, with samples
of those calibrated statistics (the full set is 2 MB; tests/test_align_corners_cpu.py has the oracle calibrate itself and
checks it against the samples).  Weights, batch and sampling are make_golden.py's, so that the fixture differs from
mscale_golden.pt by the flag alone; the samples are packed (pack / unpack below) to stay far below 1 MiB.

The flag is set BEFORE any `network.*` import: network/mynn.py:15 and network/hrnetv2.py:27 copy it into a module global
at import -- set later it would reach only network/ocr_utils.py:117 and utils/trnval_utils.py:54,
which read cfg when called."""
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


def pack(d):
    """{name: 1-D tensor} as (names, lengths, one float64 tensor): 3,000 small tensors pickle to 1.6 MB, packed to 0.6 MB.
    A gradient entry is [16 sample indices | 16 values | the norm] (indices are exact in float64)."""
    return {"names": list(d), "lengths": [int(v.numel()) for v in d.values()], "data": torch.cat([v.double().flatten() for v in d.values()])}


def unpack(p):
    out, off = {}, 0
    for k, n in zip(p["names"], p["lengths"]):
        out[k] = p["data"][off:off + n]
        off += n
    return out


def unpack_grads(p):
    """-> {name: (idx int64, values fp32, norm fp32)} as make_golden.py stores them."""
    out = {}
    for k, v in unpack(p).items():
        n = (v.numel() - 1) // 2
        out[k] = (v[:n].long(), v[n:2 * n].float(), v[2 * n].float())
    return out


def main():
    cfg = bootstrap(19)
    assert not any(m == "network" or m.startswith("network.") for m in sys.modules), "network.* imported before the flag is set"
    cfg.MODEL.ALIGN_CORNERS = True
    cfg.LOSS.SUPERVISED_MSCALE_WT = 0.05
    torch.manual_seed(0)
    torch.set_num_threads(8)
    from loss.rmi import RMILoss
    import network.mynn as mynn
    import network.hrnetv2 as hrnetv2
    import network.ocrnet as ocrnet
    assert mynn.align_corners is True and hrnetv2.align_corners is True

    net = ocrnet.HRNet_Mscale(19, RMILoss(num_classes=19, ignore_index=255))
    shapes = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    with open(os.path.join(HERE, "keys.txt")) as f:
        assert [line.split(" ")[0] for line in f] == [k for k, _ in shapes], "not the network of keys.txt"
    sd = seeded_state_dict(shapes, seed=0)
    net.load_state_dict(sd)
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.p = 0.0   # parity hygiene
    images, gts = synth_batch(1, 128, 128, seed=1234)
    gold = {"seed": 0, "batch": (1, 128, 128, 1234), "align_corners": True}      # (the batch is regenerated from its seed)
    net.train()
    loss = net({"images": images, "gts": gts})
    loss.backward()
    gold["train_loss"] = loss.detach()
    grads = {}
    for name, p in net.named_parameters():
        flat = p.grad.flatten()
        idx = sample_idx(flat.numel())
        grads[name] = (idx, flat[idx].clone(), flat.norm().clone())
    gold["grads"] = pack({k: torch.cat([i.double(), v.double(), n.double().view(1)]) for k, (i, v, n) in grads.items()})
    gold["running_sample"] = pack({k: v.flatten()[:4].clone() for k, v in net.state_dict().items()
                                   if k.endswith("running_mean") or k.endswith("running_var")})
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
    gold["calib_sample"] = pack({k: v.flatten()[:4].clone() for k, v in net.state_dict().items()
                                 if k.endswith("running_mean") or k.endswith("running_var")})
    net.eval()
    with torch.no_grad():
        o = net({"images": images, "gts": gts})
        gold["eval"] = {k: v[:, :, ::8, ::8].clone() for k, v in o.items()}
        cfg.MODEL.N_SCALES = [0.5, 1.0, 2.0]
        o = net({"images": images, "gts": gts})
        gold["eval_nscale"] = {k: v[:, :, ::8, ::8].clone() for k, v in o.items()}
        cfg.MODEL.N_SCALES = None
    out = os.path.join(HERE, "aligncorners_golden.pt")
    torch.save(gold, out)
    assert os.path.getsize(out) < 1 << 20, os.path.getsize(out)
    print("train_loss", float(gold["train_loss"]), "keys", len(shapes), "bytes", os.path.getsize(out))


if __name__ == "__main__":
    main()
