#!/usr/bin/env python
"""One training step of deepv3.DeepV3PlusW38 (scripts/train_cityscapes_deepv3.yml: 800 x 800 crop, cross entropy, SGD) on
the device: the reference's loop body through semseg_amd.graph_training (a replayed hipGraph), timed with a host clock
around a device synchronise.
    python tools/wrn38_step.py [--arch deepv3.DeepV3PlusW38] [--crop 800] [--batch 1] [--steps 10] [--warmup 3] [--eager] [--json FILE]
(tools/x71_step.py is this tool with --arch deepv3.DeepV3PlusX71 as the default.)
Storage format = library build: SSA_ACT_DTYPE=bf16 (default) | fp16 (with the dynamic loss scaler of semseg_amd.amp).
For the per-kernel table run it under the profiler in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/wrn38_step.py --steps 3 --eager"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402


def main(default_arch="deepv3.DeepV3PlusW38"):
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default=default_arch, help="a factory of semseg_amd.network (get_model)")
    ap.add_argument("--crop", type=int, default=800)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--eager", action="store_true", help="eager launches instead of the captured step")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the step tools need a GPU"
    import semseg_amd
    import __graft_entry__ as ge
    from semseg_amd import _lib, amp
    from semseg_amd.loss import CrossEntropyLoss2d
    from semseg_amd.loss.optimizer import FusedSGD
    from semseg_amd.network import get_model
    torch.manual_seed(0)
    net = get_model(a.arch, 19, CrossEntropyLoss2d(ignore_index=255)).cuda().train()
    optim = FusedSGD(net.parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
    net, optim = amp.initialize(net, optim)                 # the loss scaler on the fp16 build, nothing on bf16
    run, opt = (net, optim) if a.eager else semseg_amd.graph_training(net, optim)
    images, gts = ge._synth(a.batch, a.crop, a.crop, 40, "cuda")
    batch = {"images": images, "gts": gts}

    def step():
        opt.zero_grad()
        loss = run(batch).mean()
        with amp.scale_loss(loss, opt) as scaled:
            scaled.backward()
        opt.step()
        return loss
    for _ in range(a.warmup):
        loss = step()
    torch.cuda.synchronize()
    times = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        loss = step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    rec = {"arch": a.arch, "crop": a.crop, "batch": a.batch, "dtype": _lib.ACT, "graph": not a.eager,
           "steps": a.steps, "step_ms_median": round(times[len(times) // 2], 3), "step_ms_min": round(times[0], 3),
           "step_ms_max": round(times[-1], 3), "loss": round(float(loss.detach()), 5), "lib_sha": _lib.built_sha(),
           "peak_memory_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
    print(json.dumps(rec))
    if a.json:
        with open(a.json, "a") as f:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
