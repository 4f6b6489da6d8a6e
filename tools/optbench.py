#!/usr/bin/env python
"""What one optimizer step over the parameter list of HRNet-OCR-MScale costs, in ONE process on one GPU:

  FusedSGD(momentum=0.9)      ssa_sgd_momentum_step                 20 B per parameter (read p, g, buf; write p, buf)
  FusedAdam                   ssa_adam_advance + ssa_adam_step      28 B (read p, g, m, v; write p, m, v)
  FusedAdam(amsgrad=True)                                           36 B (+ vmax read and written)
  FusedRAdam                                                        28 B
  torch.optim.Adam(foreach=True), torch.optim.Adam(fused=True)      for context, if the installed torch offers them here

The parameters are the shapes of the real network (72.1 M elements in well over a thousand tensors, many of them a
few dozen elements) with random values; all candidates share the parameter and gradient tensors and own their state.
The candidates alternate inside every round; a timed window runs whole steps for at least --window seconds (default
0.5) after warm-up and is closed by a device synchronise.  Two figures per fused candidate: `ms` is the eager step as
a training loop without graphs issues it (host glue included), `graph_ms` the same step replayed from a captured
graph, which is how the product's training step runs it (semseg_amd/graphed.py).  Reported per candidate: the median
over the rounds with half the range as spread, kernel launches per step, the algorithmic GB/s (bytes above / time)
and its ratio to FusedSGD's in the same run.  Writes --out (default profiles/optim_bench.json).

    python tools/optbench.py [--rounds 5] [--window 0.5] [--out FILE]                       needs a GPU"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402


def parameter_shapes():
    from semseg_amd.loss import RMILoss
    from semseg_amd.network import ocrnet
    net = ocrnet.HRNet_Mscale(19, RMILoss(num_classes=19, ignore_index=255))
    return [tuple(p.shape) for p in net.parameters()]


def window(fn, seconds):
    """Whole calls of fn for at least `seconds`, closed by a synchronise: seconds per call."""
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if time.perf_counter() - t0 >= seconds:
            break
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "optbench needs a GPU"
    from semseg_amd._lib import lib
    from semseg_amd.loss.optimizer import FusedAdam, FusedRAdam, FusedSGD
    shapes = parameter_shapes()
    g = torch.Generator().manual_seed(0)
    params = [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).cuda() * 1e-2
    numel = sum(p.numel() for p in params)
    lr, wd = 1e-6, 1e-4                       # (small: thousands of steps on the same gradients must stay finite)
    cands = [("FusedSGD", 20, lambda: FusedSGD(params, lr=lr, momentum=0.9, weight_decay=wd)),
             ("FusedAdam", 28, lambda: FusedAdam(params, lr=lr, weight_decay=wd)),
             ("FusedAdam_amsgrad", 36, lambda: FusedAdam(params, lr=lr, weight_decay=wd, amsgrad=True)),
             ("FusedRAdam", 28, lambda: FusedRAdam(params, lr=lr, weight_decay=wd))]
    for name, kw in (("torch_Adam_foreach", dict(foreach=True)), ("torch_Adam_fused", dict(fused=True))):
        cands.append((name, 28, lambda kw=kw: torch.optim.Adam(params, lr=lr, weight_decay=wd, **kw)))
    runs = []
    for name, bpe, make in cands:
        try:
            opt = make()
            for _ in range(3):                # warm-up: state tensors, allocator
                opt.step()
            torch.cuda.synchronize()
        except Exception as e:                # noqa: BLE001 -- a torch variant this build does not offer on this device
            print("%s: not available here (%s: %s)" % (name, type(e).__name__, str(e)[:120]))
            continue
        run = {"name": name, "bytes_per_element": bpe, "opt": opt, "eager": [], "graph": [], "launches": None, "replay": None}
        if name.startswith("Fused"):
            lib().ssa_launch_count(1)
            opt.step()
            run["launches"] = int(lib().ssa_launch_count(1))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                opt.step()
            run["replay"] = graph.replay
        runs.append(run)
    for _ in range(args.rounds):
        for run in runs:
            run["eager"].append(window(run["opt"].step, args.window))
            if run["replay"] is not None:
                run["graph"].append(window(run["replay"], args.window))
    assert all(bool(torch.isfinite(p).all()) for p in params[:8])
    out = {"device": torch.cuda.get_device_name(0), "tensors": len(params), "elements": numel, "rounds": args.rounds,
           "window_s": args.window, "candidates": {}}
    for run in runs:
        ent = {"bytes_per_element": run["bytes_per_element"], "launches_per_step": run["launches"]}
        for key, label in (("eager", "ms"), ("graph", "graph_ms")):
            ts = run[key]
            if not ts:
                continue
            med = statistics.median(ts)
            ent[label] = med * 1e3
            ent[label + "_spread"] = (max(ts) - min(ts)) / 2 * 1e3
            ent[label.replace("ms", "GBps")] = run["bytes_per_element"] * numel / med / 1e9
        out["candidates"][run["name"]] = ent
    sgd = out["candidates"].get("FusedSGD")
    for name, ent in out["candidates"].items():
        for key in ("GBps", "graph_GBps"):
            if sgd and key in ent and key in sgd:
                ent[key + "_vs_FusedSGD"] = ent[key] / sgd[key]
        print("%-20s %s" % (name, "  ".join("%s %.4g" % (k, v) for k, v in ent.items() if isinstance(v, float))
                            + "  launches %s" % ent["launches_per_step"]))
    fused = [n for n in out["candidates"] if n.startswith("Fused") and n != "FusedSGD"]
    out["done"] = {n: {k: out["candidates"][n].get(k + "_vs_FusedSGD", 0.0) >= 0.9 for k in ("GBps", "graph_GBps")}
                   for n in fused}
    print("at least 0.9 x FusedSGD's algorithmic bandwidth:", out["done"])
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
