#!/usr/bin/env python
"""Grouped 3x3 conv (csrc/gconv.hip) and the SE gate passes (csrc/se.hip) at the shapes of DeepV3PlusSRNX50 at an
800 x 800 crop, batch 1, in ONE call:
    python tools/gconvbench.py [reps] [--rounds N] [--json profiles/gconv_bench.json]
Per grouped shape, timed ALTERNATELY round by round with device events around `reps` eager launches (medians):
  ours            ssa_gconv3x3 with the BatchNorm sums (the training form); ssa_gconv3x3_bwd for dx alone, dw alone and both;
  dense           the route of the parent commit: the weight copied onto the block diagonal of a dense [C,C,3,3] filter
                  (BackendBase._block_diagonal) through the implicit-GEMM conv of HipBackend -- forward under no_grad, and
                  forward + backward through autograd (scatter, pack, data gradient, dense weight gradient and its
                  gather), so backward = the difference;  ours_step is GConv3x3Fn forward + backward the same way;
  torch           F.conv2d(groups = G) on 16-bit channels_last tensors / aten.convolution_backward (reported, or the error);
  copy            Tensor.copy_ of the bytes the algorithm must move: forward reads x and writes y.
`take_gconv` = ours_step <= dense_step: the ship rule of HipBackend.GCONV_ROUTE.  The SE passes (SeGateFn forward and
backward) are timed beside their composition on the device (BackendBase.se_gate_add_act on HipBackend: global average pool,
two 1x1 convs with bias, ReLU, sigmoid, then torch's multiply-add and ReLU; its error, if it does not run, is recorded)
and beside a copy of the bytes they must move (forward: y, r read, z written, y read once more for the squeeze; backward:
dz, z, y read and dz, z read again, dy, dr written).  B below is the HIP backend.  Needs a GPU."""
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from semseg_amd import _lib, ops, hip_backend as hb  # noqa: E402

# (H, W, C, stride, dil), 32 groups, B = 1: the five (C, stride, dil) of the trunk at the resolution each occurs at
SHAPES = [(200, 200, 128, 1, 1), (200, 200, 256, 2, 1), (100, 100, 256, 1, 1), (100, 100, 512, 1, 2), (100, 100, 1024, 1, 4)]
SE_SHAPES = [(200, 200, 256), (100, 100, 512), (100, 100, 1024), (100, 100, 2048)]
G = 32


def _opt(name, dflt=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else dflt


def timed_us(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def measure(runs, reps, rounds):
    for fn in runs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            t[k].append(timed_us(fn, reps))
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in t.items()}


def gconv_shape(H, W, C, s, d, seed, reps, rounds):
    g = torch.Generator().manual_seed(seed)
    L = hb.lib()
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x = torch.randn((1, H, W, C), generator=g).to(hb.ACT_DTYPE).cuda()
    dy = torch.randn((1, Ho, Wo, C), generator=g).to(hb.ACT_DTYPE).cuda()
    w = torch.nn.Parameter((torch.randn((C, C // G, 3, 3), generator=g) * 0.1).cuda())
    y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.zeros_like(w.data)
    stats = torch.zeros(hb.stat_replicas() * 2 * C, dtype=torch.float64, device="cuda")
    desc = _lib.GConvDesc(1, H, W, C, G, C, Ho, Wo, C, s, d)
    n = ctypes.c_size_t(0)
    hb.check(L.ssa_gconv3x3_bwd_plan(ctypes.byref(desc), ctypes.byref(n)), "ssa_gconv3x3_bwd_plan")
    ws = torch.empty(n.value // 4, dtype=torch.float32, device="cuda")
    xt, dyt, wt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), w.detach().to(hb.ACT_DTYPE)
    nbytes = 2.0 * C * (H * W + Ho * Wo)
    cp = [torch.empty(int(nbytes) // 4, dtype=hb.ACT_DTYPE, device="cuda") for _ in range(2)]

    def bwd(want_dx, want_dw):
        hb.check(L.ssa_gconv3x3_bwd(ctypes.byref(desc), hb._p(x), hb._p(dy), C, hb._p(w.data), hb._p(dx) if want_dx else None, C,
                                    hb._p(dw) if want_dw else None, 0, hb._p(ws), hb._s()), "ssa_gconv3x3_bwd")

    def step(route):
        xr = x.detach().requires_grad_(True)
        B.begin_step(x.device)
        z = route(xr)
        B.end_forward()
        z.backward(dy)
        w.grad = None

    def dense(xr):          # HipBackend.grouped_conv's dense route as it ships (the filter kept out of the pack cache)
        return ops.HipBackend.conv2d(B, xr, B._block_diagonal(w, G, padded=True), None, s, d, d, want_stats=True)

    def dense_fwd():
        with torch.no_grad():
            B.begin_step(x.device)
            dense(x)

    runs = {
        "ours_fwd": lambda: hb.check(L.ssa_gconv3x3(ctypes.byref(desc), hb._p(x), hb._p(w.data), hb._p(y), hb._p(stats), hb._s()),
                                     "ssa_gconv3x3"),
        "ours_dx": lambda: bwd(True, False), "ours_dw": lambda: bwd(False, True), "ours_bwd": lambda: bwd(True, True),
        "ours_step": lambda: step(lambda xr: hb.GConv3x3Fn.apply(xr, w, s, d, G, True)),
        "dense_fwd": dense_fwd,
        "dense_step": lambda: step(dense),
        "copy": lambda: cp[1].copy_(cp[0]),
    }
    torch_err = None
    try:
        torch.nn.functional.conv2d(xt, wt, None, s, d, d, G)
        torch.ops.aten.convolution_backward(dyt, xt, wt, None, [s] * 2, [d] * 2, [d] * 2, False, [0, 0], G, [True, True, False])
        torch.cuda.synchronize()
        runs["torch_fwd"] = lambda: torch.nn.functional.conv2d(xt, wt, None, s, d, d, G)
        runs["torch_bwd"] = lambda: torch.ops.aten.convolution_backward(dyt, xt, wt, None, [s] * 2, [d] * 2, [d] * 2, False,
                                                                         [0, 0], G, [True, True, False])
    except Exception as e:                      # noqa: BLE001 -- a form this torch build does not offer on this device
        torch_err = "%s: %s" % (type(e).__name__, str(e)[:200])
    us = measure(runs, reps, rounds)
    m = {k: v["median"] for k, v in us.items()}
    rec = {"op": "gconv3x3", "shape": [1, H, W, C], "groups": G, "stride": s, "dil": d, "dtype": str(hb.ACT_DTYPE).replace("torch.", ""),
           "reps": reps, "rounds": rounds, "lib_sha": _lib.built_sha(), "fwd_bytes": nbytes, "us": us, "torch_error": torch_err,
           "dense_bwd_us": round(m["dense_step"] - m["dense_fwd"], 2), "fwd_fraction_of_copy_rate": round(m["copy"] / m["ours_fwd"], 3),
           "ours_fwd_over_dense_fwd": round(m["ours_fwd"] / m["dense_fwd"], 4), "ours_step_over_dense_step": round(m["ours_step"] / m["dense_step"], 4),
           "take_gconv": bool(m["ours_step"] <= m["dense_step"])}
    print("%-14s s%d d%d  ours fwd %7.1f dx %7.1f dw %7.1f step %8.1f | dense fwd %8.1f step %8.1f | torch fwd %8s bwd %8s | copy %6.1f  %s" % (
        "x".join(map(str, (H, W, C))), s, d, m["ours_fwd"], m["ours_dx"], m["ours_dw"], m["ours_step"], m["dense_fwd"], m["dense_step"],
        m.get("torch_fwd", "n/a"), m.get("torch_bwd", "n/a"), m["copy"], "GCONV" if rec["take_gconv"] else "DENSE"))
    return rec


def se_shape(H, W, C, seed, reps, rounds):
    from semseg_amd.network.seresnext import SEModule
    g = torch.Generator().manual_seed(seed)
    y = torch.randn((1, H, W, C), generator=g).to(hb.ACT_DTYPE).cuda()
    r = torch.randn((1, H, W, C), generator=g).to(hb.ACT_DTYPE).cuda()
    dz = torch.randn((1, H, W, C), generator=g).to(hb.ACT_DTYPE).cuda()
    se = SEModule(C, 16).cuda()
    n = H * W * C
    cf = [torch.empty(n * 2, dtype=hb.ACT_DTYPE, device="cuda") for _ in range(2)]       # 4 tensors moved: a copy of 2
    cb = [torch.empty(n * 7 // 2, dtype=hb.ACT_DTYPE, device="cuda") for _ in range(2)]  # 7 tensors moved

    def fwd():
        with torch.no_grad():
            B.se_gate_add_act(se, y, r, relu=True)

    def step(gate=None):
        yr, rr = y.detach().requires_grad_(True), r.detach().requires_grad_(True)
        B.begin_step(y.device)
        z = (gate or B.se_gate_add_act)(se, yr, rr, relu=True)
        B.end_forward()
        z.backward(dz)
        for p in se.parameters():
            p.grad = None

    def composed(se_, y_, r_, relu=True):
        return ops.BackendBase.se_gate_add_act(B, se_, y_, r_, relu=relu)

    def comp_fwd():
        with torch.no_grad():
            B.begin_step(y.device)
            composed(se, y, r)
    runs = {"se_fwd": fwd, "se_step": step, "copy_fwd": lambda: cf[1].copy_(cf[0]), "copy_bwd": lambda: cb[1].copy_(cb[0])}
    comp_err = None
    try:
        comp_fwd()
        step(composed)
        torch.cuda.synchronize()
        runs["composition_fwd"], runs["composition_step"] = comp_fwd, lambda: step(composed)
    except Exception as e:                      # noqa: BLE001 -- reported, not hidden
        comp_err = "%s: %s" % (type(e).__name__, str(e)[:200])
    us = measure(runs, reps, rounds)
    m = {k: v["median"] for k, v in us.items()}
    rec = {"op": "se_gate_add_act", "shape": [1, H, W, C], "dtype": str(hb.ACT_DTYPE).replace("torch.", ""), "reps": reps,
           "rounds": rounds, "lib_sha": _lib.built_sha(), "us": us, "se_bwd_us": round(m["se_step"] - m["se_fwd"], 2),
           "composition_error": comp_err,
           "composition_bwd_us": round(m["composition_step"] - m["composition_fwd"], 2) if comp_err is None else None,
           "fwd_fraction_of_copy_rate": round(m["copy_fwd"] / m["se_fwd"], 3),
           "bwd_fraction_of_copy_rate": round(m["copy_bwd"] / max(m["se_step"] - m["se_fwd"], 1e-9), 3)}
    print("se %-14s fwd %7.1f us (composition %8s, copy %6.1f)  bwd %7.1f us (composition %8s, copy %6.1f)" % (
        "x".join(map(str, (H, W, C))), m["se_fwd"], m.get("composition_fwd", "n/a"), m["copy_fwd"], rec["se_bwd_us"],
        rec["composition_bwd_us"] if comp_err is None else "n/a", m["copy_bwd"]))
    return rec


def main():
    global B
    assert torch.cuda.is_available(), "gconvbench needs a GPU"
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    rounds = int(_opt("--rounds", "5"))
    out = _opt("--json")
    B = ops.backend()
    results = []
    for i, (H, W, C, s, d) in enumerate(SHAPES):
        results.append(gconv_shape(H, W, C, s, d, 60 + i, reps, rounds))
        torch.cuda.empty_cache()
    for i, (H, W, C) in enumerate(SE_SHAPES):
        results.append(se_shape(H, W, C, 70 + i, reps, rounds))
        torch.cuda.empty_cache()
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
