#!/usr/bin/env python
"""Micro-benchmark of the bilinear resize kernels at the shapes of a 1024 x 1024 HRNet-OCR-MScale training step (1.0x
pass), align_corners off against on, through the ssa_resize_* entry points of the C ABI; each launch sequence replayed
`reps` times from a hipGraph.  Informational: no threshold -- under align_corners=True an input pixel receives from
5-6 / 9-10 / 17 outputs per axis at 2x / 4x / 8x (4 / 8 / 16 under the other rule), so its backward costs more.
    python tools/resizebench.py [reps]        writes profiles/resize_ac_bench.json"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from semseg_amd import hip_backend as hb  # noqa: E402

L = hb.lib()
P = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
A = hb.ACT_DTYPE

# (what, C, Hi, Wi, Ho, Wo, 16-bit): the fuse layers' branch upsamples, the head's concat, the logits and attention maps
SHAPES = [("fuse 2x", 48, 128, 128, 256, 256, True), ("fuse 4x", 48, 64, 64, 256, 256, True), ("fuse 8x", 48, 32, 32, 256, 256, True),
          ("fuse 2x", 96, 64, 64, 128, 128, True), ("fuse 4x", 96, 32, 32, 128, 128, True),
          ("head 2x", 96, 128, 128, 256, 256, True), ("head 4x", 192, 64, 64, 256, 256, True), ("head 8x", 384, 32, 32, 256, 256, True),
          ("logits 4x", 19, 256, 256, 1024, 1024, False), ("logits 0.5x pass 4x", 19, 128, 128, 512, 512, False),
          ("logits 2x", 19, 512, 512, 1024, 1024, False), ("attention 2x", 1, 512, 512, 1024, 1024, False)]


def timed(stream, run):
    with torch.cuda.stream(stream):
        run()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for _ in range(reps):
                run()
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        g.replay()
        e1.record(stream)
        torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000 / reps


rows = []
for what, C, hi, wi, ho, wo, is16 in SHAPES:
    dt, code = (A, 0) if is16 else (torch.float32, 1)
    x = torch.randn(1, hi, wi, C, device="cuda").to(dt)
    y = torch.empty(1, ho, wo, C, device="cuda", dtype=dt)
    dy = torch.randn(1, ho, wo, C, device="cuda").to(dt)
    dx = torch.empty(1, hi, wi, C, device="cuda", dtype=dt)
    tmp = torch.empty(1, ho, wi, C, device="cuda", dtype=torch.float32)
    s = torch.cuda.Stream()
    sp = ctypes.c_void_p(s.cuda_stream)
    row = {"what": what, "C": C, "in": [hi, wi], "out": [ho, wo], "dtype": "16-bit" if is16 else "fp32"}
    for ac in (0, 1):
        us = {"fwd": timed(s, lambda: hb.check(L.ssa_resize_bilinear_fwd(P(x), code, 1, hi, wi, C, C, P(y), code, ho, wo, C, ac, sp), "fwd")),
              "bwd": timed(s, lambda: hb.check(L.ssa_resize_bilinear_bwd(P(dy), code, 1, ho, wo, C, C, P(dx), code, hi, wi, C, ac, sp), "bwd"))}
        if is16:        # the route the glue takes for these: pass X, then pass Y
            def pair():
                hb.check(L.ssa_resize_bilinear_bwd_x(P(dy), code, 1, ho, wo, C, C, P(tmp), wi, ac, sp), "bwd_x")
                hb.check(L.ssa_resize_bilinear_bwd_y(P(tmp), 1, ho, wi, C, P(dx), code, hi, C, ac, sp), "bwd_y")
            us["bwd_x+y"] = timed(s, pair)
        row["us_align_corners_%d" % ac] = {k: round(v, 2) for k, v in us.items()}
    rows.append(row)
    print("%-20s C=%3d %4dx%-4d -> %4dx%-4d %s" % (what, C, hi, wi, ho, wo, "  ".join(
        "%s %.1f -> %.1f us" % (k, row["us_align_corners_0"][k], row["us_align_corners_1"][k]) for k in row["us_align_corners_0"])))
img = torch.randn(1, 3, 1024, 1024, device="cuda")
out = torch.empty(1, 512, 512, 16, device="cuda", dtype=A)
s = torch.cuda.Stream()
sp = ctypes.c_void_p(s.cuda_stream)
row = {"what": "image 0.5x to NHWC", "C": 3, "in": [1024, 1024], "out": [512, 512], "dtype": "fp32 -> 16-bit"}
for ac in (0, 1):
    row["us_align_corners_%d" % ac] = {"fwd": round(timed(s, lambda: hb.check(
        L.ssa_image_resize_to_nhwc(P(img), 1, 3, 1024, 1024, P(out), 512, 512, 16, ac, sp), "image")), 2)}
rows.append(row)
print("%-20s fwd %.1f -> %.1f us" % (row["what"], row["us_align_corners_0"]["fwd"], row["us_align_corners_1"]["fwd"]))
dst = os.path.join(ROOT, os.environ.get("SSA_RESIZEBENCH_OUT", os.path.join("profiles", "resize_ac_bench.json")))
with open(dst, "w") as f:
    json.dump({"device": torch.cuda.get_device_name(0), "storage": str(A), "reps": reps, "unit": "us per launch sequence",
               "rows": rows}, f, indent=1)
    f.write("\n")
print("wrote", dst)
