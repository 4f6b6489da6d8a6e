#!/usr/bin/env python
"""What dumping one validation image costs, per image at 1024 x 2048 with 19 classes, in ONE process on one GPU, for the
visual mode with assets (dump_assets: prob_mask, err_mask, pred_0.5x, attn_0.5x) and for the auto-labelling mode:

  (a) the reference's ImageDumper.dump as restated in tests/dump_ref.py, on the host arrays eval_minibatch returns today
      (int64 ndarrays, a CPU fp32 probability), without file writes
  (b) semseg_amd.utils.dumper.ImageDumper.dump on the device assets of eval_minibatch(assets_on_device=True) up to the
      bytes being on the host: the real method with Pillow's save stubbed out (the upload of nothing, the launches, the
      one trip back, colorize_mask on the host)
  (c) the floor of (b): the trip back alone -- `_to_host` of a device buffer of as many bytes as (b) brings back
  (d) the PNG writes alone, from arrays that are ready, into a temporary directory: what remains Pillow's encoder
      whichever path runs
  (e) the host formatting inside (b) alone: the Pillow objects the files are saved from, made from bytes that are ready
      (colorize_mask of the index maps, the RGB conversion of the L masks, fromarray of the rest)
  and the kernels of (b) alone by device events, next to a device-to-device copy that moves as many bytes as they read
  and write.

Paths alternate inside every round; every timed section starts after a synchronise and a short sleep and ends in one.
Writes the medians with their spread (half the range over the rounds) and the ratios (a)/(b), (b)/(c).  No threshold.

    python tools/dumpbench.py [--rounds 7] [--out profiles/dump_tail_bench.json]            needs a GPU"""
import argparse
import ctypes
import importlib
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "semantic-segmentation_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from PIL import Image  # noqa: E402

H, W, C = 1024, 2048, 19
MODES = {"visual_with_assets": dict(dump_assets=True), "auto_labelling": dict(dump_for_auto_labelling=True)}


def host_assets(rng):
    """One batch-1 dump_dict as the default eval_minibatch leaves it."""
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    u8 = rng.randint(0, 256, (1, 3, H, W)).astype(np.uint8)
    x = torch.from_numpy(u8).float().div(255).sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1))
    bs = 32                                            # blocky maps: what a PNG encoder meets in a segmentation
    blocks = rng.randint(0, C, (1, H // bs, W // bs))
    gts = np.repeat(np.repeat(blocks, bs, 1), bs, 2).astype(np.int64)
    pred = gts.copy()
    flip = rng.rand(1, H, W) < 0.05
    pred[flip] = rng.randint(0, C, int(flip.sum()))
    gts[rng.rand(1, H, W) < 0.1] = 255
    assets = {"pred_0.5x": np.ascontiguousarray(pred[:, ::2, ::2]),
              "attn_0.5x": torch.from_numpy(rng.rand(1, 1, H // 2, W // 2).astype(np.float32)),
              "predictions": pred, "prob_mask": torch.from_numpy(rng.rand(1, H, W).astype(np.float32)),
              "err_mask": ((pred != gts) & (gts != 255)).astype(int)}
    return {"input_images": x, "gt_images": torch.from_numpy(gts), "img_names": ["bench_000000"], "assets": assets}


def fresh(dd):
    return dict(dd, assets=dict(dd["assets"]))


def summary(ts):
    return {"median_ms": statistics.median(ts) * 1e3, "min_ms": min(ts) * 1e3, "max_ms": max(ts) * 1e3,
            "spread_ms": (max(ts) - min(ts)) * 0.5e3, "rounds_ms": [round(t * 1e3, 4) for t in ts]}


def timed(fn):
    torch.cuda.synchronize()
    time.sleep(0.1)
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def kernel_events(fn, reps=20):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dump_tail_bench.json"))
    a = ap.parse_args()
    assert a.rounds >= 5, "at least five rounds"
    if not torch.cuda.is_available():
        sys.exit("tools/dumpbench.py needs a GPU")
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    import dump_cases as K
    import dump_ref as R
    from semseg_amd import _lib
    from semseg_amd.config import cfg
    from semseg_amd.utils import dumper
    et = importlib.import_module("semseg_amd.utils.eval_tail")
    _, meta = R.load_golden()
    ds = R.golden_dataset(meta)
    cfg.DATASET_INST, cfg.GLOBAL_RANK = ds, 0
    mean, std = cfg.DATASET.MEAN, cfg.DATASET.STD
    dd_host = host_assets(np.random.RandomState(1))
    dd_dev = K.device_form(dd_host, "cuda")
    L = _lib.lib()
    result = {"device": torch.cuda.get_device_name(0), "image": [H, W], "classes": C, "rounds": a.rounds,
              "storage": _lib.ACT, "modes": {}}
    real_save = Image.Image.save
    for mode, kw in MODES.items():
        with tempfile.TemporaryDirectory() as tmp:
            cfg.RESULT_DIR = tmp
            d = dumper.ImageDumper(val_len=100, tensorboard=False, **kw)
            files = R.dump(fresh(dd_host), 0, ds, mean, std, **kw)
            trips = []
            real_to_host = et._to_host

            def spy(ts):
                trips.append(sum(t.numel() * t.element_size() for t in ts))
                return real_to_host(ts)

            def device_path():
                Image.Image.save = lambda self, *x, **k: None
                try:
                    d.dump(fresh(dd_dev), 0)
                finally:
                    Image.Image.save = real_save

            et._to_host = spy
            device_path()
            et._to_host = real_to_host
            back = trips[0]
            floor_buf = torch.empty((back,), dtype=torch.uint8, device="cuda")

            def write_files():
                for fn, e in files.items():
                    if e[0] == "P":
                        im = Image.fromarray(e[1]).convert("P")
                        im.putpalette(list(e[2]))
                    else:
                        im = Image.fromarray(e[1])
                    im.save(os.path.join(tmp, "w_" + fn))

            def format_files():
                for fn, e in files.items():
                    if e[0] == "P":
                        ds.colorize_mask(e[1])
                    elif e[1].ndim == 3 and ("_attn_" in fn or fn.endswith(("_prob_mask.png", "_err_mask.png"))):
                        Image.fromarray(np.ascontiguousarray(e[1][..., 0])).convert("RGB")
                    else:
                        Image.fromarray(e[1])

            paths = {"a_reference_host": lambda: R.dump(fresh(dd_host), 0, ds, mean, std, **kw),
                     "b_device_to_host_bytes": device_path,
                     "c_trip_back_alone": lambda: et._to_host([floor_buf]),
                     "d_png_writes_alone": write_files,
                     "e_host_formatting_alone": format_files}
            for fn in paths.values():                    # warm-up: allocator, pinned buffers, tables
                fn()
            times = {k: [] for k in paths}
            for _ in range(a.rounds):
                for k, fn in paths.items():
                    times[k].append(timed(fn))
            rec = {k: summary(v) for k, v in times.items()}
            rec["bytes_back"] = back
            rec["files"] = sorted(files)
            rec["a_over_b"] = rec["a_reference_host"]["median_ms"] / rec["b_device_to_host_bytes"]["median_ms"]
            rec["b_over_c"] = rec["b_device_to_host_bytes"]["median_ms"] / rec["c_trip_back_alone"]["median_ms"]
            rec["png_share_of_device_path_plus_writes"] = rec["d_png_writes_alone"]["median_ms"] / (
                rec["d_png_writes_alone"]["median_ms"] + rec["b_device_to_host_bytes"]["median_ms"])
            # the kernel of the mode alone, and a device copy of as many bytes
            n = H * W
            P = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())      # noqa: E731
            out = torch.empty((8 * n,), dtype=torch.uint8, device="cuda")
            pal, ids = d._device_tables(torch.device("cuda", torch.cuda.current_device()), ds)
            img, pred = dd_dev["assets"]["input_images"][0], dd_dev["assets"]["predictions"][0]
            prob, err = dd_dev["assets"]["prob_mask"][0], dd_dev["assets"]["err_mask"][0]
            if mode == "auto_labelling":
                rd, wr = n * (1 + 4), n * 2
                args = (None, 0, d.inv_mean, d.inv_std, None, P(pred), P(pal), P(ids), P(prob), None, 0.4, H, W, None,
                        None, None, None, P(out[:n]), P(out[n:2 * n]), None, None)
            else:
                rd, wr = n * (12 + 1 + 4 + 1), n * (3 + 3 + 1 + 1)
                args = (P(img), n, d.inv_mean, d.inv_std, None, P(pred), P(pal), P(ids), P(prob), P(err), 0.4, H, W,
                        P(out[:3 * n]), None, None, P(out[3 * n:6 * n]), None, P(out[6 * n:7 * n]), P(out[7 * n:]), None)

            def kern():
                assert L.ssa_dump_tail(*args) == 0

            src = torch.empty(((rd + wr) // 2,), dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            kern()
            dst.copy_(src)
            kt, ct = [], []
            for _ in range(a.rounds):
                kt.append(kernel_events(kern))
                ct.append(kernel_events(lambda: dst.copy_(src)))
            rec["kernel_alone"] = summary(kt)
            rec["device_copy_of_as_many_bytes"] = summary(ct)
            rec["kernel_bytes_read"], rec["kernel_bytes_written"] = rd, wr
            rec["kernel_bytes_per_s"] = (rd + wr) / statistics.median(kt)
            rec["device_copy_bytes_per_s"] = (rd + wr) / statistics.median(ct)
            rec["kernel_over_device_copy"] = statistics.median(kt) / statistics.median(ct)
            result["modes"][mode] = rec
            print(mode, json.dumps({k: (v["median_ms"] if isinstance(v, dict) else v) for k, v in rec.items()
                                    if k != "files"}, indent=1))
    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    print(json.dumps({"dumpbench": {m: {"a_ms": r["a_reference_host"]["median_ms"],
                                        "b_ms": r["b_device_to_host_bytes"]["median_ms"],
                                        "c_ms": r["c_trip_back_alone"]["median_ms"],
                                        "d_ms": r["d_png_writes_alone"]["median_ms"],
                                        "e_ms": r["e_host_formatting_alone"]["median_ms"], "a_over_b": r["a_over_b"],
                                        "b_over_c": r["b_over_c"], "kernel_ms": r["kernel_alone"]["median_ms"]}
                                    for m, r in result["modes"].items()}}))


if __name__ == "__main__":
    main()
