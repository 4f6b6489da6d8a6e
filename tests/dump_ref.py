"""ImageDumper.dump (utils/misc.py:279-386) restated in NumPy, Pillow and torch: what every file of a dump holds, without
writing one.  `dump()` returns {file name relative to save_dir: (mode, array)} -- for a P file (mode, indices, palette).

The lines of arithmetic, each checked against the live library it restates by tests/test_dump_cpu.py:
  denorm_bytes   Normalize(inv_mean, inv_std) (sub_, div_) then ToPILImage (mul(255).byte()): three fp32 operations
  blend_bytes    Image.blend: a + alpha * (b - a), each operation rounded to fp32, truncated toward zero
  mask_bytes     (mask * 255).astype(np.uint8) of an fp32 mask
  u8_trunc       the cast itself: truncation toward zero; outside [0, 256) (undefined in the reference) it saturates and
                 NaN gives 0 -- the rule the kernels of csrc/dump_tail.hip follow
  palette_table  colorize_mask(arange(256)).convert('RGB'): Pillow's own answer for any palette length
  id_table       the loop of misc.py:321-322 over the indices 0..255 as one table
"""
import io
import json
import os

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dump_golden.npz")
ALPHA = 0.4                                        # misc.py:342


def u8_trunc(v):
    v = np.asarray(v, np.float32)
    return np.clip(np.where(np.isnan(v), np.float32(0), v), np.float32(0), np.float32(255)).astype(np.uint8)


def inv_norm(mean, std):
    """The fp32 values torchvision's Normalize forms from the reference's Python lists (misc.py:240-242)."""
    inv_mean = np.array([-m / s for m, s in zip(mean, std)], dtype=np.float32)
    inv_std = np.array([1 / s for s in std], dtype=np.float32)
    return inv_mean, inv_std


def denorm_bytes(x, inv_mean, inv_std):
    """x fp32 [3][H][W] -> uint8 [H][W][3]"""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):                # (an overflow to infinity saturates like any other large value)
        t = (x - inv_mean.reshape(3, 1, 1)).astype(np.float32)
        t = (t / inv_std.reshape(3, 1, 1)).astype(np.float32)
        return np.ascontiguousarray(u8_trunc(t * np.float32(255)).transpose(1, 2, 0))


def blend_bytes(a, b, alpha=ALPHA):
    fa, fb = a.astype(np.float32), b.astype(np.float32)
    d = (fb - fa).astype(np.float32)
    return u8_trunc(fa + (np.float32(alpha) * d).astype(np.float32))


def mask_bytes(m):
    with np.errstate(all="ignore"):
        return u8_trunc(np.asarray(m, np.float32) * np.float32(255))


def err_bytes(e):
    return (np.asarray(e).astype(np.int64) * 255).astype(np.uint8)


def palette_table(colorize_mask):
    pil = colorize_mask(np.arange(256, dtype=np.uint8).reshape(1, 256))
    return np.ascontiguousarray(np.array(pil.convert("RGB"))[0])


def id_table(id_to_trainid):
    lut = np.zeros(256, np.int64)
    for label_id, train_id in id_to_trainid.items():
        if 0 <= train_id <= 255:
            lut[train_id] = label_id
    return np.clip(lut, 0, 255).astype(np.uint8)


class Dataset:
    """What ImageDumper reads of cfg.DATASET_INST: colorize_mask (datasets/base_loader.py:94-100) and id_to_trainid."""

    def __init__(self, color_mapping, id_to_trainid):
        self.color_mapping = list(color_mapping)
        self.id_to_trainid = dict(id_to_trainid)

    def colorize_mask(self, image_array):
        new_mask = Image.fromarray(image_array.astype(np.uint8)).convert("P")
        new_mask.putpalette(self.color_mapping)
        return new_mask


def _p_entry(pil):
    pal = np.array(pil.getpalette(), dtype=np.uint8)
    return ("P", np.array(pil), np.concatenate([pal, np.zeros(768 - pal.size, np.uint8)]))


def decode(path_or_bytes):
    """A written file as dump() describes it."""
    pil = Image.open(io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else path_or_bytes)
    pil.load()
    if pil.mode == "P":
        return _p_entry(pil)
    return (pil.mode, np.array(pil))


def same(a, b):
    return len(a) == len(b) and a[0] == b[0] and all(
        x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def dumps(val_idx, val_len, dump_all_images=False, dump_num=10, global_rank=0, labelling=False):
    """misc.py:234-238, 293-298, 347-349: (files are written, the image reaches the web page)"""
    viz = max(1, val_len // dump_num)
    freq = 1 if dump_all_images else viz
    if labelling:
        return True, False
    if val_idx % freq or global_rank != 0:
        return False, False
    return True, not (val_idx % viz or global_rank != 0)


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def dump(dump_dict, val_idx, dataset, mean, std, val_len=100, dump_all_images=False, dump_assets=False, dump_num=10,
         dump_for_auto_labelling=False, dump_for_submission=False, global_rank=0):
    """{file name: entry} of one ImageDumper.dump call with the reference's host assets (utils/trnval_utils.py:
    187-196: int64 ndarrays, a CPU fp32 prob_mask, attn_* tensors).  Deletes assets['predictions'] as the reference does."""
    files = {}
    labelling = dump_for_auto_labelling or dump_for_submission
    writes, visualised = dumps(val_idx, val_len, dump_all_images, dump_num, global_rank, labelling)
    if not writes:
        return files
    assets = dump_dict["assets"]
    image = _np(dump_dict["input_images"][0])
    prob = _np(assets["prob_mask"][0])
    gt = _np(dump_dict["gt_images"][0])
    prediction = _np(assets["predictions"][0])
    del assets["predictions"]
    name = dump_dict["img_names"][0]
    if dump_for_auto_labelling:
        files["%s_prob.png" % name] = ("L", mask_bytes(prob))
    if labelling:
        label_out = np.zeros_like(prediction)
        for label_id, train_id in dataset.id_to_trainid.items():
            label_out[np.where(prediction == train_id)] = label_id
        files["%s.png" % name] = ("L", np.clip(label_out, 0, 255).astype(np.uint8))
        return files
    inv_mean, inv_std = inv_norm(mean, std)
    rgb = denorm_bytes(image, inv_mean, inv_std)
    files["%s_input.png" % name] = ("RGB", rgb)
    files["%s_gt.png" % name] = _p_entry(dataset.colorize_mask(gt))
    pred_pil = dataset.colorize_mask(prediction)
    files["%s_prediction.png" % name] = _p_entry(pred_pil)
    files["composited_%s.png" % name] = ("RGB", blend_bytes(rgb, np.array(pred_pil.convert("RGB"))))
    if not visualised or not dump_assets:
        return files
    for asset in assets:
        mask = assets[asset][0]
        fn = "%s_%s.png" % (name, asset)
        if "pred_" in asset:
            files[fn] = _p_entry(dataset.colorize_mask(_np(mask)))
            continue
        mask = _np(mask).squeeze()
        l8 = err_bytes(mask) if mask.dtype.kind in "iub" else mask_bytes(mask)
        files[fn] = ("RGB", np.ascontiguousarray(np.repeat(l8[..., None], 3, axis=-1)))
    return files


def webpage_rows(dump_dict_names, asset_names, save_dir, dump_assets):
    """imgs_to_webpage entry of one visualised image (misc.py:356-360, 383): plain names for the three images, the
    joined path for asset masks (pred_* assets are not listed)."""
    name = dump_dict_names[0]
    rows = [("%s_input.png" % name, "input"), ("%s_gt.png" % name, "gt"), ("%s_prediction.png" % name, "prediction")]
    if dump_assets:
        rows += [(os.path.join(save_dir, "%s_%s.png" % (name, a)), a) for a in asset_names if "pred_" not in a]
    return rows


def load_golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["meta"]))


def golden_dataset(meta):
    return Dataset(meta["color_mapping"], {int(k): int(v) for k, v in meta["id_to_trainid"]})


def golden_dump_dict(z, meta):
    """The dump_dict the golden maker handed to the reference (host assets), fresh on every call."""
    assets = {}
    for key in meta["asset_order"]:
        a = z["asset_" + key]
        assets[key] = torch.from_numpy(a.copy()) if key == "prob_mask" or "attn_" in key else a.copy()
    return {"input_images": torch.from_numpy(z["input_images"].copy()), "gt_images": torch.from_numpy(z["gt_images"].copy()),
            "img_names": list(meta["img_names"]), "assets": assets}


def golden_files(z, meta, mode):
    out = {}
    for i, e in enumerate(meta["files"][mode]):
        arr = z["file_%s_%d" % (mode, i)]
        out[e["name"]] = (e["mode"], arr, z["pal_%s_%d" % (mode, i)]) if e["mode"] == "P" else (e["mode"], arr)
    return out
