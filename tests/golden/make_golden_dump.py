"""Golden files for the device ImageDumper, recorded from the REAL reference (utils/misc.py ImageDumper.dump, loaded
through ref_bootstrap.py) running on the installed Pillow, NumPy and torch.
    python tests/golden/make_golden_dump.py   ->   dump_golden.npz

What the image lacks is shimmed with the few lines it stands for: cv2.imwrite becomes a Pillow write of the array it is
handed (clipped into a byte as OpenCV's saturating conversion would), torchvision.transforms gets Normalize, ToPILImage,
Resize, ToTensor, CenterCrop and Compose, tabulate is inert.  The palette and label2trainid are the reference's own
(datasets/cityscapes.py fill_colormap's list, datasets/cityscapes_labels.py).

  input      a 2 x 3 x 37 x 53 batch: a random uint8 image normalised with the ImageNet mean / std, labels in 0..18 and
             255, 19-class predictions; assets pred_0.5x (19 x 27), attn_0.5x (fp32 in [0, 1], 19 x 27), prob_mask, err_mask
  files      the decoded files of the visual mode with dump_assets, of the submission mode and of the auto-labelling mode,
             with the web page rows of the visual mode
Data only."""
import importlib.util
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dump_ref as D                              # noqa: E402
from ref_bootstrap import REF, bootstrap          # noqa: E402


def transforms_shim():
    class Normalize:
        def __init__(self, mean, std):
            self.mean, self.std = mean, std

        def __call__(self, tensor):
            tensor = tensor.clone()
            mean = torch.as_tensor(self.mean, dtype=tensor.dtype)
            std = torch.as_tensor(self.std, dtype=tensor.dtype)
            return tensor.sub_(mean.view(-1, 1, 1)).div_(std.view(-1, 1, 1))

    class ToPILImage:
        def __call__(self, pic):
            if pic.is_floating_point():
                pic = pic.mul(255).byte()
            return Image.fromarray(np.transpose(pic.cpu().numpy(), (1, 2, 0)))

    class Resize:
        def __init__(self, size):
            self.size = size

        def __call__(self, img):
            w, h = img.size
            if w <= h:
                return img.resize((self.size, int(self.size * h / w)), Image.BILINEAR)
            return img.resize((int(self.size * w / h), self.size), Image.BILINEAR)

    class CenterCrop:
        def __init__(self, size):
            self.size = size

        def __call__(self, img):
            w, h = img.size
            th, tw = self.size
            left, top = int(round((w - tw) / 2.0)), int(round((h - th) / 2.0))
            return img.crop((left, top, left + tw, top + th))

    class ToTensor:
        def __call__(self, img):
            a = np.array(img.convert("RGB"))
            return torch.from_numpy(a).permute(2, 0, 1).float().div(255)

    class Compose:
        def __init__(self, ts):
            self.ts = ts

        def __call__(self, x):
            for t in self.ts:
                x = t(x)
            return x

    return dict(Normalize=Normalize, ToPILImage=ToPILImage, Resize=Resize, CenterCrop=CenterCrop, ToTensor=ToTensor,
                Compose=Compose)


def imwrite(path, arr):
    Image.fromarray(np.clip(np.asarray(arr), 0, 255).astype(np.uint8)).save(path)
    return True


def reference():
    cfg = bootstrap()
    sys.modules["cv2"].imwrite = imwrite
    sys.modules["torchvision.transforms"].__dict__.update(transforms_shim())
    sys.modules["tabulate"] = types.ModuleType("tabulate")
    sys.modules["tabulate"].tabulate = lambda *a, **k: ""
    import utils.misc as misc                     # the reference's
    spec = importlib.util.spec_from_file_location("ref_cityscapes_labels",
                                                  os.path.join(REF, "datasets", "cityscapes_labels.py"))
    labels = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(labels)
    return cfg, misc, labels


def cityscapes_color_mapping(labels):
    """fill_colormap's list (datasets/cityscapes.py:218-241): the colours of the train ids 0..18, zero padded."""
    by_train = {lb.trainId: lb.color for lb in labels.labels if 0 <= lb.trainId < 19 and not lb.ignoreInEval}
    pal = [v for t in range(19) for v in by_train[t]]
    return pal + [0] * (768 - len(pal))


def inputs():
    rng = np.random.RandomState(7)
    B, H, W, h, w = 2, 37, 53, 19, 27
    mean, std = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
    u8 = rng.randint(0, 256, (B, 3, H, W)).astype(np.uint8)
    x = torch.from_numpy(u8).float().div(255)
    x = x.sub(torch.tensor(mean).view(1, 3, 1, 1)).div(torch.tensor(std).view(1, 3, 1, 1))
    gts = rng.randint(0, 19, (B, H, W)).astype(np.int64)
    gts[rng.rand(B, H, W) < 0.15] = 255
    pred = rng.randint(0, 19, (B, H, W)).astype(np.int64)
    assets = {
        "pred_0.5x": rng.randint(0, 19, (B, h, w)).astype(np.int64),
        "attn_0.5x": rng.rand(B, 1, h, w).astype(np.float32),
        "predictions": pred,
        "prob_mask": rng.rand(B, H, W).astype(np.float32),
        "err_mask": ((pred != gts) & (gts != 255)).astype(int),
    }
    assets["attn_0.5x"][0, 0, 0, :4] = (0.0, 1.0, np.nextafter(np.float32(1), np.float32(0)), 0.5)
    return mean, std, x.numpy(), gts, assets, ["frankfurt_000000_000294", "second_of_the_batch"]


def main():
    cfg, misc, labels = reference()
    mean, std, images, gts, assets, names = inputs()
    color_mapping = cityscapes_color_mapping(labels)
    ds = D.Dataset(color_mapping, labels.label2trainid)
    cfg.DATASET.NAME = "cityscapes"
    cfg.DATASET.MEAN, cfg.DATASET.STD = mean, std
    cfg.DATASET_INST = ds
    cfg.GLOBAL_RANK = 0
    order = list(assets)
    out = {"input_images": images, "gt_images": gts}
    for k, v in assets.items():
        out["asset_" + k] = v
    meta = {"pillow": Image.__version__, "numpy": np.__version__, "torch": torch.__version__, "mean": mean, "std": std,
            "color_mapping": color_mapping, "id_to_trainid": [[int(k), int(v)] for k, v in labels.label2trainid.items()],
            "asset_order": order, "img_names": names, "files": {}, "val_len": 100}
    modes = {"visual": dict(dump_assets=True), "submission": dict(dump_for_submission=True),
             "auto_labelling": dict(dump_for_auto_labelling=True)}
    for mode, kw in modes.items():
        with tempfile.TemporaryDirectory() as tmp:
            cfg.RESULT_DIR = tmp
            dumper = misc.ImageDumper(val_len=100, tensorboard=False, write_webpage=True, **kw)
            dd = {"input_images": torch.from_numpy(images.copy()), "gt_images": torch.from_numpy(gts.copy()),
                  "img_names": list(names),
                  "assets": {k: (torch.from_numpy(v.copy()) if k == "prob_mask" or "attn_" in k else v.copy())
                             for k, v in assets.items()}}
            dumper.dump(dd, 0)
            assert "predictions" not in dd["assets"]
            entries = []
            for i, fn in enumerate(sorted(os.listdir(dumper.save_dir))):
                path = os.path.join(dumper.save_dir, fn)
                if not fn.endswith(".png"):
                    continue
                e = D.decode(path)
                out["file_%s_%d" % (mode, len(entries))] = e[1]
                if e[0] == "P":
                    out["pal_%s_%d" % (mode, len(entries))] = e[2]
                entries.append({"name": fn, "mode": e[0]})
            meta["files"][mode] = entries
            if mode == "visual":
                assert os.path.relpath(dumper.save_dir, tmp) == "best_images"
                meta["webpage"] = [[[os.path.relpath(f, dumper.save_dir) if os.path.isabs(f) else f, d] for f, d in row]
                                   for row in dumper.imgs_to_webpage]
                meta["tensorboard_images"] = len(dumper.imgs_to_tensorboard[0])
            else:
                meta["save_dir_" + mode] = os.path.relpath(dumper.save_dir, tmp)
    path = os.path.join(HERE, "dump_golden.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    print({m: [e["name"] for e in v] for m, v in meta["files"].items()}, "bytes", os.path.getsize(path))


if __name__ == "__main__":
    main()
