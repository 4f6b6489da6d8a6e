"""ImageDumper on the device (utils/misc.py:204-417, driven from train.py:552-597).

The reference's class of that name with the per-pixel work of `dump` in csrc/dump_tail.hip: the de-normalised input and
its composite with the colourised prediction, the train-id -> label-id mapping of --dump_for_submission /
--dump_for_auto_labelling, the byte forms of the probability, the error mask and the attention maps.  Same constructor,
attributes (`save_dir`, `viz_frequency`, `dump_frequency`, `imgs_to_webpage`, `imgs_to_tensorboard`), methods, file
names, directories and image modes; `dropin.install(device_dumper=True)` registers it as `utils.misc.ImageDumper`.

`dump` takes the reference's host assets (utils/trnval_utils.py:187-196: int64 ndarrays, CPU tensors; uploaded first)
and the device assets of `eval_minibatch(..., assets_on_device=True)`.  Per dumped image:
  one ssa_dump_tail for everything at the image's size (input, composite; with dump_assets the bytes of prob_mask and
  err_mask), one ssa_mask_u8 per attn_* asset, and ONE trip back (`_to_host`: pinned copies, one synchronisation).
  A P file stores indices, and the prediction and every pred_* asset already ARE index bytes on the device: they ride
  in that trip as they are and get the dataset's palette on the host (colorize_mask), as the label map does.
In the two labelling modes one launch writes the label ids and (auto-labelling) the probability bytes: 2 bytes per pixel
come back.  `{name}.png` and `{name}_prob.png` are written with Pillow where the reference calls cv2.imwrite.
The tensorboard grid is not built: `tensorboard=` is accepted and `imgs_to_tensorboard` stays empty."""
import ctypes
import importlib
import os

import numpy as np
import torch
from PIL import Image

from .._lib import lib, check
_et = importlib.import_module(__package__ + ".eval_tail")    # (the package re-exports a function of that name)

ALPHA = 0.4                                    # misc.py:342


class ResultsPage(object):
    """utils/results_page.py:80-154: the HTML page of embedded images."""

    def __init__(self, experiment_name, html_filename):
        self.experiment_name = experiment_name
        self.html_filename = html_filename
        self.outfile = open(self.html_filename, 'w')
        self.items = []

    def _print_header(self):
        self.outfile.write('<!DOCTYPE html>\n<html>\n  <head>\n    <title>Experiment = {}</title>\n  </head>\n'
                           '  <body>'.format(self.experiment_name))

    def _print_footer(self):
        self.outfile.write('  </body>\n</html>')

    def _print_table_header(self, table_name):
        self.outfile.write('    <h3>{}</h3>\n    <table border="1" style="table-layout: fixed;">\n'
                           '      <tr>'.format(table_name))

    def _print_table_footer(self):
        self.outfile.write('      </tr>\n    </table>')

    def _print_table_guts(self, img_fn, descr):
        self.outfile.write('        <td halign="center" style="word-wrap: break-word;" valign="top">\n'
                           '          <p>\n            <a href="{img_fn}">\n'
                           '              <img src="{img_fn}" style="width:768px">\n            </a><br>\n'
                           '            <p>{descr}</p>\n          </p>\n        </td>'.format(img_fn=img_fn, descr=descr))

    def add_table(self, img_label_pairs, table_heading=''):
        self.items.append([img_label_pairs, table_heading])

    def _write_table(self, table, heading):
        self._print_table_header(heading)
        for img, descr in table:
            self._print_table_guts(img, descr)
        self._print_table_footer()

    def write_page(self):
        self._print_header()
        for table, heading in self.items:
            self._write_table(table, heading)
        self._print_footer()
        self.outfile.flush()


def palette_table(colorize_mask):
    """256 x 3 bytes: the RGB conversion of colorize_mask over every index -- Pillow's own answer for any palette (a
    palette shorter than 256 entries is black beyond its end)."""
    pil = colorize_mask(np.arange(256, dtype=np.uint8).reshape(1, 256))
    return np.ascontiguousarray(np.array(pil.convert("RGB"))[0])


def id_table(id_to_trainid):
    """256 bytes: misc.py:321-322 over the indices 0..255, in the dictionary's order (later entries win).  Train ids
    outside 0..255 are skipped; label ids are clipped into a byte, where OpenCV's imwrite would saturate."""
    lut = np.zeros(256, np.int64)
    for label_id, train_id in id_to_trainid.items():
        if 0 <= train_id <= 255:
            lut[train_id] = label_id
    return np.clip(lut, 0, 255).astype(np.uint8)


def _default_device():
    return torch.device("cuda", torch.cuda.current_device())


def _bytes(x, dev):
    """Class ids / a 0-1 mask -> uint8 tensor on dev holding the low 8 bits (astype(np.uint8))."""
    t = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    if t.dtype != torch.uint8:
        t = t.to(torch.int64).bitwise_and(255).to(torch.uint8)
    return t.to(dev).contiguous()


def _host_u8(x):
    """The same bytes as an ndarray, for a tensor or array that is on the host already."""
    a = x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return a.astype(np.uint8)


def _on_host(x):
    return not (isinstance(x, torch.Tensor) and x.device.type != "cpu")


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class _Pack:
    """The byte outputs of one dumped image in ONE device buffer (16-byte aligned pieces): one copy brings them back."""

    def __init__(self):
        self.sizes, self.offsets, self.total, self.buf = {}, {}, 0, None

    def add(self, name, shape):
        self.offsets[name], self.sizes[name] = self.total, tuple(shape)
        self.total += (int(np.prod(shape)) + 15) // 16 * 16

    def alloc(self, dev):
        self.buf = torch.empty((max(self.total, 16),), dtype=torch.uint8, device=dev)

    def dev(self, name):
        if name not in self.offsets:
            return None
        n = int(np.prod(self.sizes[name]))
        return self.buf[self.offsets[name]:self.offsets[name] + n]

    def host(self, hbuf, name):
        n = int(np.prod(self.sizes[name]))
        return hbuf[self.offsets[name]:self.offsets[name] + n].reshape(self.sizes[name])


class ImageDumper():
    """utils/misc.py:204-417.  You pass images/tensors from the evaluation loop into this object; it converts them to
    images on the device and writes them to disk."""

    def __init__(self, val_len, tensorboard=True, write_webpage=True, webpage_fn='index.html', dump_all_images=False,
                 dump_assets=False, dump_err_prob=False, dump_num=10, dump_for_auto_labelling=False,
                 dump_for_submission=False):
        cfg = self._cfg()
        self.val_len = val_len
        self.tensorboard = tensorboard
        self.write_webpage = write_webpage
        self.webpage_fn = os.path.join(cfg.RESULT_DIR, 'best_images', webpage_fn)
        self.dump_assets = dump_assets
        self.dump_for_auto_labelling = dump_for_auto_labelling
        self.dump_for_submission = dump_for_submission
        self.viz_frequency = max(1, val_len // dump_num)
        self.dump_frequency = 1 if dump_all_images else self.viz_frequency
        # the fp32 values Normalize forms from these Python floats (misc.py:240-245)
        self.inv_mean = (ctypes.c_float * 3)(*[-mean / std for mean, std in zip(cfg.DATASET.MEAN, cfg.DATASET.STD)])
        self.inv_std = (ctypes.c_float * 3)(*[1 / std for std in cfg.DATASET.STD])
        if self.dump_for_submission:
            self.save_dir = os.path.join(cfg.RESULT_DIR, 'submit')
        elif self.dump_for_auto_labelling:
            self.save_dir = os.path.join(cfg.RESULT_DIR)
        else:
            self.save_dir = os.path.join(cfg.RESULT_DIR, 'best_images')
        os.makedirs(self.save_dir, exist_ok=True)
        self.imgs_to_tensorboard = []
        self.imgs_to_webpage = []
        self._tables = {}                       # device -> (palette [256][3], id table [256]) of cfg.DATASET_INST

    @staticmethod
    def _cfg():
        """The reference's cfg when its config module is loaded (RESULT_DIR, DATASET_INST and GLOBAL_RANK live there),
        else this package's."""
        import sys
        ref = sys.modules.get("config")
        if ref is not None and hasattr(ref, "assert_and_infer_cfg"):
            return ref.cfg
        from ..config import cfg
        return cfg

    def reset(self):
        self.imgs_to_tensorboard = []
        self.imgs_to_webpage = []

    def _device_tables(self, dev, dataset):
        key = (str(dev), id(dataset))
        if key not in self._tables:
            pal = torch.from_numpy(palette_table(dataset.colorize_mask)).to(dev)
            ids = torch.from_numpy(id_table(getattr(dataset, "id_to_trainid", {}))).to(dev)
            self._tables[key] = (pal, ids)
        return self._tables[key]

    def dump(self, dump_dict, val_idx):
        """
        dump a single batch of images

        :dump_dict: a dictionary containing elements to dump out
          'input_images': source image
          'gt_images': label
          'img_names': img_names
          'assets': dict with keys:
            'predictions': final prediction
            'pred_*': different scales of predictions
            'attn_*': different scales of attn
            'err_mask': err_mask
            ('input_images', 'gt_images': the device copies eval_minibatch(assets_on_device=True) made)
        """
        from .. import hip_backend as hb
        cfg = self._cfg()
        rank = getattr(cfg, "GLOBAL_RANK", 0)
        labelling = self.dump_for_auto_labelling or self.dump_for_submission
        if not labelling and (val_idx % self.dump_frequency or rank != 0):
            return
        dataset = cfg.DATASET_INST
        idx = 0  # only use first element of batch
        assets = dump_dict['assets']
        input_image = assets.get('input_images', dump_dict['input_images'])[idx]
        prob_image = assets['prob_mask'][idx]
        gt_image = dump_dict['gt_images'][idx]
        prediction = assets['predictions'][idx]
        del assets['predictions']
        img_name = dump_dict['img_names'][idx]
        dev = next((t.device for t in (prediction, prob_image, input_image)
                    if isinstance(t, torch.Tensor) and t.device.type != "cpu"), None) or _default_device()
        pal, ids = self._device_tables(dev, dataset)
        H, W = int(prediction.shape[-2]), int(prediction.shape[-1])
        pred_d = _bytes(prediction, dev)
        L = lib()

        def launch(H, W, image=None, pred=None, prob=None, err=None, **outs):
            check(L.ssa_dump_tail(_p(image), image.stride(0) if image is not None else 0, self.inv_mean, self.inv_std,
                                  None, _p(pred), _p(pal), _p(ids), _p(prob), _p(err), ALPHA, H, W,
                                  *[_p(outs.get(k)) for k in ("input_rgb", "gt_rgb", "pred_rgb", "comp_rgb",
                                                              "label_ids", "prob_u8", "err_u8")], hb._s()),
                  "ssa_dump_tail")

        def prob_on_device():
            p = torch.as_tensor(prob_image).to(device=dev, dtype=torch.float32).contiguous()
            assert tuple(p.shape) == (H, W), "prob_mask must have the prediction's size"
            return p

        pack = _Pack()
        if labelling:
            pack.add("label_ids", (H, W))
            prob_d = None
            if self.dump_for_auto_labelling:
                pack.add("prob_u8", (H, W))
                prob_d = prob_on_device()
            pack.alloc(dev)
            launch(H, W, pred=pred_d, prob=prob_d, label_ids=pack.dev("label_ids"), prob_u8=pack.dev("prob_u8"))
            hbuf = _et._to_host([pack.buf])[0].numpy()
            if self.dump_for_auto_labelling:
                Image.fromarray(pack.host(hbuf, "prob_u8")).save(os.path.join(self.save_dir, '{}_prob.png'.format(img_name)))
            Image.fromarray(pack.host(hbuf, "label_ids")).save(os.path.join(self.save_dir, '{}.png'.format(img_name)))
            return

        visualised = not (val_idx % self.viz_frequency or rank != 0)
        image_d = torch.as_tensor(input_image).to(device=dev, dtype=torch.float32)
        if image_d.dim() != 3 or image_d.shape[0] != 3 or tuple(image_d.shape[1:]) != (H, W):
            raise ValueError("input image %s does not match the prediction %s" % (tuple(image_d.shape), (H, W)))
        if image_d.stride(2) != 1 or image_d.stride(1) != W or image_d.stride(0) < H * W:
            image_d = image_d.contiguous()
        pack.add("input_rgb", (H, W, 3))
        pack.add("comp_rgb", (H, W, 3))
        # the assets: what needs a kernel, what travels as it is (index bytes), what is on the host already
        in_launch, masks, index_assets = {}, [], []
        if visualised and self.dump_assets:
            for asset in assets:
                if asset in ('input_images', 'gt_images'):
                    continue
                mask = assets[asset][idx]
                if 'pred_' in asset:
                    index_assets.append((asset, mask))
                    continue
                sq = mask.squeeze()
                floating = sq.is_floating_point() if isinstance(sq, torch.Tensor) else sq.dtype.kind == "f"
                if tuple(sq.shape) == (H, W) and floating and "prob_u8" not in in_launch:
                    in_launch["prob_u8"] = asset
                    pack.add(asset, (H, W))
                    masks.append((asset, "prob", torch.as_tensor(sq).to(device=dev, dtype=torch.float32).contiguous()))
                elif tuple(sq.shape) == (H, W) and not floating and "err_u8" not in in_launch:
                    in_launch["err_u8"] = asset
                    pack.add(asset, (H, W))
                    masks.append((asset, "err", _bytes(sq, dev)))
                elif floating:
                    pack.add(asset, tuple(sq.shape))
                    masks.append((asset, "mask", torch.as_tensor(sq).to(device=dev, dtype=torch.float32).contiguous()))
                else:
                    pack.add(asset, tuple(sq.shape))
                    masks.append((asset, "bits", _bytes(sq, dev)))
        pack.alloc(dev)
        by_kind = {kind: (asset, t) for asset, kind, t in masks if kind in ("prob", "err")}
        launch(H, W, image=image_d, pred=pred_d, prob=by_kind.get("prob", (None, None))[1],
               err=by_kind.get("err", (None, None))[1], input_rgb=pack.dev("input_rgb"), comp_rgb=pack.dev("comp_rgb"),
               prob_u8=pack.dev(by_kind["prob"][0]) if "prob" in by_kind else None,
               err_u8=pack.dev(by_kind["err"][0]) if "err" in by_kind else None)
        for asset, kind, t in masks:
            if kind == "mask":
                check(L.ssa_mask_u8(_p(t), t.numel(), _p(pack.dev(asset)), hb._s()), "ssa_mask_u8")
            elif kind == "bits":                # an integer mask at a size of its own: (m * 255) & 255
                launch(1, t.numel(), err=t, err_u8=pack.dev(asset))
        # one trip: the packed bytes and whatever index bytes live on the device
        travel = [pack.buf]
        if not _on_host(prediction):
            travel.append(pred_d)
        dev_index = [(a, _bytes(m, dev)) for a, m in index_assets if not _on_host(m)]
        travel += [t for _, t in dev_index]
        if not _on_host(gt_image):              # (the loader's label map is a host tensor; a device one travels too)
            travel.append(_bytes(gt_image, dev))
        host = _et._to_host(travel)
        hbuf = host[0].numpy()
        pred_h = _host_u8(prediction) if _on_host(prediction) else host[1].numpy()
        first_index = 1 if _on_host(prediction) else 2
        index_h = dict(zip([a for a, _ in dev_index], [h.numpy() for h in host[first_index:first_index + len(dev_index)]]))
        gt_h = _host_u8(gt_image) if _on_host(gt_image) else host[-1].numpy()

        colorize_mask_fn = dataset.colorize_mask
        input_image_fn = f'{img_name}_input.png'
        Image.fromarray(pack.host(hbuf, "input_rgb")).save(os.path.join(self.save_dir, input_image_fn))
        gt_fn = '{}_gt.png'.format(img_name)
        colorize_mask_fn(gt_h).save(os.path.join(self.save_dir, gt_fn))
        prediction_fn = '{}_prediction.png'.format(img_name)
        colorize_mask_fn(pred_h).save(os.path.join(self.save_dir, prediction_fn))
        composited_fn = os.path.join(self.save_dir, 'composited_{}.png'.format(img_name))
        Image.fromarray(pack.host(hbuf, "comp_rgb")).save(composited_fn)

        # only visualize a limited number of images
        if not visualised:
            return
        to_webpage = [(input_image_fn, 'input'), (gt_fn, 'gt'), (prediction_fn, 'prediction')]
        if self.dump_assets:
            kinds = {asset: kind for asset, kind, _ in masks}
            for asset in assets:
                if asset in ('input_images', 'gt_images'):
                    continue
                mask_fn = os.path.join(self.save_dir, f'{img_name}_{asset}.png')
                if 'pred_' in asset:
                    m = assets[asset][idx]
                    colorize_mask_fn(index_h[asset] if asset in index_h else _host_u8(m)).save(mask_fn)
                    continue
                assert asset in kinds
                Image.fromarray(pack.host(hbuf, asset)).convert('RGB').save(mask_fn)
                to_webpage.append((mask_fn, asset))
        self.imgs_to_webpage.append(to_webpage)

    def write_summaries(self, was_best):
        """The html summary page (always); the tensorboard image grid of the reference is not built."""
        if self.write_webpage:
            ip = ResultsPage('prediction examples', self.webpage_fn)
            for img_set in self.imgs_to_webpage:
                ip.add_table(img_set)
            ip.write_page()
