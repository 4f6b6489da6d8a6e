"""Evaluation tail on the GPU (utils/trnval_utils.py:82-198, utils/misc.py:50-67): the full [B,C,H,W] fp32 prediction
never travels to the host.

  confusion_matrix   argmax + histogram of one tensor (ssa_confusion_matrix)
  eval_tail          flip x scale averaging, argmax, max probability, error mask, histogram and cross entropy of up to
                     eight predictions in ONE launch (ssa_eval_tail, csrc/eval_tail.hip)
  eval_minibatch     the reference's function of that name on top of it (`dropin.install(device_eval_tail=True)` puts it
                     under `utils.trnval_utils`, where train.py imports it from)
"""
import ctypes
import sys

import numpy as np
import torch

from .._lib import lib, check


def confusion_matrix(pred, gts, num_classes, hist=None, return_predictions=False):
    """pred: the model's 'pred' output, [B,C,H,W] fp32 (the zero-copy NCHW view of an NHWC
    buffer that semseg_amd.network returns, or any layout); gts: [B,H,W] int64.
    Returns (hist int64 [C,C] on the device, accumulated into `hist` if given
    [, predictions uint8 [B,H,W]])."""
    assert pred.is_cuda and pred.dim() == 4 and pred.shape[1] == num_classes
    B, C, H, W = pred.shape
    nhwc = pred.permute(0, 2, 3, 1)
    if nhwc.dtype != torch.float32 or not nhwc.is_contiguous():
        nhwc = nhwc.float().contiguous()
    g = gts.to(device=pred.device, dtype=torch.int64).contiguous()
    assert tuple(g.shape) == (B, H, W)
    if hist is None:
        hist = torch.zeros((C, C), dtype=torch.int64, device=pred.device)
    out = torch.empty((B, H, W), dtype=torch.uint8, device=pred.device) if return_predictions else None
    P = ctypes.c_void_p
    check(lib().ssa_confusion_matrix(P(nhwc.data_ptr()), C, P(g.data_ptr()), B * H * W, C,
                                     P(out.data_ptr()) if out is not None else None, P(hist.data_ptr()),
                                     P(torch.cuda.current_stream().cuda_stream)), "ssa_confusion_matrix")
    return (hist, out) if return_predictions else hist


def fast_hist(pred, gtruth, num_classes):
    """Name-compatible with utils/misc.py:50 for device tensors: pred = class ids [N]
    (any integer dtype), gtruth [N]; returns int64 [C,C] on the device."""
    p = pred.reshape(-1).to(torch.int64)
    g = gtruth.reshape(-1).to(torch.int64)
    mask = (g >= 0) & (g < num_classes)
    return torch.bincount(num_classes * g[mask] + p[mask], minlength=num_classes ** 2).reshape(num_classes, num_classes)


class EvalTailResult:
    """Device tensors of one eval_tail call; what was not asked for is None."""
    __slots__ = ("pred", "prob", "err", "hist", "loss_acc", "avg")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def loss(self):
        """CrossEntropyLoss2d's mean as a Python float (one device-to-host copy); NaN over zero valid pixels."""
        return _mean_loss(self.loss_acc.cpu())


def _mean_loss(acc):
    a = acc.tolist()
    return float(np.float32(a[0] / a[1])) if a[1] else float("nan")


def eval_tail(srcs, flips, num_classes, gts=None, ignore_label=255, n_scales=1, n_flips=1, hist=None, loss_acc=None,
              want=("pred", "prob", "err"), avg=False):
    """out = (sum of srcs, those with flips[i] set mirrored along W) / n_scales / n_flips in the reference's statement
    order, then per pixel of `out`: first argmax (`pred`, uint8 [B,H,W]), maximum softmax probability (`prob`, fp32),
    error mask against `gts` (`err`, uint8) -- the ones named in `want` -- and, when `gts` is given, the confusion
    matrix (`hist`, int64 [C,C]) and CrossEntropyLoss2d's {sum, count} (`loss_acc`, double[2]); `hist` / `loss_acc`
    passed in are ACCUMULATED into.  avg=True also returns `out` as a [B,C,H,W] view of a dense NHWC tensor.
    srcs: 1..8 tensors [B,C,H,W] of one shape -- the permuted NHWC views the networks return are read in place (a
    channel slice of a wider NHWC buffer included), any other layout is made contiguous once."""
    from .. import hip_backend as hb
    srcs = list(srcs)
    flips = [int(bool(f)) for f in flips]
    if not 1 <= len(srcs) <= 8 or len(flips) != len(srcs):
        raise ValueError("eval_tail takes 1..8 sources and one flip flag per source")
    B, C, H, W = srcs[0].shape
    if C != num_classes or any(tuple(t.shape) != (B, C, H, W) for t in srcs):
        raise ValueError("eval_tail: every source must be [B, %d, H, W] of one size" % num_classes)
    dev = srcs[0].device
    prep = []
    for t in srcs:
        x = t.detach().permute(0, 2, 3, 1)
        prep.append(hb._pixels(x if x.dtype == torch.float32 else x.float()))
    if len({ld for _, ld in prep}) > 1:             # one pixel stride for all: the odd ones out become dense
        prep = [(x, ld) if ld == C else (x.contiguous(), C) for x, ld in prep]
    ld = prep[0][1]
    g = None
    if gts is not None:
        g = gts.to(device=dev, dtype=torch.int64).contiguous()
        if tuple(g.shape) != (B, H, W):
            raise ValueError("eval_tail: gts must be [B, H, W]")
        if hist is None:
            hist = torch.zeros((C, C), dtype=torch.int64, device=dev)
        if loss_acc is None:
            loss_acc = torch.zeros((2,), dtype=torch.float64, device=dev)
    else:
        hist = loss_acc = None

    def out(name, dtype):
        return torch.empty((B, H, W), dtype=dtype, device=dev) if name in want else None
    pred, prob = out("pred", torch.uint8), out("prob", torch.float32)
    err = out("err", torch.uint8) if g is not None else None
    dense = torch.empty((B, H, W, C), dtype=torch.float32, device=dev) if avg else None
    P = ctypes.c_void_p
    ptrs = (ctypes.c_void_p * len(prep))(*[x.data_ptr() for x, _ in prep])
    flg = (ctypes.c_int * len(prep))(*flips)
    check(lib().ssa_eval_tail(ptrs, flg, len(prep), ld, B, H, W, C, hb._p(g), int(ignore_label), float(n_scales),
                              float(n_flips), hb._p(pred), hb._p(prob), hb._p(err), hb._p(hist), hb._p(loss_acc),
                              hb._p(dense), hb._s()), "ssa_eval_tail")
    return EvalTailResult(pred=pred, prob=prob, err=err, hist=hist, loss_acc=loss_acc,
                          avg=dense.permute(0, 3, 1, 2) if avg else None)


# ---------------------------------------------------------------------------- eval_minibatch
_SYNC_CFG = [False]       # dropin.install(device_eval_tail=True): refresh our cfg from the reference's on every call


def flip_tensor(x, dim):
    """utils/trnval_utils.py:41-48 (an index gather there); pure data movement on the tensor's own device."""
    return torch.flip(x, (dim if dim >= 0 else x.dim() + dim,))


def resize_tensor(inputs, target_size):
    """utils/trnval_utils.py:51-55: bilinear, align_corners=cfg.MODEL.ALIGN_CORNERS (read at call time), [B,C,H,W] fp32
    through ssa_resize_bilinear_fwd; returns the permuted view of the new NHWC tensor."""
    from .. import hip_backend as hb
    from ..config import cfg
    x = inputs.detach().permute(0, 2, 3, 1)
    if x.dtype != torch.float32:
        x = x.float()
    with torch.no_grad():
        y = hb.BilinearFn.apply(x, int(target_size[0]), int(target_size[1]), True, bool(cfg.MODEL.ALIGN_CORNERS))
    return y.permute(0, 3, 1, 2)


def fmt_scale(prefix, scale):
    """utils/misc.py:503-513 (its replace() is discarded there: the name keeps the dot)."""
    return "%s_%sx" % (prefix, str(float(scale)))


def _to_host(tensors):
    """Device tensors -> host tensors with ONE synchronisation (pinned buffers, asynchronous copies)."""
    if not any(t.is_cuda for t in tensors):
        return list(tensors)
    outs = []
    for t in tensors:
        h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        h.copy_(t, non_blocking=True)
        outs.append(h)
    torch.cuda.current_stream().synchronize()
    return outs


def eval_minibatch(data, net, criterion, val_loss, calc_metrics, args, val_idx, assets_on_device=False, boundary=None):
    """utils/trnval_utils.py:82-198 with its tail on the device.  Same arguments, same returns: (assets, _iou_acc) with
    `predictions` int64 ndarray [B,H,W], `prob_mask` CPU fp32 tensor, `err_mask` int ndarray (calc_metrics), every
    `pred_*` of the last pass as int64 ndarray at its own size, every `attn_*` passed through, `_iou_acc` int64 [C,C];
    val_loss.update(loss, pixels) when calc_metrics.  The images go to the device of the net's first parameter once and
    are flipped / resized there; every pass's prediction (resized to the input size where its scale is not 1) is a
    source of ONE ssa_eval_tail.  What comes back per batch: uint8 predictions and error mask, the fp32 probability,
    C x C counters and two doubles, in one synchronisation.  The loss rides in the same launch when `criterion` is this
    package's CrossEntropyLoss2d with the dataset's ignore label; any other criterion is called on the averaged tensor.
    assets_on_device=True (what `dropin.install(device_dumper=True)` passes): the assets stay where the tail wrote them,
    for utils/dumper.py -- `predictions`, `err_mask` and every `pred_*` as device uint8, `prob_mask` as device fp32, the
    `attn_*` untouched, and the uploaded batch under `input_images` / `gt_images`; only the counters come back.
    boundary: a utils.f_boundary.BoundaryMeter, fed the final `pred` bytes and the ground truth on the device when
    calc_metrics (the reference's `mf_score`, which its own loop never fills); None leaves every path as it is."""
    from ..config import cfg
    from ..loss.criteria import CrossEntropyLoss2d
    if _SYNC_CFG[0] and "config" in sys.modules and hasattr(sys.modules["config"], "assert_and_infer_cfg"):
        from ..dropin import sync_config
        sync_config()
    scales = [args.default_scale]
    if args.multi_scale_inference:
        scales.extend([float(x) for x in args.extra_scales.split(",")])
    images, gt_image, img_names, scale_float = data
    assert images.dim() == 4 and gt_image.dim() == 3
    assert images.shape[2:] == gt_image.shape[1:]
    batch_pixel_size = images.size(0) * images.size(2) * images.size(3)
    input_size = images.size(2), images.size(3)
    flips = [1, 0] if args.do_flip else [0]       # ends unflipped: the dumped assets are those of the last pass
    dev = next(net.parameters()).device
    C = cfg.DATASET.NUM_CLASSES
    ignore = cfg.DATASET.IGNORE_LABEL
    with torch.no_grad():
        images = images.to(dev)
        gts = gt_image.to(dev)
        srcs, src_flips = [], []
        passes = [(f, s) for f in flips for s in scales]
        for i, (flip, scale) in enumerate(passes):
            inputs = flip_tensor(images, 3) if flip == 1 else images
            if scale != 1.0:
                inputs = resize_tensor(inputs, [round(sz * scale) for sz in input_size])
            output_dict = net({"images": inputs, "gts": gts})
            _pred = output_dict["pred"]
            if not cfg.MODEL.MSCALE:        # the averaged scales' own predictions, kept for visualisation
                output_dict[fmt_scale("pred", scale)] = _pred
            if scale != 1.0:
                _pred = resize_tensor(_pred, input_size)
            elif i + 1 < len(passes):
                _pred = _pred.clone()       # the net may reuse its output buffers in the next pass (GraphedEval)
            srcs.append(_pred)
            src_flips.append(flip)
        assert tuple(srcs[0].shape[2:]) == tuple(gts.shape[1:]) and srcs[0].shape[1] == C, \
            "output_size %s gt size %s" % (tuple(srcs[0].shape[1:]), tuple(gts.shape[1:]))
        fused = bool(calc_metrics) and isinstance(criterion, CrossEntropyLoss2d) and criterion.ignore_index == ignore
        res = eval_tail(srcs, src_flips, C, gts=gts, ignore_label=ignore, n_scales=len(scales), n_flips=len(flips),
                        want=("pred", "prob", "err") if calc_metrics else ("pred", "prob"),
                        avg=bool(calc_metrics) and not fused)
        if boundary is not None and calc_metrics:
            boundary.update(res.pred, gts)
        loss = None
        if calc_metrics and not fused:
            loss = criterion(res.avg, gts).item()
        names, extra = [], []
        for item, t in output_dict.items():
            if "pred_" in item:
                names.append(item)
                extra.append(eval_tail([t], [0], t.shape[1], want=("pred",)).pred)
        if assets_on_device:
            host = _to_host([res.hist] + ([res.loss_acc] if fused else []))
            if fused:
                loss = _mean_loss(host[1])
            if calc_metrics:
                val_loss.update(loss, batch_pixel_size)
            extra_d = dict(zip(names, extra))
            assets = {item: extra_d.get(item, output_dict[item]) for item in output_dict
                      if "attn_" in item or "pred_" in item}
            assets["predictions"], assets["prob_mask"] = res.pred, res.prob
            if calc_metrics:
                assets["err_mask"] = res.err
            assets["input_images"], assets["gt_images"] = images, gts
            return assets, host[0].numpy().astype(np.int64)
        dev_out = [res.pred, res.prob, res.hist] + ([res.err] if calc_metrics else []) + ([res.loss_acc] if fused else [])
        host = _to_host(dev_out + extra)
    pred_h, prob_h, hist_h = host[0], host[1], host[2]
    k = 3
    if calc_metrics:
        err_h = host[k]
        k += 1
    if fused:
        loss = _mean_loss(host[k])
        k += 1
    if calc_metrics:
        val_loss.update(loss, batch_pixel_size)
    extra_h = dict(zip(names, host[k:]))
    assets = {}
    for item in output_dict:
        if "attn_" in item:
            assets[item] = output_dict[item]
        if "pred_" in item:
            assets[item] = extra_h[item].numpy().astype(np.int64)
    assets["predictions"] = pred_h.numpy().astype(np.int64)
    assets["prob_mask"] = prob_h
    if calc_metrics:
        assets["err_mask"] = err_h.numpy().astype(int)
    return assets, hist_h.numpy().astype(np.int64)


def validate_topn(val_loader, net, criterion, optim, epoch, args):
    raise NotImplementedError("validate_topn is not provided: the reference's own version calls the undefined name "
                              "`run_minibatch` (utils/trnval_utils.py:227) and cannot run either")
