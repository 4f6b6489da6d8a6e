"""CPU restatement of the reference's evaluation tail, in its statement order: utils/trnval_utils.py:82-198
(eval_minibatch, flip_tensor, resize_tensor, calc_err_mask_all), utils/misc.py:50-67 (fast_hist), :503-513 (fmt_scale)
and loss/utils.py:121-134 (CrossEntropyLoss2d).  torch / numpy on the host only; nothing of semseg_amd is imported: this
is what the device tail (ssa_eval_tail, semseg_amd.utils.eval_minibatch) is compared against, and
tests/test_eval_tail_cpu.py pins it to a fixture recorded from the reference itself (tests/golden/evaltail_golden.pt).
Also the stub networks of the end-to-end cases."""
import numpy as np
import torch
import torch.nn.functional as F


def flip_tensor(x, dim):
    dim = x.dim() + dim if dim < 0 else dim
    index = tuple(slice(None) if i != dim else torch.arange(x.size(i) - 1, -1, -1).long() for i in range(x.dim()))
    return x[index]


def resize_tensor(x, size):
    return F.interpolate(x, size=size, mode="bilinear", align_corners=False)


def fmt_scale(prefix, scale):
    return "%s_%sx" % (prefix, str(float(scale)))


def calc_err_mask_all(pred, gtruth, ignore_label):
    mask = (gtruth >= 0) & (gtruth != ignore_label)
    return (mask & (pred != gtruth)).astype(int)


def fast_hist(pred, gtruth, num_classes):
    mask = (gtruth >= 0) & (gtruth < num_classes)
    hist = np.bincount(num_classes * gtruth[mask].astype(int) + pred[mask], minlength=num_classes ** 2)
    return hist.reshape(num_classes, num_classes)


def cross_entropy_2d(output, gts, ignore_label):
    return F.nll_loss(F.log_softmax(output, dim=1), gts, ignore_index=ignore_label)


def average(srcs, flips, n_scales, n_flips):
    """output = 0.0; output = output + (flipped) prediction, pass after pass; output / len(scales) / len(flips)"""
    output = 0.0
    for s, f in zip(srcs, flips):
        output = output + (flip_tensor(s, 3) if f else s)
    return output / n_scales / n_flips


def tail(srcs, flips, n_scales, n_flips, gts, num_classes, ignore_label, with_loss=True):
    """What follows the pass loop, on [B,C,H,W] CPU tensors: dict of avg, loss (a float; NaN over no valid pixel),
    predictions (int64 ndarray), prob_mask (fp32 tensor), err_mask, hist."""
    output = average(srcs, flips, n_scales, n_flips)
    out = {"avg": output}
    if gts is not None and with_loss:
        out["loss"] = cross_entropy_2d(output, gts, ignore_label).item()
    max_probs, predictions = F.softmax(output, dim=1).max(1)
    predictions = predictions.numpy()
    out["predictions"] = predictions
    out["prob_mask"] = max_probs
    if gts is not None:
        out["err_mask"] = calc_err_mask_all(predictions, gts.numpy(), ignore_label)
        out["hist"] = fast_hist(predictions.flatten(), gts.numpy().flatten(), num_classes)
    return out


def argmax_is_softmax_argmax(output):
    """The precondition of the exact integer comparisons: softmax merged no two distinct logits into one float at the
    maximum, so the first argmax of the probabilities is the first argmax of the logits."""
    return bool((F.softmax(output, dim=1).max(1)[1] == output.max(1)[1]).all())


def eval_minibatch(data, net, criterion, val_loss, calc_metrics, args, val_idx, num_classes, ignore_label, mscale,
                   debug=None):
    """The reference's eval_minibatch on CPU tensors (`.cuda()` dropped); cfg.DATASET.NUM_CLASSES / IGNORE_LABEL and
    cfg.MODEL.MSCALE are arguments.  debug (a dict) receives the averaged logits under 'output'."""
    scales = [args.default_scale]
    if args.multi_scale_inference:
        scales.extend([float(x) for x in args.extra_scales.split(",")])
    images, gt_image, img_names, scale_float = data
    assert len(images.size()) == 4 and len(gt_image.size()) == 3
    assert images.size()[2:] == gt_image.size()[1:]
    batch_pixel_size = images.size(0) * images.size(2) * images.size(3)
    input_size = images.size(2), images.size(3)
    flips = [1, 0] if args.do_flip else [0]
    with torch.no_grad():
        output = 0.0
        for flip in flips:
            for scale in scales:
                inputs = flip_tensor(images, 3) if flip == 1 else images
                infer_size = [round(sz * scale) for sz in input_size]
                if scale != 1.0:
                    inputs = resize_tensor(inputs, infer_size)
                output_dict = net({"images": inputs, "gts": gt_image})
                _pred = output_dict["pred"]
                if not mscale:
                    output_dict[fmt_scale("pred", scale)] = _pred
                if scale != 1.0:
                    _pred = resize_tensor(_pred, input_size)
                if flip == 1:
                    output = output + flip_tensor(_pred, 3)
                else:
                    output = output + _pred
    output = output / len(scales) / len(flips)
    assert output.size()[2:] == gt_image.size()[1:] and output.size()[1] == num_classes
    if debug is not None:
        debug["output"] = output
    if calc_metrics:
        val_loss.update(criterion(output, gt_image).item(), batch_pixel_size)
    output_data = F.softmax(output, dim=1).cpu().data
    max_probs, predictions = output_data.max(1)
    assets = {}
    for item in output_dict:
        if "attn_" in item:
            assets[item] = output_dict[item]
        if "pred_" in item:
            smax = F.softmax(output_dict[item], dim=1)
            _, pred = smax.data.max(1)
            assets[item] = pred.cpu().numpy()
    predictions = predictions.numpy()
    assets["predictions"] = predictions
    assets["prob_mask"] = max_probs
    if calc_metrics:
        assets["err_mask"] = calc_err_mask_all(predictions, gt_image.numpy(), ignore_label)
    _iou_acc = fast_hist(predictions.flatten(), gt_image.numpy().flatten(), num_classes)
    return assets, _iou_acc


# ------------------------------------------------------------------------------------------------ test fixtures
class Meter:
    """utils/misc.py AverageMeter, the part eval_minibatch touches."""

    def __init__(self):
        self.val = self.avg = self.sum = self.count = 0

    def update(self, val, n=1):
        self.val = val
        self.sum += val * n
        self.count += n
        self.avg = self.sum / self.count


class Args:
    def __init__(self, default_scale=1.0, multi_scale_inference=False, extra_scales="0.5,2.0", do_flip=False):
        self.default_scale = default_scale
        self.multi_scale_inference = multi_scale_inference
        self.extra_scales = extra_scales
        self.do_flip = do_flip


class CpuCrossEntropyLoss2d(torch.nn.Module):
    def __init__(self, ignore_index):
        super().__init__()
        self.ignore_index = ignore_index

    def forward(self, inputs, targets, do_rmi=None):
        return cross_entropy_2d(inputs, targets, self.ignore_index)


class MscaleStub(torch.nn.Module):
    """Stands in for an MSCALE network: every output is ONE multiplication of an image channel by a per-class constant
    (single rounding: the host and the device agree bit for bit, and a mirrored input gives the mirrored 'pred'); the
    half-size outputs take every second pixel."""

    def __init__(self, num_classes, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer("k", (torch.rand(3, num_classes, generator=g) * 4.0 - 2.0))
        self.num_classes = num_classes

    def forward(self, inputs):
        x = inputs["images"]
        ch = torch.arange(self.num_classes, device=x.device) % 3

        def logits(row):
            return x[:, ch] * self.k[row].view(1, -1, 1, 1)
        return {"pred": logits(0), "pred_05x": logits(1)[..., ::2, ::2].contiguous(), "pred_10x": logits(2),
                "attn_05x": (x[:, :1] * 0.25)[..., ::2, ::2].contiguous()}


class SeededStub(torch.nn.Module):
    """Stands in for a single-scale network under multi_scale_inference: ignores the pixel values and returns the
    n-th call's seeded logits (randn * 3) at the size of its input."""

    def __init__(self, num_classes, seed):
        super().__init__()
        self.anchor = torch.nn.Parameter(torch.zeros(1))
        self.num_classes, self.seed, self.calls = num_classes, seed, 0

    def forward(self, inputs):
        x = inputs["images"]
        g = torch.Generator().manual_seed(self.seed + self.calls)
        self.calls += 1
        y = torch.randn(x.shape[0], self.num_classes, x.shape[2], x.shape[3], generator=g) * 3.0
        return {"pred": y.to(x.device)}


def make_batch(B, H, W, num_classes, ignore_label, seed, with_negative=False):
    g = torch.Generator().manual_seed(seed)
    images = torch.randn(B, 3, H, W, generator=g) * 2.0
    gts = torch.randint(0, num_classes, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    gts[r < 0.1] = ignore_label
    if with_negative:
        gts[(r >= 0.1) & (r < 0.13)] = -1
    return images, gts.long(), ["img%d" % i for i in range(B)], 1.0
