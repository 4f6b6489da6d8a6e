"""Operator surface used by semseg_amd.network / semseg_amd.loss.

All functions take and return NHWC tensors ([B,H,W,C]); activations in the
backend's `act_dtype` (bf16 on the HIP backend), logits/losses fp32.  The
default -- and only shipped -- backend is the HIP one (hip_backend.py over
libsemseg_hip.so); it is created on first use and raises if the library is
missing.  `_set_backend_for_tests` exists so the CPU test-suite can check the
module wiring against the reference with the oracle's operators; product code
never calls it.

Multi-problem calls.  The hot ops (conv, conv+BN, BasicBlock, fuse sum, bilinear)
accept a LIST of independent problems wherever they accept a tensor -- the resolution
branches of a HighResolutionModule times the scale passes of MscaleOCR -- and return a
list.  `BackendBase` maps such a call over the single-problem primitives; the HIP
backend overrides them with grouped launches (one launch per kernel instantiation for
the whole list, csrc/group.h).
"""
import torch

_BACKEND = None


def _is_list(v):
    return isinstance(v, (list, tuple))


def _lst(v, n):
    return list(v) if _is_list(v) else [v] * n


def _align_corners():
    """cfg.MODEL.ALIGN_CORNERS (the reference's --align_corners), read when a resize is CALLED -- the reference reads it
    at import (network/mynn.py:15); here a changed flag holds from the next call on.  The HIP backend hands it to the
    kernels explicitly; a captured step (graphed.py) has the value of its capture baked in."""
    from .config import cfg
    return bool(cfg.MODEL.ALIGN_CORNERS)


class BackendBase:
    """List-aware front of the operator surface over single-problem primitives
    (`_conv2d`, `_conv_bn_act`, `_batch_norm_act`, `_sum_act`, `_bilinear`)."""

    def group(self):
        import contextlib
        return contextlib.nullcontext()

    def conv2d(self, x, weight, bias, stride, padding, dilation, out_f32=False, want_stats=False):
        if not _is_list(x):
            return self._conv2d(x, weight, bias, stride, padding, dilation, out_f32)
        n = len(x)
        return [self._conv2d(xi, w, b, stride, padding, dilation, out_f32)
                for xi, w, b in zip(x, _lst(weight, n), _lst(bias, n))]

    def cat_slots(self, like, widths):
        """Output placement for a later `cat`: None here (the result is concatenated by a copy); the HIP backend hands
        out channel slices of ONE buffer per problem of `like`, which `conv_bn_act(..., out=)` writes and `cat` then
        recognises -- the concatenation costs nothing (SpatialOCR_Module: 2 x 134 MB per step at 1024 x 1024)."""
        return None

    def conv_bn_act(self, conv, bn, x, residual=None, relu=False, post=None, out=None):
        assert out is None, "output placement is the HIP backend's (cat_slots returns None here)"
        if not _is_list(x):
            return self._conv_bn_act(conv, bn, x, residual, relu, post)
        n = len(x)
        return [self._conv_bn_act(c, b, xi, r, rl, po) for c, b, xi, r, rl, po in
                zip(_lst(conv, n), _lst(bn, n), x, _lst(residual, n), _lst(relu, n), _lst(post, n))]

    def batch_norm_act(self, x, bn, residual=None, relu=False, post=None):
        if not _is_list(x):
            return self._batch_norm_act(x, bn, residual, relu, post)
        n = len(x)
        return [self._batch_norm_act(xi, b, r, rl, po) for xi, b, r, rl, po in
                zip(x, _lst(bn, n), _lst(residual, n), _lst(relu, n), _lst(post, n))]

    def add_bn_act(self, a, b, bn, relu=True, post=None):
        """Head of a pre-activation block (network/wider_resnet.py:172-185): s = a + b, z = post * act(bn(s)); returns
        (s, z).  s is the block input: it also feeds the shortcut.  Here the composition of the two ops; the HIP backend
        takes the batch statistics in the pass that stores the sum and adds the shortcut's gradient in bn's backward."""
        s = self.sum_act([a, b], relu=False)
        return s, self.batch_norm_act(s, bn, None, relu, post)

    def depthwise_conv(self, x, weight, stride, dilation, want_stats=False):
        """nn.Conv2d(C, C, 3, stride, padding = dilation, dilation, groups = C, bias = False) (network/xception.py:29-37;
        fixed_padding is symmetric for a 3x3 kernel).  One problem.  Here a composition on the backend's own dense conv,
        so that every backend applies its own rounding model: the [C,1,3,3] weight scattered onto the diagonal of a
        dense [C,C,3,3] filter by a differentiable index write (the other products are exact zeros).  The HIP backend
        runs the depthwise kernels."""
        assert not _is_list(x), "depthwise_conv takes one problem"
        C = weight.shape[0]
        idx = torch.arange(C, device=weight.device)
        dense = weight.new_zeros((C, C) + tuple(weight.shape[2:])).index_put((idx, idx), weight[:, 0])
        return self._conv2d(x, dense, None, stride, dilation, dilation)

    def depthwise_conv_bn(self, sep, x):
        """The first half of a SeparableConv2d (network/xception.py:35-38): depthwise 3x3 -> sep.bn, no ReLU.  One problem."""
        dw = sep.conv1
        assert dw.groups == dw.in_channels == dw.out_channels and dw.kernel_size == (3, 3) and dw.bias is None and \
            dw.padding[0] in (0, dw.dilation[0])
        y = self.depthwise_conv(x, dw.weight, dw.stride[0], dw.dilation[0], want_stats=sep.bn.training)
        return self._batch_norm_act(y, sep.bn, None, False, None)

    def separable_conv_bn_act(self, sep, bn, x, residual=None, relu=False):
        """SeparableConv2d + the BatchNorm behind it (network/xception.py:24-40, 62-64): depthwise 3x3 -> sep.bn ->
        pointwise 1x1 -> bn (+ residual, ReLU).  One problem."""
        assert not _is_list(x), "separable_conv_bn_act takes one problem"
        return self.conv_bn_act(sep.pointwise, bn, self.depthwise_conv_bn(sep, x), residual, relu)

    def grouped_conv(self, x, weight, stride, dilation, groups, want_stats=False):
        """nn.Conv2d(C, C, 3, stride, padding = dilation, dilation, groups, bias = False) with 1 < groups < C
        (network/SEresnext.py:183-185 after the surgery of network/utils.py:71-81).  One problem.  The form of
        depthwise_conv: the [C,C/groups,3,3] weight copied onto the block diagonal of a dense [C,C,3,3] filter
        (differentiably; the other products are exact zeros), through the backend's own dense conv."""
        assert not _is_list(x), "grouped_conv takes one problem"
        C, Cg = weight.shape[0], weight.shape[1]
        assert C == Cg * groups, (tuple(weight.shape), groups)
        return self._conv2d(x, self._block_diagonal(weight, groups), None, stride, dilation, dilation)

    @staticmethod
    def _block_diagonal(weight, groups, padded=False):
        """[C, C / groups, kh, kw] -> the dense [C, C, kh, kw] filter with the groups on the block diagonal.  One strided
        copy into the diagonal view of a zero tensor (differentiable: the weight's gradient is that view of the dense
        filter's), no index tensors.  padded: the rows of the result have a spare element, so the result is not
        contiguous (HipBackend.grouped_conv says why)."""
        C, Cg, kh, kw = weight.shape
        assert C == Cg * groups, (tuple(weight.shape), groups)
        dense = weight.new_zeros((C, C, kh, kw + int(bool(padded))))[..., :kw]
        diag = torch.diagonal(dense.view(groups, Cg, groups, Cg, kh, kw), 0, 0, 2)        # [Cg, Cg, kh, kw, groups]
        diag.copy_(weight.view(groups, Cg, Cg, kh, kw).permute(1, 2, 3, 4, 0))
        return dense

    def grouped_conv_bn_act(self, conv, bn, x, relu=False):
        """Grouped 3x3 `conv` -> bn (-> ReLU): conv2 / bn2 of an SE-ResNeXt bottleneck (network/SEresnext.py:105-107).
        One problem."""
        assert conv.kernel_size == (3, 3) and conv.bias is None and conv.padding[0] == conv.dilation[0] and \
            conv.in_channels == conv.out_channels and conv.padding_mode == "zeros"
        y = self.grouped_conv(x, conv.weight, conv.stride[0], conv.dilation[0], conv.groups, want_stats=bn.training)
        return self.batch_norm_act(y, bn, None, relu, None)

    @staticmethod
    def _dil_conv_check(conv):
        assert conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.bias is None and conv.groups == 1 and \
            tuple(conv.padding) == tuple(conv.dilation) and conv.padding_mode == "zeros", \
            "dil_conv_bn_act takes nn.Conv2d(Cin, Cout, 3, stride 1, padding = dilation = (dh, dw), bias = False)"

    def dil_conv_bn_act(self, conv, bn, x, relu=True, out=None):
        """3x3 stride-1 `conv` with a dilation per axis, padding = dilation -> bn (-> ReLU): one conv of the Dense
        Prediction Cell (dpc_conv, network/utils.py:249-260).  x: one problem, or a LIST of independent problems (b, c, d
        of the cell) with `conv` / `bn` (/ `out`) lists of the same length.  Here the backend's own dense conv primitive
        with the TUPLE padding / dilation (it ends in F.conv2d, which takes them per axis), so that every backend applies
        its own rounding model -- the discipline of grouped_conv_bn_act -- then its own BatchNorm.  The HIP backend, whose
        conv route reads one dilation, overrides this with the kernels of csrc/conv_dil.hip."""
        assert out is None, "output placement is the HIP backend's (cat_slots returns None here)"
        if _is_list(x):
            return [self.dil_conv_bn_act(c, b, xi, relu) for c, b, xi in zip(conv, bn, x)]
        self._dil_conv_check(conv)
        y = self._conv2d(x, conv.weight, None, 1, tuple(conv.padding), tuple(conv.dilation))
        return self.batch_norm_act(y, bn, None, relu, None)

    def max_pool3x3s2_ceil(self, x):
        """nn.MaxPool2d(3, stride=2, ceil_mode=True), no padding (network/SEresnext.py:271-272): [B,H,W,C] ->
        [B,H//2,W//2,C] for H, W >= 2; a window that overhangs the edge takes the taps it has."""
        y = torch.nn.functional.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 0, ceil_mode=True)
        return y.permute(0, 2, 3, 1)

    def se_gate_add_act(self, se, y, residual=None, relu=True):
        """Squeeze-and-excitation gate and the block tail behind it (network/SEresnext.py:84-91, 115-116):
        s = sigmoid(fc2(relu(fc1(mean_hw(y))))) per (image, channel), z = act(s * y + residual).  One problem."""
        m = self.global_avg_pool(y)
        h = self.relu(self._conv2d(m, se.fc1.weight, se.fc1.bias, 1, 0, 1))
        s = self.sigmoid(self._conv2d(h, se.fc2.weight, se.fc2.bias, 1, 0, 1))
        z = s.to(y.dtype) * y
        if residual is not None:
            z = z + residual
        return torch.relu(z) if relu else z

    def basic_block(self, blocks, xs):
        """conv3x3-BN-ReLU-conv3x3-BN-(+x)-ReLU (network/hrnetv2.py:37-66, no downsample branch)
        of blocks[i] on xs[i]."""
        mid = [self._conv_bn_act(b.conv1, b.bn1, x, None, True, None) for b, x in zip(blocks, xs)]
        return [self._conv_bn_act(b.conv2, b.bn2, m, x, True, None) for b, m, x in zip(blocks, mid, xs)]

    def sum_act(self, tensors, relu=True):
        if tensors and _is_list(tensors[0]):
            return [self._sum_act(t, relu) for t in tensors]
        return self._sum_act(tensors, relu)

    def bilinear(self, x, size, out_f32=False):
        if not _is_list(x):
            return self._bilinear(x, size, out_f32)
        sizes = size if _is_list(size[0]) or hasattr(size[0], "__len__") else [size] * len(x)
        return [self._bilinear(xi, s, out_f32) for xi, s in zip(x, sizes)]

    def upsample_cat(self, groups):
        """groups[p] = [y0, y1, ...] (NHWC): y1.. resized to y0's size (bilinear, align_corners=False) and all of them
        concatenated on channels -- the head input of HighResolutionNet.forward (network/hrnetv2.py:418-431)."""
        sizes = [tuple(g[0].shape[1:3]) for g in groups]
        low = [(p, i) for p, g in enumerate(groups) for i in range(1, len(g))]
        ups = self.bilinear([groups[p][i] for p, i in low], [sizes[p] for p, i in low]) if low else []
        up = dict(zip(low, ups))
        return [self.cat([g[0]] + [up[(p, i)] for i in range(1, len(g))]) for p, g in enumerate(groups)]

    def fan_out(self, tensors, counts):
        """tensors[i] is about to be consumed counts[i] times: returns counts[i] handles per tensor (the
        HIP backend sums their gradients with one grouped launch instead of autograd's adds)."""
        return [[t] * c for t, c in zip(tensors, counts)]

    def fork(self, thunk, tag="fuse", has_bn=True):
        """A sub-graph nothing on the caller's path needs until `join()`: returns join, a callable that hands back
        thunk's result.  Here it simply ran; the HIP backend issues it on a second stream (a parallel branch of the
        captured step) and `join()` makes the current stream wait for it."""
        out = thunk()
        return lambda: out

    @staticmethod
    def parallel(thunks, level=1):
        """Independent sub-graphs, issued one after the other (thunks[1:] first, thunks[0] last:
        the reference runs the low-scale pass before the 1.0x pass, and BatchNorm running
        statistics are updated in issue order)."""
        outs = [None] * len(thunks)
        for i in range(1, len(thunks)):
            outs[i] = thunks[i]()
        outs[0] = thunks[0]()
        return outs


class HipBackend(BackendBase):
    name = "hip"

    def __init__(self):
        from . import hip_backend as hb
        hb.lib()   # fail loudly now if the extension is absent
        self.hb = hb
        self.act_dtype = hb.ACT_DTYPE

    def begin_step(self, device=None):
        self.hb.begin_step(device)

    def group(self):
        return self.hb.group()

    def image_to_nhwc(self, images, out_hw=None):
        return self.hb.image_to_nhwc(images, out_hw, align_corners=_align_corners())

    # -- convolution -----------------------------------------------------------------
    def conv2d(self, x, weight, bias, stride, padding, dilation, out_f32=False, want_stats=False):
        multi = _is_list(x)
        xs = list(x) if multi else [x]
        n = len(xs)
        ws, bs = _lst(weight, n), _lst(bias, n)
        spec = tuple((stride, padding, dilation, bool(out_f32), bool(want_stats)) for _ in range(n))
        flat = []
        for xi, w, b in zip(xs, ws, bs):
            flat += [xi, w, b]
        ys = self.hb.ConvGroupFn.apply(spec, *flat)
        return list(ys) if multi else ys[0]

    def _conv2d(self, x, weight, bias, stride, padding, dilation, out_f32=False):
        """One problem through conv2d: what BackendBase's compositions (depthwise_conv's dense form) call."""
        return HipBackend.conv2d(self, x, weight, bias, stride, padding, dilation, out_f32)

    def _bn_meta(self, bn, relu):
        track = bn.training and bn.track_running_stats and bn.running_mean is not None
        # training: the running statistics are updated by end_forward() (deferred, one launch, in
        # issue order: the passes over one layer are problems of the same grouped launch)
        return self.hb.BnMeta(0.1 if bn.momentum is None else bn.momentum, bn.eps, bool(bn.training), bool(relu),
                              getattr(bn, "sync", False), self.hb._BN_UPDATES.slot(bn) if track else None,
                              None if bn.training else bn.running_mean, None if bn.training else bn.running_var)

    def batch_norm_act(self, x, bn, residual=None, relu=False, post=None):
        multi = _is_list(x)
        xs = list(x) if multi else [x]
        n = len(xs)
        zs = self._bn_group(xs, _lst(bn, n), _lst(residual, n), _lst(relu, n), _lst(post, n))
        return zs if multi else zs[0]

    def _bn_group(self, xs, bns, ress, relus, posts, outs=None):
        metas = tuple(self._bn_meta(b, r) for b, r in zip(bns, relus))
        if outs is not None:
            for m, o in zip(metas, outs):
                m.out = o
        flat = []
        for xi, b, r, po in zip(xs, bns, ress, posts):
            flat += [xi, b.weight, b.bias, r, po]
        return list(self.hb.BnActGroupFn.apply(metas, *flat))

    def conv_bn_act(self, conv, bn, x, residual=None, relu=False, post=None, out=None):
        """conv -> BatchNorm (+residual, ReLU, mask).  In training the conv epilogue accumulates
        the batch statistics, and the normalisation picks them up instead of re-reading the
        conv output.  Lists = independent problems (grouped launches).  out: where the result goes (a `cat_slots`
        channel slice per problem) instead of a fresh tensor."""
        multi = _is_list(x)
        xs = list(x) if multi else [x]
        outs = None if out is None else (list(out) if multi else [out])
        zs = self._conv_bn_group(_lst(conv, len(xs)), _lst(bn, len(xs)), xs, residual, relu, post, outs)
        return zs if multi else zs[0]

    def cat_slots(self, like, widths):
        multi = _is_list(like)
        slots = []
        for t in (like if multi else [like]):
            B, H, W = t.shape[:3]
            buf = torch.empty((B, H, W, sum(widths)), dtype=self.act_dtype, device=t.device)
            views, off = [], 0
            for w in widths:
                views.append(buf[..., off:off + w])
                off += w
            slots.append(views)
        return slots if multi else slots[0]

    def _conv_bn_group(self, convs, bns, xs, residual=None, relu=False, post=None, outs=None):
        n = len(xs)
        ress, relus, posts = _lst(residual, n), _lst(relu, n), _lst(post, n)
        if not torch.is_grad_enabled() and outs is None and not any(b.training for b in bns) and \
                all(po is None for po in posts):
            # inference: the trunk's 3x3 convs carry their BatchNorm (+ residual, ReLU) as the epilogue -- one launch
            # instead of two and no round trip of the conv output through HBM (hip_backend.conv_bn_infer_group)
            metas = [self._bn_meta(b, r) for b, r in zip(bns, relus)]
            zs = self.hb.conv_bn_infer_group(convs, metas, [b.weight for b in bns], [b.bias for b in bns], xs, ress, relus)
            rest = [i for i in range(n) if zs[i] is None]
            if rest and len(rest) < n:
                sub = self._conv_bn_unfused([convs[i] for i in rest], [bns[i] for i in rest], [xs[i] for i in rest],
                                            [ress[i] for i in rest], [relus[i] for i in rest], [None] * len(rest), None)
                for i, z in zip(rest, sub):
                    zs[i] = z
            if not rest or len(rest) < n:
                return zs
        return self._conv_bn_unfused(convs, bns, xs, ress, relus, posts, outs)

    def _conv_bn_unfused(self, convs, bns, xs, ress, relus, posts, outs):
        spec = tuple((c.stride[0], c.padding[0], c.dilation[0], False, bool(b.training)) for c, b in zip(convs, bns))
        flat = []
        for xi, c in zip(xs, convs):
            flat += [xi, c.weight, c.bias]
        ys = self.hb.ConvGroupFn.apply(spec, *flat)
        return self._bn_group(list(ys), bns, ress, relus, posts, outs)

    def add_bn_act(self, a, b, bn, relu=True, post=None):
        C = a.shape[3]
        if not (bn.training and relu and a.dtype == self.act_dtype and b.dtype == self.act_dtype and C % 8 == 0 and C <= 2048):
            # inference (ssa_sum_act, then the evaluation apply) and forms the fused passes are not built for
            return BackendBase.add_bn_act(self, a, b, bn, relu, post)
        return self.hb.AddBnActFn.apply(self._bn_meta(bn, relu), a, b, bn.weight, bn.bias, post)

    def depthwise_conv(self, x, weight, stride, dilation, want_stats=False):
        assert not _is_list(x), "depthwise_conv takes one problem"
        return self.hb.DwConv3x3Fn.apply(x, weight, int(stride), int(dilation), bool(want_stats))

    def depthwise_conv_bn(self, sep, x):
        """Training: the inner BatchNorm's statistics ride on the depthwise kernel (no ssa_bn_stats pass).  Inference
        (SSA_FUSE_EVAL_BN): the inner BatchNorm is the depthwise kernel's epilogue.  (The outer BatchNorm of
        separable_conv_bn_act rides on the pointwise conv either way: conv_bn_act.)"""
        inner, dw = sep.bn, sep.conv1
        assert dw.groups == dw.in_channels == dw.out_channels and dw.kernel_size == (3, 3) and dw.bias is None and \
            dw.padding[0] in (0, dw.dilation[0])
        if not torch.is_grad_enabled() and not inner.training:
            y = self.hb.dwconv_bn_infer(dw.weight, self._bn_meta(inner, False), inner.weight, inner.bias, x, dw.stride[0],
                                        dw.dilation[0])
            if y is not None:
                return y
        y = HipBackend.depthwise_conv(self, x, dw.weight, dw.stride[0], dw.dilation[0], want_stats=inner.training)
        return HipBackend.batch_norm_act(self, y, inner)

    def basic_block(self, blocks, xs):
        ok = torch.is_grad_enabled() and all(
            b.bn1.training and b.bn2.training and b.conv1.bias is None and b.conv2.bias is None and
            b.conv1.stride[0] == 1 and b.conv1.kernel_size[0] == 3 and b.conv1.padding[0] == 1 and
            b.conv1.dilation[0] == 1 and b.conv1.in_channels == b.conv2.out_channels and
            b.conv1.weight.requires_grad for b in blocks)
        if not ok:
            mid = self._conv_bn_group([b.conv1 for b in blocks], [b.bn1 for b in blocks], list(xs), relu=True)
            return self._conv_bn_group([b.conv2 for b in blocks], [b.bn2 for b in blocks], mid, residual=list(xs), relu=True)
        metas = tuple((self._bn_meta(b.bn1, True), self._bn_meta(b.bn2, True)) for b in blocks)
        flat = []
        for b, x in zip(blocks, xs):
            flat += [x, b.conv1.weight, b.bn1.weight, b.bn1.bias, b.conv2.weight, b.bn2.weight, b.bn2.bias]
        return list(self.hb.BasicBlockGroupFn.apply(metas, *flat))

    def fork(self, thunk, tag="fuse", has_bn=True):
        return self.hb.fork(thunk, tag, has_bn)

    def fan_out(self, tensors, counts):
        if not torch.is_grad_enabled() or not any(t.requires_grad for t in tensors) or max(counts) < 2 or \
                any(t.dtype != self.act_dtype or t.numel() % 8 for t in tensors):
            return BackendBase.fan_out(self, tensors, counts)
        flat = self.hb.FanOutGroupFn.apply(tuple(counts), *tensors)
        out, off = [], 0
        for c in counts:
            out.append(list(flat[off:off + c]))
            off += c
        return out

    def end_forward(self):
        self.hb.end_forward()

    def flush_backward(self):
        """Deferred backward work whose results another end-of-backward callback is about to read."""
        self.hb.flush_wgrads(join=True)

    def sum_act(self, tensors, relu=True):
        multi = bool(tensors) and _is_list(tensors[0])
        probs = [list(t) for t in tensors] if multi else [list(tensors)]
        flat = [t for p in probs for t in p]
        zs = self.hb.SumActGroupFn.apply(bool(relu), tuple(len(p) for p in probs), *flat)
        return list(zs) if multi else zs[0]

    def bilinear(self, x, size, out_f32=False):
        multi = _is_list(x)
        xs = list(x) if multi else [x]
        sizes = [tuple(s) for s in size] if (multi and hasattr(size[0], "__len__")) else [tuple(size)] * len(xs)
        outs = [None] * len(xs)
        todo, spec = [], []
        for i, (t, s) in enumerate(zip(xs, sizes)):
            if tuple(t.shape[1:3]) == s and (t.dtype == torch.float32) == bool(out_f32 or t.dtype == torch.float32):
                outs[i] = t
            else:
                todo.append(i)
                spec.append((int(s[0]), int(s[1]), bool(out_f32)))
        if todo:
            ys = self.hb.BilinearGroupFn.apply(tuple(spec), *[xs[i] for i in todo], align_corners=_align_corners())
            for i, y in zip(todo, ys):
                outs[i] = y
        return outs if multi else outs[0]

    def upsample_cat(self, groups):
        counts = tuple(len(g) for g in groups)
        return list(self.hb.UpsampleCatGroupFn.apply(counts, *[t for g in groups for t in g], align_corners=_align_corners()))

    def max_pool3x3s2(self, x):
        return self.hb.MaxPool3x3s2Fn.apply(x)

    def global_avg_pool(self, x):
        return self.hb.GlobalAvgPoolFn.apply(x)

    def max_pool3x3s2_ceil(self, x):
        return self.hb.MaxPool3x3s2CeilFn.apply(x)

    # (C, stride, dilation) -> True: the grouped kernels of csrc/gconv.hip; False: the block-diagonal dense filter
    # through the implicit-GEMM conv.  The ship rule: a shape takes the grouped kernels only where tools/gconvbench.py
    # measured them faster in the sum of forward and both gradients (profiles/gconv_bench.json); shapes never measured
    # take the grouped kernels (32x fewer multiply-adds at 32 groups).  Layer1's 200 x 200 x 128 (Cg = 4) loses on the
    # weight gradient's gather: the captured 800 x 800 step is 16.9 ms with it on the dense route, 17.4 ms without.
    GCONV_ROUTE = {(128, 1, 1): False}

    def grouped_conv(self, x, weight, stride, dilation, groups, want_stats=False):
        assert not _is_list(x), "grouped_conv takes one problem"
        if not self.hb.gconv_supported(x, weight, int(stride), int(dilation), int(groups)) or \
                not self.GCONV_ROUTE.get((weight.shape[0], int(stride), int(dilation)), True):
            # The dense filter is a temporary.  A contiguous fp32 filter would enter the packed-filter cache under its
            # storage address and reset the device job tables of the batched re-pack every step; the next step's
            # begin_step would rebuild them with host-to-device copies, which a stream capture refuses.  A filter that is
            # not contiguous is packed from a copy and never registered (hip_backend._packed_filter).
            return HipBackend.conv2d(self, x, self._block_diagonal(weight, groups, padded=True), None, stride, dilation,
                                     dilation, want_stats=want_stats)
        return self.hb.GConv3x3Fn.apply(x, weight, int(stride), int(dilation), int(groups), bool(want_stats))

    def grouped_conv_bn_act(self, conv, bn, x, relu=False):
        """Training: bn's statistics ride on the grouped conv kernel (or on the dense conv's epilogue), no ssa_bn_stats
        pass; evaluation: the separate apply launch."""
        assert conv.kernel_size == (3, 3) and conv.bias is None and conv.padding[0] == conv.dilation[0] and \
            conv.in_channels == conv.out_channels and conv.padding_mode == "zeros"
        y = HipBackend.grouped_conv(self, x, conv.weight, conv.stride[0], conv.dilation[0], conv.groups,
                                    want_stats=bn.training)
        return HipBackend.batch_norm_act(self, y, bn, None, relu)

    def dil_conv_bn_act(self, conv, bn, x, relu=True, out=None):
        """The kernels of csrc/conv_dil.hip; a list of problems shares one group bracket (one launch forward, one for the
        data gradients).  Training: bn's statistics ride on the conv epilogue.  out: the `cat_slots` channel slice (one
        per problem) the BatchNorm writes; x may itself be such a slice -- b, c, d read `a` out of the cell's output."""
        multi = _is_list(x)
        xs = list(x) if multi else [x]
        n = len(xs)
        convs, bns = _lst(conv, n), _lst(bn, n)
        outs = None if out is None else (list(out) if multi else [out])
        flat = []
        for c, xi in zip(convs, xs):
            self._dil_conv_check(c)
            if xi.dtype != self.act_dtype:
                raise NotImplementedError("the rectangular-dilation conv kernels take NHWC %s" % self.act_dtype)
            flat += [xi, c.weight]
        spec = tuple((tuple(c.dilation), bool(b.training)) for c, b in zip(convs, bns))
        ys = self.hb.DilConvGroupFn.apply(spec, *flat)
        zs = self._bn_group(list(ys), bns, [None] * n, [relu] * n, [None] * n, outs)
        return zs if multi else zs[0]

    def se_gate_add_act(self, se, y, residual=None, relu=True):
        assert not _is_list(y), "se_gate_add_act takes one problem"
        if y.dtype != self.act_dtype or y.shape[3] % 8:
            raise NotImplementedError("the SE gate kernels take NHWC %s with C %% 8 == 0" % self.act_dtype)
        return self.hb.SeGateFn.apply(y, residual, se.fc1.weight, se.fc1.bias, se.fc2.weight, se.fc2.bias, bool(relu))

    def cat(self, tensors):
        if len(tensors) == 2 and self.hb.adjacent_slices(tensors[0], tensors[1]):
            return self.hb.CatViewFn.apply(tensors[0], tensors[1])      # both already lie in one buffer (cat_slots)
        if len(tensors) > 2 and self.hb.slices_of_one_buffer(tensors):
            return self.hb.CatSlotsFn.apply(*tensors)                   # the same for the Dense Prediction Cell's five
        return torch.cat(tensors, dim=3)      # pure data movement

    def to_act(self, x):
        return x.to(self.act_dtype)           # dtype cast only

    def ocr_gather(self, feats, logits):
        return self.hb.OcrGatherFn.apply(feats, logits)

    def ocr_attention(self, q, k, v, scale):
        return self.hb.OcrAttnFn.apply(q, k, v, scale)

    def sigmoid(self, x):
        return self.hb.SigmoidFn.apply(x)

    def bcast_mul(self, a, x):
        return self.hb.BcastMulFn.apply(a, x)

    def attn_blend(self, lo, a, hi):
        return self.hb.AttnBlendFn.apply(lo, a, hi)

    def ewise(self, op, a, b):
        """fp32 a (+|*|/) b, same shapes ('add', 'mul', 'div')."""
        return self.hb.EwiseFn.apply(op, a, b)

    def relu(self, x):
        return self.sum_act([x], relu=True)

    def cross_entropy(self, logits, labels, ignore_index):
        if logits.requires_grad and torch.is_grad_enabled():
            self.hb._no_fp16_training()
        return self.hb.CrossEntropyFn.apply(logits, labels, ignore_index)

    def relax_nll(self, logits, target, classes, ignore_index, border=1, strict=None, upper_bound=1.0,
                  batch_weights=False):
        if logits.requires_grad and torch.is_grad_enabled():
            self.hb._no_fp16_training()
        return self.hb.RelaxNllFn.apply(logits, target, classes, ignore_index, border, strict, upper_bound,
                                        batch_weights)[0]

    def bce_rmi(self, logits, labels, do_rmi, weight_lambda=0.5):
        if logits.requires_grad and torch.is_grad_enabled():
            self.hb._no_fp16_training()
        return self.hb.BceRmiFn.apply(logits, labels, bool(do_rmi), weight_lambda)


def backend():
    global _BACKEND
    if _BACKEND is None:
        _BACKEND = HipBackend()
    return _BACKEND


def _set_backend_for_tests(b):
    """Test-suite hook (tests/test_wiring_cpu.py).  Not used by product code."""
    global _BACKEND
    _BACKEND = b
