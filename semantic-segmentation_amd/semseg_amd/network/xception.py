"""Aligned Xception-71 trunk (output stride 8) for DeepLabV3+: `network/xception.py:24-279` of the reference on the HIP
operator surface.  State-dict keys are the reference's (`block1.rep.0.conv1.weight`, `block1.rep.0.bn.weight`,
`block1.rep.0.pointwise.weight`, `block1.rep.1.weight`, `block1.skip.weight`, `block1.skipbn.*`, `block4.rep.1.conv1.weight`,
`conv3.conv1.weight`, ...): `rep` keeps the reference's ReLU placeholders, so the indices inside it depend on
start_with_relu as they do there.

Where the ReLUs go.  The reference's blocks share ONE nn.ReLU(inplace=True); as the first element of `rep` it rewrites
the block input, so a block with start_with_relu computes rep'(relu(inp)) + skip(relu(inp)) (network/xception.py:56-61,
96-105: the skip branch reads `inp` after `rep` ran).  Every ReLU of the trunk therefore sits directly behind a
BatchNorm (+ residual add) and is that op's epilogue here: inside a block behind each SeparableConv2d + BatchNorm but the
last, and the ReLU a block is followed by -- the trunk's own (behind block1, block20) or the leading one of the next
block -- behind the block's last BatchNorm + skip add.  The depthwise kernel never needs a ReLU on its input."""
import math

import torch
from torch import nn

from .. import ops
from ..config import cfg
from ..nn import Conv2d, Norm2d, conv_bn


class SeparableConv2d(nn.Module):
    """network/xception.py:24-40: depthwise 3x3 (`conv1`, padding = dilation: fixed_padding is symmetric for a 3x3
    kernel) -> `bn` -> 1x1 `pointwise`.  `conv1` keeps nn.Conv2d's container (padding 0 like the reference's; the
    operator pads)."""

    def __init__(self, inplanes, planes, kernel_size=3, stride=1, dilation=1, bias=False):
        super().__init__()
        assert kernel_size == 3 and not bias
        self.conv1 = nn.Conv2d(inplanes, inplanes, kernel_size, stride, 0, dilation, groups=inplanes, bias=bias)
        self.bn = Norm2d(inplanes)
        self.pointwise = Conv2d(inplanes, planes, 1, 1, 0, 1, 1, bias=bias)

    def forward(self, x):
        """The module on its own, as the reference's: no BatchNorm behind the pointwise conv."""
        return self.pointwise(ops.backend().depthwise_conv_bn(self, x))


class Block(nn.Module):
    """network/xception.py:43-107."""

    def __init__(self, inplanes, planes, reps, stride=1, dilation=1, start_with_relu=True, grow_first=True,
                 is_last=False):
        super().__init__()
        if planes != inplanes or stride != 1:
            self.skip = Conv2d(inplanes, planes, 1, stride=stride, bias=False)
            self.skipbn = Norm2d(planes)
        else:
            self.skip = None
        self.relu = nn.ReLU(inplace=True)
        self.start_with_relu = start_with_relu
        rep = []
        filters = inplanes
        if grow_first:
            rep += [self.relu, SeparableConv2d(inplanes, planes, 3, 1, dilation), Norm2d(planes)]
            filters = planes
        for _ in range(reps - 1):
            rep += [self.relu, SeparableConv2d(filters, filters, 3, 1, dilation), Norm2d(filters)]
        if not grow_first:
            rep += [self.relu, SeparableConv2d(inplanes, planes, 3, 1, dilation), Norm2d(planes)]
        if stride != 1:
            rep += [self.relu, SeparableConv2d(planes, planes, 3, 2), Norm2d(planes)]
        if stride == 1 and is_last:
            rep += [self.relu, SeparableConv2d(planes, planes, 3, 1), Norm2d(planes)]
        if not start_with_relu:
            rep = rep[1:]
        self.rep = nn.Sequential(*rep)

    def pairs(self):
        """The (SeparableConv2d, BatchNorm) pairs of `rep`, in order."""
        mods = [m for m in self.rep if not isinstance(m, nn.ReLU)]
        return list(zip(mods[0::2], mods[1::2]))

    def body(self, x, relu_out):
        """x: the block input AFTER the leading ReLU (if the block has one).  relu_out: the ReLU the block's output
        meets next, folded into the last BatchNorm + skip add."""
        B = ops.backend()
        x, x_skip = B.fan_out([x], [2])[0]
        skip = x_skip if self.skip is None else conv_bn(self.skip, self.skipbn, x_skip)
        pairs = self.pairs()
        for sep, bn in pairs[:-1]:
            x = B.separable_conv_bn_act(sep, bn, x, relu=True)
        sep, bn = pairs[-1]
        return B.separable_conv_bn_act(sep, bn, x, residual=skip, relu=relu_out)

    def forward(self, inp):
        """The block on its own (network/xception.py:96-107), the in-place leading ReLU included."""
        return self.body(ops.backend().relu(inp) if self.start_with_relu else inp, False)


class xception71(nn.Module):
    """Modified Aligned Xception (network/xception.py:110-268) at output stride 8: middle flow dilation 2, exit flow
    (2, 4), exit stride 1.
    forward(x NHWC [B,H,W,16]) -> (str2 [B,H/2,W/2,64], str4 [B,H/4,W/4,128], feats [B,H/8,W/8,2048])."""

    def __init__(self, output_stride=8, pretrained=True):
        super().__init__()
        assert output_stride == 8, "Only stride8 supported right now"
        self.output_stride = output_stride
        mid, exit_dil = 2, (2, 4)
        self.conv1 = Conv2d(3, 32, 3, stride=2, padding=1, bias=False)
        self.bn1 = Norm2d(32)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = Conv2d(32, 64, 3, stride=1, padding=1, bias=False)
        self.bn2 = Norm2d(64)
        self.block1 = Block(64, 128, reps=2, stride=2, start_with_relu=False)
        self.block2 = Block(128, 256, reps=2, stride=1, start_with_relu=False, grow_first=True)
        self.block3 = Block(256, 728, reps=2, stride=2, start_with_relu=True, grow_first=True, is_last=True)
        for i in range(4, 20):
            self.add_module("block%d" % i, Block(728, 728, reps=3, stride=1, dilation=mid, start_with_relu=True,
                                                 grow_first=True))
        self.block20 = Block(728, 1024, reps=2, stride=1, dilation=exit_dil[0], start_with_relu=True, grow_first=False,
                             is_last=True)
        self.conv3 = SeparableConv2d(1024, 1536, 3, stride=1, dilation=exit_dil[1])
        self.bn3 = Norm2d(1536)
        self.conv4 = SeparableConv2d(1536, 1536, 3, stride=1, dilation=exit_dil[1])
        self.bn4 = Norm2d(1536)
        self.conv5 = SeparableConv2d(1536, 2048, 3, stride=1, dilation=exit_dil[1])
        self.bn5 = Norm2d(2048)
        self._init_weight()
        if pretrained and cfg.MODEL.X71_CHECKPOINT:
            load_x71_checkpoint(self, cfg.MODEL.X71_CHECKPOINT)

    def forward(self, x):
        B = ops.backend()
        x = conv_bn(self.conv1, self.bn1, x, relu=True)
        str2 = conv_bn(self.conv2, self.bn2, x, relu=True)
        str2, x = B.fan_out([str2], [2])[0]
        str4 = self.block1.body(x, True)                    # str4 = relu(block1(str2))
        str4, x = B.fan_out([str4], [2])[0]
        # every block from here on is followed by a block that starts with the in-place ReLU (block20: by the trunk's)
        for i in range(2, 21):
            x = getattr(self, "block%d" % i).body(x, True)
        x = B.separable_conv_bn_act(self.conv3, self.bn3, x, relu=True)
        x = B.separable_conv_bn_act(self.conv4, self.bn4, x, relu=True)
        x = B.separable_conv_bn_act(self.conv5, self.bn5, x, relu=True)
        return str2, str4, x

    def _init_weight(self):
        """network/xception.py:258-268."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                n = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / n))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()


def load_x71_checkpoint(net, path):
    """cfg.MODEL.X71_CHECKPOINT (network/xception.py:270-279): checkpoint['model_dict'] saved from a DataParallel
    wrapper -- `module.` stripped, laid over the current state dict and loaded with strict=False (keys the trunk does
    not have are ignored, keys the file lacks keep their initial values)."""
    ckpt = torch.load(path, map_location="cpu")
    model_dict = {k.replace("module.", ""): v for k, v in ckpt["model_dict"].items()}
    state_dict = net.state_dict()
    state_dict.update(model_dict)
    net.load_state_dict(state_dict, strict=False)
