"""WiderResNet-38 (A2, dilated, output stride 8) trunk for DeepLabV3+: `network/wider_resnet.py:71-185,
269-379, 398-434` of the reference on the HIP operator surface.  State-dict keys are the reference's
(`mod1.conv1.weight`, `mod2.block1.bn1.0.weight`, `mod6.block1.convs.bn3.0.running_mean`,
`mod4.block1.proj_conv.weight`, ...); like the reference's `wrn38` wrapper it has no `bn_out` and no classifier.

The blocks are PRE-activation: a block starts with BatchNorm + ReLU on the residual sum of the block before
(network/wider_resnet.py:172-185), which also is its shortcut.  The trunk's forward is therefore written flat over
the blocks: a block leaves the pair (last conv output, shortcut) open, and the head of the next block closes it with
`ops.add_bn_act` -- the sum is stored once, its batch statistics are taken in the same pass, and in backward the
shortcut's gradient joins bn1's inside the pass.  Where no BatchNorm follows (in front of pool3, at the trunk output)
a plain `sum_act(relu=False)` closes the pair."""
from collections import OrderedDict

import torch
from torch import nn

from .. import ops
from ..config import cfg
from ..nn import Conv2d, BNReLU, conv_bn


class IdentityResidualBlock(nn.Module):
    """network/wider_resnet.py:71-185 (groups = 1).  channels: two values = two 3x3 convs, three = the bottleneck
    1x1 / 3x3 / 1x1.  dropout: probability of the Dropout2d behind the last BatchNorm + ReLU, or None."""

    def __init__(self, in_channels, channels, stride=1, dilation=1, dropout=None):
        super().__init__()
        if len(channels) not in (2, 3):
            raise ValueError("channels must contain either two or three values")
        self.is_bottleneck = len(channels) == 3
        self.bn1 = BNReLU(in_channels)
        if not self.is_bottleneck:
            layers = [("conv1", Conv2d(in_channels, channels[0], 3, stride=stride, padding=dilation, bias=False,
                                       dilation=dilation)),
                      ("bn2", BNReLU(channels[0])),
                      ("conv2", Conv2d(channels[0], channels[1], 3, stride=1, padding=dilation, bias=False,
                                       dilation=dilation))]
            if dropout is not None:
                layers = layers[0:2] + [("dropout", nn.Dropout2d(p=dropout))] + layers[2:]
        else:
            layers = [("conv1", Conv2d(in_channels, channels[0], 1, stride=stride, padding=0, bias=False)),
                      ("bn2", BNReLU(channels[0])),
                      ("conv2", Conv2d(channels[0], channels[1], 3, stride=1, padding=dilation, bias=False,
                                       dilation=dilation)),
                      ("bn3", BNReLU(channels[1])),
                      ("conv3", Conv2d(channels[1], channels[2], 1, stride=1, padding=0, bias=False))]
            if dropout is not None:
                layers = layers[0:4] + [("dropout", nn.Dropout2d(p=dropout))] + layers[4:]
        self.convs = nn.Sequential(OrderedDict(layers))
        if stride != 1 or in_channels != channels[-1]:
            self.proj_conv = Conv2d(in_channels, channels[-1], 1, stride=stride, padding=0, bias=False)

    def _mask(self, x, width):
        """The Dropout2d mask of this block as a per-(image, channel) multiplier (drawn as SpatialOCR_Module._mask
        draws it), handed to the BatchNorm pass as `post`."""
        drop = getattr(self.convs, "dropout", None)
        if drop is None or not (self.training and drop.p > 0):
            return None
        keep = 1.0 - drop.p
        return (torch.rand(x.shape[0], width, device=x.device) < keep).to(torch.float32) / keep

    def last_norm(self):
        return self.convs.bn3[0] if self.is_bottleneck else self.convs.bn2[0]

    def body(self, s, y):
        """s: the block input (None for the very first block, whose input has no consumer but bn1); y = relu(bn1(s)).
        Returns the open pair (last conv output, shortcut)."""
        c = self.convs
        if hasattr(self, "proj_conv"):
            y, y_proj = ops.backend().fan_out([y], [2])[0]
            shortcut = self.proj_conv(y_proj)
        else:
            shortcut = s
        if not self.is_bottleneck:
            out = conv_bn(c.conv1, c.bn2[0], y, relu=True, post=self._mask(y, c.conv1.out_channels))
            return c.conv2(out), shortcut
        out = conv_bn(c.conv1, c.bn2[0], y, relu=True)
        out = conv_bn(c.conv2, c.bn3[0], out, relu=True, post=self._mask(y, c.conv2.out_channels))
        return c.conv3(out), shortcut

    def forward(self, x):
        """The block on its own (network/wider_resnet.py:172-185): x -> x_next."""
        B = ops.backend()
        out, shortcut = self.body(x, self.bn1[0](x, relu=True))
        return B.sum_act([out, shortcut], relu=False)


_CHANNELS = [(128, 128), (256, 256), (512, 512), (512, 1024), (512, 1024, 2048), (1024, 2048, 4096)]


class wrn38(nn.Module):
    """WiderResNetA2(structure [3, 3, 6, 3, 1, 1], dilation=True) behind the reference's `wrn38` wrapper
    (network/wider_resnet.py:398-434): stride 2 at mod4.block1, dilation 2 in mod5 and 4 in mod6 / mod7,
    Dropout2d 0.3 / 0.5 in mod6 / mod7.
    forward(x NHWC [B,H,W,16]) -> (s2 [B,H/2,W/2,128], s4 [B,H/4,W/4,256], feats [B,H/8,W/8,4096])."""
    structure = (3, 3, 6, 3, 1, 1)

    def __init__(self, pretrained=True):
        super().__init__()
        self.mod1 = nn.Sequential(OrderedDict([("conv1", Conv2d(3, 64, 3, stride=1, padding=1, bias=False))]))
        in_channels = 64
        for mod_id, num in enumerate(self.structure):
            blocks = []
            for block_id in range(num):
                dil = 2 if mod_id == 3 else (4 if mod_id > 3 else 1)
                stride = 2 if block_id == 0 and mod_id == 2 else 1
                drop = 0.3 if mod_id == 4 else (0.5 if mod_id == 5 else None)
                blocks.append(("block%d" % (block_id + 1),
                               IdentityResidualBlock(in_channels, _CHANNELS[mod_id], stride=stride, dilation=dil,
                                                     dropout=drop)))
                in_channels = _CHANNELS[mod_id][-1]
            if mod_id < 2:
                self.add_module("pool%d" % (mod_id + 2), nn.MaxPool2d(3, stride=2, padding=1))
            self.add_module("mod%d" % (mod_id + 2), nn.Sequential(OrderedDict(blocks)))
        if pretrained and cfg.MODEL.WRN38_CHECKPOINT:
            load_wrn38_checkpoint(self, cfg.MODEL.WRN38_CHECKPOINT)

    def _run(self, blocks, x, pair):
        """The blocks of one module.  x: a tensor no open pair leads to (module input behind a pool), else None and
        `pair` = the open (conv output, shortcut) of the block before.  Returns (inputs of the blocks, open pair)."""
        B = ops.backend()
        inputs = []
        for blk in blocks:
            if pair is None:
                s, y = x, blk.bn1[0](x, relu=True)
            else:
                s, y = B.add_bn_act(pair[0], pair[1], blk.bn1[0], relu=True)
            inputs.append(s)
            pair = blk.body(s, y)
        return inputs, pair

    def forward(self, x):
        B = ops.backend()
        x = self.mod1.conv1(x)
        _, pair = self._run(self.mod2, B.max_pool3x3s2(x), None)
        s2 = B.sum_act(list(pair), relu=False)
        s2, s2_pool = B.fan_out([s2], [2])[0]
        _, pair = self._run(self.mod3, B.max_pool3x3s2(s2_pool), None)
        inputs, pair = self._run(self.mod4, None, pair)
        s4 = inputs[0]                                  # mod3's output = the sum at the head of mod4.block1
        for mod in (self.mod5, self.mod6, self.mod7):
            _, pair = self._run(mod, None, pair)
        return s2, s4, B.sum_act(list(pair), relu=False)


def load_wrn38_checkpoint(net, path):
    """cfg.MODEL.WRN38_CHECKPOINT (network/wider_resnet.py:405-409): the ImageNet classifier's
    checkpoint['state_dict'] saved from a DataParallel wrapper -- `module.` stripped, the classifier and `bn_out`
    (which the wrapper drops) left out, everything else loaded strictly."""
    checkpoint = torch.load(path, map_location="cpu")
    sd = {}
    for k, v in checkpoint["state_dict"].items():
        k = k[len("module."):] if k.startswith("module.") else k
        if k.startswith("classifier.") or k.startswith("bn_out."):
            continue
        sd[k] = v
    net.load_state_dict(sd, strict=True)
