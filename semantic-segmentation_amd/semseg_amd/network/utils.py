"""Trunk selection and the scale-attention head (network/utils.py:102-141,
343-367 of the reference)."""
from collections import OrderedDict

from torch import nn

from .. import ops
from ..config import cfg
from ..nn import Conv2d, Norm2d, BNReLU, conv_bn  # noqa: F401  (BNReLU re-exported like the reference)


def get_trunk(trunk_name, output_stride=8):
    """network/utils.py:102-141 -- the trunks of BASELINE.json's configs: HRNetV2-W48
    (hot path) and ResNet-50 (DeepLabV3+ plumbing config), WiderResNet-38 (scripts/train_cityscapes_deepv3.yml) and
    Xception-71 (deepv3.DeepV3PlusX71), SE-ResNeXt-50 / -101 (deepv3.DeepV3PlusSRNX50 / SRNX101).  The reference returns
    s2_ch = 48 for the SE-ResNeXt trunks although their layer1 delivers 256 channels, and its DeepV3PlusSRNX50 cannot
    run a forward (bot_fine raises); here s2_ch is 256."""
    assert output_stride == 8, "Only stride8 supported right now"
    if trunk_name == "hrnetv2":
        from . import hrnetv2
        backbone = hrnetv2.get_seg_model()
        return backbone, -1, -1, backbone.high_level_ch
    if trunk_name == "resnet-50":
        from .resnet import get_resnet
        return get_resnet(trunk_name, output_stride=output_stride), 256, -1, 2048
    if trunk_name == "wrn38":
        from .wider_resnet import wrn38
        return wrn38(pretrained=True), 128, 256, 4096
    if trunk_name == "xception71":
        from .xception import xception71
        return xception71(output_stride=output_stride, pretrained=True), 64, 128, 2048
    if trunk_name in ("seresnext-50", "seresnext-101"):
        from .resnet import get_resnet
        return get_resnet(trunk_name, output_stride=output_stride), 256, -1, 2048
    raise ValueError("unsupported trunk {} (supported: hrnetv2, resnet-50, wrn38, xception71, seresnext-50, "
                     "seresnext-101)".format(trunk_name))


class ConvBnRelu(nn.Module):
    """conv -> BatchNorm (eps 1e-5) -> ReLU with children conv / bn / relu (network/utils.py:144-159); one
    conv_bn call, so the batch statistics come out of the conv's epilogue."""

    def __init__(self, in_planes, out_planes, kernel_size, stride=1, padding=0, norm_layer=Norm2d):
        super().__init__()
        self.conv = Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = norm_layer(out_planes, eps=1e-5)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return conv_bn(self.conv, self.bn, x, relu=True)


class AttnHead(nn.Sequential):
    """3x3 -> BN -> ReLU -> 3x3 -> BN -> ReLU -> 1x1 -> sigmoid; children are
    named conv0/bn0/re0/conv1/bn1/re1/conv2/sig as in network/utils.py:348-363."""

    def forward(self, x):
        B = ops.backend()
        x = conv_bn(self.conv0, self.bn0, x, relu=True)
        if hasattr(self, "conv1"):
            x = conv_bn(self.conv1, self.bn1, x, relu=True)
        y = self.conv2(x, out_f32=True)                    # [B,H,W,1] fp32 (a list for a list)
        return [B.sigmoid(t) for t in y] if isinstance(y, (list, tuple)) else B.sigmoid(y)


def make_attn_head(in_ch, out_ch):
    bot_ch = cfg.MODEL.SEGATTN_BOT_CH
    od = OrderedDict([("conv0", Conv2d(in_ch, bot_ch, kernel_size=3, padding=1, bias=False)),
                      ("bn0", Norm2d(bot_ch)),
                      ("re0", nn.ReLU(inplace=True))])
    if cfg.MODEL.MSCALE_INNER_3x3:
        od["conv1"] = Conv2d(bot_ch, bot_ch, kernel_size=3, padding=1, bias=False)
        od["bn1"] = Norm2d(bot_ch)
        od["re1"] = nn.ReLU(inplace=True)
    od["conv2"] = Conv2d(bot_ch, out_ch, kernel_size=1, bias=False)
    od["sig"] = nn.Sigmoid()
    return AttnHead(od)


class SegHead(nn.Sequential):
    """3x3 -> BN -> ReLU -> 3x3 -> BN -> ReLU -> 1x1 (children 0..6 as in
    network/utils.py:320-329); returns fp32 logits [B,H,W,classes]."""

    def forward(self, x):
        x = conv_bn(self[0], self[1], x, relu=True)
        x = conv_bn(self[3], self[4], x, relu=True)
        return self[6](x, out_f32=True)


def make_seg_head(in_ch, out_ch):
    """network/utils.py:320-329"""
    bot_ch = cfg.MODEL.SEGATTN_BOT_CH
    return SegHead(Conv2d(in_ch, bot_ch, kernel_size=3, padding=1, bias=False), Norm2d(bot_ch), nn.ReLU(inplace=True),
                   Conv2d(bot_ch, bot_ch, kernel_size=3, padding=1, bias=False), Norm2d(bot_ch), nn.ReLU(inplace=True),
                   Conv2d(bot_ch, out_ch, kernel_size=1, bias=False))
