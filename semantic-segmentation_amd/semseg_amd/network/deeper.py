"""Panoptic-DeepLab style decoder on a stride-8 trunk (network/deeper.py of the reference): the `--arch` names
`deeper.DeeperW38` and `deeper.DeeperX71`.  Same factory names, call contract and state_dict keys (`trunk`, `aspp`,
`convs2`, `convs4`, `conv_up1`, `conv_up2`, `conv_up3`, `conv_up5`); NHWC 16-bit storage on the HIP kernels.  The two
5x5 ConvBnRelu layers (conv_up2 320->256 at stride 4, conv_up3 288->256 at stride 2) are more arithmetic than the rest
of either network and run on csrc/conv_halo5.hip.

Not carried over: `DeeperEffB4` (network/deeper.py:90-91) -- the reference ships no EfficientNet trunk file and its
own get_trunk raises for 'efficientnet_b4'."""
from torch import nn

from .. import ops
from ..nn import Conv2d
from .deepv3 import get_aspp
from .mynn import Upsample2
from .utils import ConvBnRelu, get_trunk


class DeeperDecoder(nn.Module):
    """The layers DeeperS8 and mscale.MscaleDeeper share (network/deeper.py:50-55, network/mscale.py:379-384); mixed
    into both, so the keys carry no extra prefix."""

    def _make_decoder(self, s2_ch, s4_ch, aspp_out_ch, num_classes):
        self.convs2 = Conv2d(s2_ch, 32, kernel_size=1, bias=False)
        self.convs4 = Conv2d(s4_ch, 64, kernel_size=1, bias=False)
        self.conv_up1 = Conv2d(aspp_out_ch, 256, kernel_size=1, bias=False)
        self.conv_up2 = ConvBnRelu(256 + 64, 256, kernel_size=5, padding=2)
        self.conv_up3 = ConvBnRelu(256 + 32, 256, kernel_size=5, padding=2)
        self.conv_up5 = Conv2d(256, num_classes, kernel_size=1, bias=False)

    def _decode(self, aspp, s2_features, s4_features):
        """aspp at stride 8 -> the 256-channel features at stride 2 (network/deeper.py:62-71)."""
        B = ops.backend()
        s2_features = self.convs2(s2_features)
        s4_features = self.convs4(s4_features)
        x = Upsample2(self.conv_up1(aspp))
        x = self.conv_up2(B.cat([x, s4_features]))
        x = Upsample2(x)
        return self.conv_up3(B.cat([x, s2_features]))


class DeeperS8(DeeperDecoder):
    """Panoptic-DeepLab style semantic segmentation network, stride 8 only (network/deeper.py:36-79)."""

    def __init__(self, num_classes, trunk="wrn38", criterion=None):
        super().__init__()
        self.criterion = criterion
        self.trunk, s2_ch, s4_ch, high_level_ch = get_trunk(trunk_name=trunk, output_stride=8)
        self.aspp, aspp_out_ch = get_aspp(high_level_ch, bottleneck_ch=256, output_stride=8)
        self._make_decoder(s2_ch, s4_ch, aspp_out_ch, num_classes)

    def forward(self, inputs):
        assert "images" in inputs
        B = ops.backend()
        B.begin_step(inputs["images"].device)
        images = inputs["images"]
        x = B.image_to_nhwc(images, (images.shape[2], images.shape[3]))
        s2_features, s4_features, final_features = self.trunk(x)
        up3 = self._decode(self.aspp(final_features), s2_features, s4_features)
        out = Upsample2(self.conv_up5(up3, out_f32=True), out_f32=True)      # [B,H,W,classes] fp32
        B.end_forward()
        out = out.permute(0, 3, 1, 2)
        if self.training:
            assert "gts" in inputs
            return self.criterion(out, inputs["gts"])
        return {"pred": out}


def DeeperW38(num_classes, criterion, s2s4=True):
    return DeeperS8(num_classes, criterion=criterion, trunk="wrn38")


def DeeperX71(num_classes, criterion, s2s4=True):
    return DeeperS8(num_classes, criterion=criterion, trunk="xception71")


def DeeperEffB4(num_classes, criterion, s2s4=True):
    raise ValueError("deeper.DeeperEffB4: no EfficientNet trunk (the reference's get_trunk raises for it as well)")
