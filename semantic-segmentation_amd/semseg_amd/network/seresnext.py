"""SE-ResNeXt-50 / -101 (32x4d) trunks at output stride 8 for DeepLabV3+: `network/SEresnext.py:70-118, 170-362` and the
SE-ResNeXt half of get_resnet's dilation surgery (`network/utils.py:48-99`) of the reference, on the HIP operator surface.
State-dict keys are the reference's (`layer0.conv1.weight`, `layer0.bn1.running_mean`, `layer1.0.conv2.weight`,
`layer1.0.se_module.fc1.bias`, `layer1.0.downsample.1.weight`, ...).  The classifier half of SENet (`avg_pool`,
`dropout`, `last_linear`) is not built: get_resnet never takes it over.

The block computes relu(se(bn3(conv3(.))) + residual) (network/SEresnext.py:98-118): the gate scales the block output
per (image, channel) BEFORE the residual add and the ReLU, so it is one operator with them (ops.se_gate_add_act) and bn3
runs without either.  conv2 is the grouped 3x3 conv (32 groups) and goes through ops.grouped_conv_bn_act; nn.Conv2d of
this package stays groups == 1.  layer0's pool is MaxPool2d(3, stride=2, ceil_mode=True) without padding
(ops.max_pool3x3s2_ceil), not the padding-1 pool of the ResNet trunk."""
import math
from collections import OrderedDict

import torch
from torch import nn

from .. import ops
from ..config import cfg
from ..nn import Conv2d, Norm2d, conv_bn


class SEModule(nn.Module):
    """network/SEresnext.py:70-91: fc1 / fc2 are 1x1 convs WITH bias on the [B,C,1,1] channel means."""

    def __init__(self, channels, reduction):
        super().__init__()
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc1 = nn.Conv2d(channels, channels // reduction, kernel_size=1, padding=0)
        self.relu = nn.ReLU(inplace=True)
        self.fc2 = nn.Conv2d(channels // reduction, channels, kernel_size=1, padding=0)
        self.sigmoid = nn.Sigmoid()

    def forward(self, x):
        """The module on its own, as the reference's: x * gate(x)."""
        return ops.backend().se_gate_add_act(self, x, None, relu=False)


class SEResNeXtBottleneck(nn.Module):
    """ResNeXt bottleneck type C with a squeeze-and-excitation module (network/SEresnext.py:170-191); conv2 carries
    the stride and, after the stride-8 surgery, the dilation."""
    expansion = 4

    def __init__(self, inplanes, planes, groups, reduction, stride=1, dilation=1, downsample=None, base_width=4):
        super().__init__()
        width = math.floor(planes * (base_width / 64)) * groups
        self.conv1 = Conv2d(inplanes, width, kernel_size=1, bias=False, stride=1)
        self.bn1 = Norm2d(width)
        # the grouped conv keeps torch's container (the weight is [width, width / groups, 3, 3]); the operator pads
        self.conv2 = nn.Conv2d(width, width, kernel_size=3, stride=stride, padding=dilation, dilation=dilation,
                               groups=groups, bias=False)
        self.bn2 = Norm2d(width)
        self.conv3 = Conv2d(width, planes * 4, kernel_size=1, bias=False)
        self.bn3 = Norm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.se_module = SEModule(planes * 4, reduction=reduction)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        B = ops.backend()
        res = x if self.downsample is None else conv_bn(self.downsample[0], self.downsample[1], x)
        out = conv_bn(self.conv1, self.bn1, x, relu=True)
        out = B.grouped_conv_bn_act(self.conv2, self.bn2, out, relu=True)
        out = conv_bn(self.conv3, self.bn3, out)
        return B.se_gate_add_act(self.se_module, out, res, relu=True)


class SEResNeXtTrunk(nn.Module):
    """get_resnet('seresnext-50' | 'seresnext-101', output_stride=8): SENet(SEResNeXtBottleneck, layers, groups=32,
    reduction=16, inplanes=64, input_3x3=False, downsample_kernel_size=1) with layer3 / layer4 at stride 1 and dilation
    2 / 4 on every conv2 (network/utils.py:71-81; the surgery also resets `downsample.0` of their first blocks to
    stride 1).
    forward(x NHWC [B,H,W,16]) -> (s2 [B,H/4,W/4,256], None, feats [B,H/8,W/8,2048])."""

    def __init__(self, layers=(3, 4, 6, 3), output_stride=8, groups=32, reduction=16, pretrained=True):
        super().__init__()
        assert output_stride == 8, "Only stride8 supported right now"
        self.inplanes = 64
        self.groups, self.reduction = groups, reduction
        self.layer0 = nn.Sequential(OrderedDict([
            ("conv1", Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)),
            ("bn1", Norm2d(64)),
            ("relu1", nn.ReLU(inplace=True)),
            ("pool", nn.MaxPool2d(3, stride=2, ceil_mode=True))]))
        self.layer1 = self._make_layer(64, layers[0], stride=1, dilation=1)
        self.layer2 = self._make_layer(128, layers[1], stride=2, dilation=1)
        self.layer3 = self._make_layer(256, layers[2], stride=1, dilation=2)
        self.layer4 = self._make_layer(512, layers[3], stride=1, dilation=4)
        # (the reference defines no initialiser of its own -- it always loads the ImageNet file: torch's defaults stay)
        if pretrained and cfg.MODEL.SRNX_CHECKPOINT:
            load_srnx_checkpoint(self, cfg.MODEL.SRNX_CHECKPOINT)

    def _make_layer(self, planes, blocks, stride, dilation):
        # network/SEresnext.py:317-335: a 1x1 downsample branch in the first block of every layer (layer1 changes the
        # channel count); in layer3 / layer4 the surgery resets its stride to 1 but the branch stays
        exp = SEResNeXtBottleneck.expansion
        downsample = nn.Sequential(Conv2d(self.inplanes, planes * exp, kernel_size=1, stride=stride, padding=0, bias=False),
                                   Norm2d(planes * exp))
        layers = [SEResNeXtBottleneck(self.inplanes, planes, self.groups, self.reduction, stride, dilation, downsample)]
        self.inplanes = planes * exp
        for _ in range(1, blocks):
            layers.append(SEResNeXtBottleneck(self.inplanes, planes, self.groups, self.reduction, 1, dilation))
        return nn.Sequential(*layers)

    def forward(self, x):
        x = conv_bn(self.layer0.conv1, self.layer0.bn1, x, relu=True)
        x = ops.backend().max_pool3x3s2_ceil(x)
        x = self.layer1(x)
        s2 = x
        x = self.layer2(x)
        x = self.layer3(x)
        x = self.layer4(x)
        return s2, None, x


def load_srnx_checkpoint(net, path):
    """cfg.MODEL.SRNX_CHECKPOINT: a local file, read the way X71_CHECKPOINT is (network/xception.py:270-279): a plain
    state dict or checkpoint['model_dict'], `module.` stripped, laid over the current state dict and loaded with
    strict=False -- keys the trunk does not have (`last_linear.*` of the ImageNet classifier) are ignored, keys the file
    lacks keep their initial values.  Nothing is ever downloaded."""
    ckpt = torch.load(path, map_location="cpu")
    ckpt = ckpt.get("model_dict", ckpt)
    # only the LEADING `module.` of a DataParallel wrapper: `se_module.` is part of this trunk's own key names
    model_dict = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in ckpt.items()}
    state_dict = net.state_dict()
    state_dict.update(model_dict)
    net.load_state_dict(state_dict, strict=False)
