"""UNet++ with a ResNet-18 encoder (row U1 breadth of SURVEY.md §8(a)) on hand-written gfx950 kernels.

The reference builds `smp.UnetPlusPlus(encoder_name=backbone, encoder_weights=..., in_channels=num_channels, classes=num_classes)`
(models/model_utilities.py:127-141 of the reference) from segmentation-models-pytorch 0.3.2, a third-party package that is neither
part of the reference nor installed here: this class restates the published architecture of its `unetplusplus/decoder.py` with the
same constructor keywords and the smp / torchvision state-dict key names (tests/unetpp_ref.py is the plain-torch restatement the GPU
tests compare with).  PARITY UNPINNED, like Unet: there is nothing to import; ImageNet weights would need the network and are refused.

Encoder features f1..f5 (64, 64, 128, 256, 512 channels at strides 2..32), features = (f5, f4, f3, f2, f1).  Decoder blocks x_{d}_{l}
for l in 0..3, d in 0..l, plus x_0_4; every block is smp's DecoderBlock (nearest x2 of the input, concat with the skip behind it,
conv3x3-BN-ReLU twice):

    x_d_d = block(features[d], skip = features[d+1])                                         d in 0..3
    x_d_l = block(x_d_{l-1}, skip = cat(x_{d+1}_l, ..., x_l_l, features[l+1]))               l = d + 1 .. 3
    out   = x_0_4(x_0_3) ; logits = conv3x3(out, 16 -> classes, bias)
"""
import functools
from collections import OrderedDict

from . import _lib
from .arena import ArenaModule, bn_spec
from .unet import DECODER_CHANNELS, Unet, encoder_specs

IN_CH = (512, 256, 128, 64, 32)
SKIP_CH = (256, 128, 64, 64, 0)
OUT_CH = DECODER_CHANNELS


def block_table():
    """{name: (input channels, skip channels, output channels)} in smp's construction order: outer loop over l, inner over d, then x_0_4"""
    t = OrderedDict()
    for l in range(4):
        for d in range(l + 1):
            if d == 0:
                t[f"x_{d}_{l}"] = (IN_CH[l], SKIP_CH[l] * (l + 1), OUT_CH[l])
            else:
                t[f"x_{d}_{l}"] = (SKIP_CH[l - 1], SKIP_CH[l] * (l + 1 - d), SKIP_CH[l])
    t["x_0_4"] = (IN_CH[4], 0, OUT_CH[4])
    return t


def forward_order():
    """block names in the order the forward pass computes them: the diagonal x_d_d, then L = l - d = 1, 2, 3, then x_0_4"""
    return [f"x_{d}_{d + L}" for L in range(4) for d in range(4 - L)] + ["x_0_4"]


def unetpp_specs(in_channels, classes):
    p, b, c = OrderedDict(), OrderedDict(), OrderedDict()
    bn = functools.partial(bn_spec, p, b, c)
    encoder_specs(p, bn, in_channels)
    for name, (ci, cs, co) in block_table().items():
        k = f"decoder.blocks.{name}"
        p[f"{k}.conv1.0.weight"] = (co, ci + cs, 3, 3)
        bn(f"{k}.conv1.1", co)
        p[f"{k}.conv2.0.weight"] = (co, co, 3, 3)
        bn(f"{k}.conv2.1", co)
    p["segmentation_head.0.weight"] = (classes, OUT_CH[-1], 3, 3)
    p["segmentation_head.0.bias"] = (classes,)
    return p, b, c


class UnetPlusPlus(Unet):
    """an ArenaModule through Unet, whose weight initialisation and forward() it shares"""

    def __init__(self, encoder_name="resnet18", encoder_depth=5, encoder_weights=None, decoder_use_batchnorm=True,
                 decoder_channels=DECODER_CHANNELS, decoder_attention_type=None, in_channels=3, classes=1, activation=None, precision="bf16"):
        ArenaModule.__init__(self)
        if encoder_name != "resnet18" or encoder_depth != 5 or tuple(decoder_channels) != DECODER_CHANNELS or not decoder_use_batchnorm:
            raise NotImplementedError("UnetPlusPlus (HIP): resnet18 encoder, depth 5, decoder (256,128,64,32,16) with BatchNorm")
        if encoder_weights is not None:
            raise _lib.KsmiError("UnetPlusPlus (HIP): pretrained encoder weights need the network; pass encoder_weights=None and load a state dict")
        if activation is not None or classes > 8 or decoder_attention_type is not None:
            raise NotImplementedError("UnetPlusPlus (HIP): activation=None, classes <= 8, decoder_attention_type=None")
        self.in_channels, self.classes, self.precision = in_channels, classes, precision
        ps, bs, cs = unetpp_specs(in_channels, classes)
        self._setup_arena(ps, bs, cs)
        self._init_weights()

    def plan(self, B, H, W, training, with_backward):
        def build():
            from .unet_plan import UnetPlusPlusPlan
            return UnetPlusPlusPlan(self, B, H, W, self.act_dtype(), training, with_backward)
        return self._cached_plan((B, H, W, self.act_dtype(), bool(training), bool(with_backward)), build)
