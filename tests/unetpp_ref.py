"""Plain-torch restatement (TEST INFRASTRUCTURE) of smp 0.3.2 `UnetPlusPlus(encoder_name="resnet18", encoder_weights=None, in_channels=c,
classes=n)` -- PARITY UNPINNED, like oracle/unet_ref.py: segmentation-models-pytorch is not installed, so this restates the published
architecture of its `unetplusplus/decoder.py` with torch.nn.functional only.

  encoder  torchvision ResNet-18 as in oracle/unet_ref.py (its helpers are imported): f1..f5 = (64, 64, 128, 256, 512) channels at
           strides 2..32; features = (f5, f4, f3, f2, f1)
  decoder  blocks x_{d}_{l}, l in 0..3, d in 0..l, plus x_0_4; each = DecoderBlock: nearest x2 of the input, cat(input, skip),
           Conv3x3(no bias)-BN-ReLU twice
             x_d_d = block(features[d], features[d+1])
             x_d_l = block(x_d_{l-1}, cat(x_{d+1}_l, ..., x_l_l, features[l+1]))
             out   = x_0_4(x_0_3)
  head     Conv2d(16, classes, 3, padding=1)

The channel table is written out here on its own (it is what tests/test_unetpp_cpu.py compares the model's table with).
"""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle.unet_ref import LAYERS, _bn, _bn_spec, _relu, is_buffer, unet_state_dict_spec

IN_CH = (512, 256, 128, 64, 32)
SKIP_CH = (256, 128, 64, 64, 0)
OUT_CH = (256, 128, 64, 32, 16)


def block_channels():
    """{name: (in, skip, out)} in smp's construction order (outer loop l, inner loop d, then x_0_4)"""
    t = OrderedDict()
    for l in range(4):
        for d in range(l + 1):
            if d == 0:
                t[f"x_{d}_{l}"] = (IN_CH[l], SKIP_CH[l] * (l + 1), OUT_CH[l])
            else:
                t[f"x_{d}_{l}"] = (SKIP_CH[l - 1], SKIP_CH[l] * (l + 1 - d), SKIP_CH[l])
    t["x_0_4"] = (IN_CH[4], 0, OUT_CH[4])
    return t


def unetpp_state_dict_spec(in_channels=2, classes=3):
    s = OrderedDict((k, v) for k, v in unet_state_dict_spec(in_channels, classes).items() if k.startswith("encoder."))
    for name, (ci, cs, co) in block_channels().items():
        p = f"decoder.blocks.{name}"
        s[f"{p}.conv1.0.weight"] = (co, ci + cs, 3, 3)
        _bn_spec(s, f"{p}.conv1.1", co)
        s[f"{p}.conv2.0.weight"] = (co, co, 3, 3)
        _bn_spec(s, f"{p}.conv2.1", co)
    s["segmentation_head.0.weight"] = (classes, OUT_CH[-1], 3, 3)
    s["segmentation_head.0.bias"] = (classes,)
    return s


def new_state_dict(in_channels=2, classes=3):
    sd = OrderedDict()
    for k, shp in unetpp_state_dict_spec(in_channels, classes).items():
        sd[k] = torch.zeros(shp, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32)
    return sd


def _encoder(sd, x, training, new_stats, rnd):
    """f1..f5 (oracle/unet_ref.unet_forward's encoder half; rnd = the rounding of a stored tensor, identity in fp32)"""
    t = rnd(F.conv2d(rnd(x), rnd(sd["encoder.conv1.weight"], True), None, stride=2, padding=3))
    t = rnd(_relu(_bn(sd, "encoder.bn1", t, training, new_stats), None, "stem"))
    feats = [t]
    t = F.max_pool2d(t, 3, 2, 1)
    for li, (c, stride) in enumerate(LAYERS):
        for bi in range(2):
            p = f"encoder.layer{li + 1}.{bi}"
            s_ = stride if bi == 0 else 1
            idn = t
            o = rnd(F.conv2d(t, rnd(sd[f"{p}.conv1.weight"], True), None, stride=s_, padding=1))
            o = rnd(_relu(_bn(sd, f"{p}.bn1", o, training, new_stats), None, ""))
            o = _bn(sd, f"{p}.bn2", rnd(F.conv2d(o, rnd(sd[f"{p}.conv2.weight"], True), None, padding=1)), training, new_stats)
            if f"{p}.downsample.0.weight" in sd:
                idn = rnd(F.conv2d(t, rnd(sd[f"{p}.downsample.0.weight"], True), None, stride=s_))
                idn = rnd(_bn(sd, f"{p}.downsample.1", idn, training, new_stats))
            t = rnd(_relu(o + idn, None, ""))
        feats.append(t)
    return feats


def _block(sd, name, x, skip, training, new_stats, rnd):
    p = f"decoder.blocks.{name}"
    y = F.interpolate(x, scale_factor=2, mode="nearest")
    if skip is not None:
        y = torch.cat([y, skip], dim=1)
    y = rnd(F.conv2d(y, rnd(sd[f"{p}.conv1.0.weight"], True), None, padding=1))
    y = rnd(F.relu(_bn(sd, f"{p}.conv1.1", y, training, new_stats)))
    y = rnd(F.conv2d(y, rnd(sd[f"{p}.conv2.0.weight"], True), None, padding=1))
    return rnd(F.relu(_bn(sd, f"{p}.conv2.1", y, training, new_stats)))


def unetpp_forward(sd, x, training=False, inter=None, new_stats=None, rnd=None):
    """logits [B, classes, H, W]; inter: optional dict that receives f1..f5 and every x_d_l.
    rnd(t, is_weight=False): optional rounding of every tensor the HIP plan stores (activations, and their gradients on the way back)
    and of the convolution weights as operands -- oracle/bf16_storage.py's contract; None = plain fp32."""
    if rnd is None:
        rnd = lambda t, w=False: t
    feats = _encoder(sd, x, training, new_stats, rnd)
    if inter is not None:
        inter.update({f"f{i + 1}": f for i, f in enumerate(feats)})
    features = feats[::-1]                  # f5, f4, f3, f2, f1
    xs = {}
    for d in range(4):
        xs[(d, d)] = _block(sd, f"x_{d}_{d}", features[d], features[d + 1], training, new_stats, rnd)
    for L in range(1, 4):
        for d in range(4 - L):
            l = d + L
            cat = torch.cat([xs[(i, l)] for i in range(d + 1, l + 1)] + [features[l + 1]], dim=1)
            xs[(d, l)] = _block(sd, f"x_{d}_{l}", xs[(d, l - 1)], cat, training, new_stats, rnd)
    xs[(0, 4)] = _block(sd, "x_0_4", xs[(0, 3)], None, training, new_stats, rnd)
    if inter is not None:
        inter.update({f"x_{d}_{l}": v for (d, l), v in xs.items()})
    return F.conv2d(xs[(0, 4)], rnd(sd["segmentation_head.0.weight"], True), sd["segmentation_head.0.bias"], padding=1)


def loss_and_grads(sd, x, labels, weights=None, rnd=None, grad_of=()):
    """-> dict: logits, loss, grads {parameter key: gradient}, new_stats (running statistics), inter {f1..f5, x_d_l: activation} and
    inter_grads {name: gradient of that activation, for the names in grad_of}"""
    params = {k: (v.detach().clone().requires_grad_(True) if not is_buffer(k) else v) for k, v in sd.items()}
    new_stats, inter = {}, {}
    logits = unetpp_forward(params, x, training=True, inter=inter, new_stats=new_stats, rnd=rnd)
    for name in grad_of:
        inter[name].retain_grad()
    w = None if weights is None else torch.tensor(list(weights), dtype=logits.dtype)
    loss = F.cross_entropy(logits, labels, weight=w, ignore_index=3)
    loss.backward()
    return {"logits": logits.detach(), "loss": float(loss.detach()), "grads": {k: p.grad for k, p in params.items() if not is_buffer(k)},
            "new_stats": new_stats, "inter": {k: v.detach() for k, v in inter.items()}, "inter_grads": {name: inter[name].grad for name in grad_of}}


def bf16_storage_rnd():
    """the rounding hooks of oracle/bf16_storage.py for unetpp_forward: stored activations rounded both ways, weights straight-through"""
    from oracle.bf16_storage import _RoundSTE, round_both
    return lambda t, w=False: _RoundSTE.apply(t) if w else round_both(t)
