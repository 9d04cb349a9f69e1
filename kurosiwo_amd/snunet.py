"""SNUNet-ECAM on hand-written gfx950 kernels (rows S1-S9 of SURVEY.md §8(a)).

Drop-in for the reference class (/root/reference/models/snunet.py:65-153): same
constructor, same state-dict keys (236), same ``model(xA, xB) -> logits [B,3,H,W]``
contract with autograd, ``.train()/.eval()``, BatchNorm running statistics.

MI355X-first design:
  * every parameter lives in one flat fp32 arena (and every gradient in a second one)
    so the optimiser step and the data-parallel all-reduce are single flat operations;
  * a *plan* (static launch list over preallocated NHWC activations) is built once per
    (batch, H, W, dtype, mode) and replayed -- capturable in a HIP graph;
  * torch.cat is never materialised (virtual concat inside the implicit-GEMM K loop),
    BatchNorm-apply + ReLU are fused into the consumer conv's operand load, BN statistics
    are produced by the conv epilogue.
There is no CPU/eager fallback: a CPU tensor raises.
"""
import math
import os
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _lib
from .arena import ArenaModule, bn_spec
from .runtime import require_gpu

BN_EPS, BN_MOMENTUM = 1e-5, 0.1


def _blocks(n, c):
    f = [n, 2 * n, 4 * n, 8 * n, 16 * n]
    # (name, in_ch, out_ch) in the registration order of snunet.py:75-103 ; ("up", name, ch)
    return [
        ("block", "conv0_0", c, f[0]), ("block", "conv1_0", f[0], f[1]), ("up", "Up1_0", f[1]),
        ("block", "conv2_0", f[1], f[2]), ("up", "Up2_0", f[2]), ("block", "conv3_0", f[2], f[3]),
        ("up", "Up3_0", f[3]), ("block", "conv4_0", f[3], f[4]), ("up", "Up4_0", f[4]),
        ("block", "conv0_1", f[0] * 2 + f[1], f[0]), ("block", "conv1_1", f[1] * 2 + f[2], f[1]),
        ("up", "Up1_1", f[1]), ("block", "conv2_1", f[2] * 2 + f[3], f[2]), ("up", "Up2_1", f[2]),
        ("block", "conv3_1", f[3] * 2 + f[4], f[3]), ("up", "Up3_1", f[3]),
        ("block", "conv0_2", f[0] * 3 + f[1], f[0]), ("block", "conv1_2", f[1] * 3 + f[2], f[1]),
        ("up", "Up1_2", f[1]), ("block", "conv2_2", f[2] * 3 + f[3], f[2]), ("up", "Up2_2", f[2]),
        ("block", "conv0_3", f[0] * 4 + f[1], f[0]), ("block", "conv1_3", f[1] * 4 + f[2], f[1]),
        ("up", "Up1_3", f[1]), ("block", "conv0_4", f[0] * 5 + f[1], f[0]),
    ]


def snunet_specs(in_channels, out_ch, n):
    """(params, fp32 buffers, int64 counters) keyed and ordered as the reference's state dict."""
    p, b, c = OrderedDict(), OrderedDict(), OrderedDict()
    for item in _blocks(n, in_channels):
        if item[0] == "block":
            _, name, cin, cout = item
            for conv, bn, ci in (("conv1", "bn1", cin), ("conv2", "bn2", cout)):
                p[f"{name}.{conv}.weight"] = (cout, ci, 3, 3)
                p[f"{name}.{conv}.bias"] = (cout,)
                bn_spec(p, b, c, f"{name}.{bn}", cout)
        else:
            _, name, ch = item
            p[f"{name}.up.weight"] = (ch, ch, 2, 2)
            p[f"{name}.up.bias"] = (ch,)
    p["ca.fc1.weight"] = (4 * n // 16, 4 * n, 1, 1)
    p["ca.fc2.weight"] = (4 * n, 4 * n // 16, 1, 1)
    p["ca1.fc1.weight"] = (n // 4, n, 1, 1)
    p["ca1.fc2.weight"] = (n, n // 4, 1, 1)
    p["conv_final.weight"] = (out_ch, 4 * n, 1, 1)
    p["conv_final.bias"] = (out_ch,)
    return p, b, c


class SNUNet_ECAM(ArenaModule):
    ARENA_ALIGN = 4            # no bf16 mirror; the layout is kept so that dumps and checkpoints of flat_params compare with earlier builds

    def __init__(self, in_channels, out_ch, base_channel=32, precision="bf16"):
        super().__init__()
        if out_ch != 3:
            raise _lib.KsmiError("SNUNet_ECAM (HIP): out_ch must be 3 (num_classes of the reference configs)")
        self.in_channels, self.out_ch, self.base_channel = in_channels, out_ch, base_channel
        self.precision = precision            # "bf16" (performance) | "fp32" (parity)
        # optional: BatchNorm statistics over the global batch under data parallelism (snunet_plan.SNUNetPlan.sync_bn; KSMI_SYNC_BN=1 or
        # configs["sync_bn"]); default = the reference's per-process BatchNorm
        self.sync_bn = os.environ.get("KSMI_SYNC_BN", "0") == "1"
        self._setup_arena(*snunet_specs(in_channels, out_ch, base_channel))
        self._init_parameters()
        self._raw_norm = None
        self._raw_version = 0          # bumped whenever the pipeline values change: part of the plan cache key

    # ------------------------------------------------------------------ raw-tile input
    def set_input_pipeline(self, mean=None, std=None, clamp=None):
        """Fold the Dataset's per-tile pipeline (dataset/Dataset.py:164-168 clamp to [0, clamp_input] + nan_to_num(clamp_input),
        :193-198 Normalize) into the image load of conv0_0.conv1: after this call forward() takes RAW tiles (NaNs included).
        `mean`, `std`: per input channel; `clamp`: a float (every channel) or per channel, a negative entry = no clamp for that
        channel (DEM: NaN -> mean).  set_input_pipeline() with no arguments returns to normalised inputs."""
        if mean is None:
            if self._raw_norm is not None:
                self._drop_raw_plans()
            self._raw_norm = None
            return self
        mean = [float(v) for v in mean]
        std = [float(v) for v in std]
        clamp = [float(clamp)] * len(mean) if not hasattr(clamp, "__len__") else [float(v) for v in clamp]
        if not (len(mean) == len(std) == len(clamp) == self.in_channels):
            raise ValueError(f"set_input_pipeline: {self.in_channels} input channels, got {len(mean)} means, {len(std)} stds, {len(clamp)} clamps")
        if any(v == 0.0 for v in std):
            raise ValueError("set_input_pipeline: a zero standard deviation")
        new = torch.tensor([mean, std, clamp], dtype=torch.float32)
        if self._raw_norm is None or not torch.equal(self._raw_norm.cpu(), new):       # (same values: the plans built on them stay valid)
            self._drop_raw_plans()                 # plans hold raw device pointers into the old tensor
            self._raw_norm = new
            self._raw_version += 1
        return self

    def _drop_raw_plans(self):
        for k in [k for k in self._plans if k[6] is not None]:
            del self._plans[k]

    def _raw_ptrs(self, dev):
        """(mean, std, clamp) device pointers for the first conv, or three nulls"""
        if self._raw_norm is None:
            return 0, 0, 0
        if self._raw_norm.device != dev:
            self._raw_norm = self._raw_norm.to(dev)
        base, step = self._raw_norm.data_ptr(), self.in_channels * 4
        return base, base + step, base + 2 * step

    def _init_parameters(self):
        """snunet.py:110-115: kaiming_normal_(fan_out, relu) on every nn.Conv2d weight, BN gamma=1
        beta=0; conv biases and ConvTranspose2d keep the PyTorch default init."""
        with torch.no_grad():
            for key, shp in self._pspec.items():
                p = self._p(key).view(shp)
                if ".up." in key:
                    if key.endswith("weight"):
                        nn.init.kaiming_uniform_(p, a=math.sqrt(5))
                    else:
                        fan_in = self._pspec[key.replace("bias", "weight")][1] * 4
                        p.uniform_(-1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))
                elif ".bn" in key:
                    p.fill_(1.0 if key.endswith("weight") else 0.0)
                elif key.endswith("weight"):
                    nn.init.kaiming_normal_(p, mode="fan_out", nonlinearity="relu")
                else:
                    w = self._pspec[key.replace("bias", "weight")]
                    fan_in = w[1] * w[2] * w[3]
                    p.uniform_(-1 / math.sqrt(fan_in), 1 / math.sqrt(fan_in))

    # ------------------------------------------------------------------ forward
    def plan(self, B, H, W, training, with_backward, tail=0):
        # the key carries a version counter, not id(tensor): _raw_ptrs() moves the tensor to the device (a new object), and a freed
        # tensor's id can be handed out again
        key = (B, H, W, self.act_dtype(), bool(training), bool(with_backward), None if self._raw_norm is None else self._raw_version, tail,
               bool(self.sync_bn))

        def build():
            from .snunet_plan import SNUNetPlan
            plan = SNUNetPlan(self, B, H, W, self.act_dtype(), training, with_backward, tail=tail, sync_bn=self.sync_bn)
            if self._raw_norm is not None:
                plan.keep.append(self._raw_norm)   # the plan's launches hold data_ptr()s into it
            return plan
        return self._cached_plan(key, build)

    def forward(self, xA, xB, dem=None):
        """xA, xB: the two dates [B,C,H,W].  dem (optional, [B,Cd,H,W]): channels shared by both dates; forward(xA, xB, dem) equals
        forward(cat(xA, dem), cat(xB, dem)) (the trainer's input assembly, change_detection_trainer.py:117-133) without the copies."""
        require_gpu(xA)
        tail = 0 if dem is None else dem.shape[1]
        if xA.shape != xB.shape or xA.dim() != 4 or xA.shape[1] + tail != self.in_channels or (dem is not None and (
                dem.dim() != 4 or dem.shape[0] != xA.shape[0] or dem.shape[2:] != xA.shape[2:])):
            raise ValueError(f"expected two [B,{self.in_channels - tail},H,W] tensors" + (f" and a [B,{tail},H,W] tail" if tail else "") +
                             f", got {tuple(xA.shape)} {tuple(xB.shape)}" + (f" {tuple(dem.shape)}" if tail else ""))
        B, _, H, W = xA.shape
        if H % 16 or W % 16:
            raise ValueError("H and W must be multiples of 16 (four 2x2 max-pools)")
        want_grad = self._wants_grad()
        plan = self.plan(B, H, W, self.training, want_grad, tail)
        return self._apply_plan(plan, want_grad, xA.contiguous().float(), xB.contiguous().float(),
                                None if dem is None else dem.contiguous().float())
