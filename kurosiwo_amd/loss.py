"""Loss surface of the reference on the fused HIP kernel (rows L1/L2).

  create_loss(configs, mode)      <- /root/reference/utilities/utilities.py:307-347
  BCEandDiceLoss(weights, ignore_index, use_softmax)
                                  <- /root/reference/utilities/bce_and_dice.py:7-24
                                     (+ utilities/dice.py:93-137)
  CrossEntropyLoss(weight, ignore_index)  == nn.CrossEntropyLoss as used by create_loss
  DiceLoss(mode, ignore_index)            == smp.losses.DiceLoss (multiclass, smooth 0, eps 1e-7)
  LovaszLoss(mode, per_image, ignore_index) == smp.losses.LovaszLoss (multiclass, per_image=False)
  FocalLoss(alpha, gamma, reduction, ignore_index) == adeelh/pytorch-multi-class-focal-loss FocalLoss (reduction="mean")
                                          (the last three: csrc/loss.hip, ksmi_seg_loss_*; formulas in include/ksmi.h)

callable(preds fp32 [B,3,H,W], lbl int64 [B,H,W]) -> 0-dim tensor with autograd.
Dice and Lovasz reduce over the whole batch this callable sees: under data parallelism each rank computes them over its own shard.
"""
import torch
import torch.nn as nn

from . import _lib
from .runtime import require_gpu, stream_ptr


class _CEDiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, cw, with_dice, ignore_index):
        lib = _lib.load()
        B, Cc, H, W = logits.shape
        out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
        ws = torch.empty(lib.ksmi_loss_workspace(B, H * W), dtype=torch.uint8, device=logits.device)
        _lib.check(lib.ksmi_ce_dice_forward(logits.data_ptr(), labels.data_ptr(), cw.data_ptr(), int(with_dice),
                                            out3.data_ptr(), ws.data_ptr(), B, H * W, ignore_index, stream_ptr()), "ce_dice_forward")
        ctx.save_for_backward(logits, labels, cw, ws)
        ctx.with_dice, ctx.ignore_index = with_dice, ignore_index
        ctx.parts = out3
        return out3[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels, cw, ws = ctx.saved_tensors
        lib = _lib.load()
        B, Cc, H, W = logits.shape
        dl = torch.empty_like(logits)
        gs = grad_out.contiguous().float()
        _lib.check(lib.ksmi_ce_dice_backward(logits.data_ptr(), labels.data_ptr(), cw.data_ptr(), int(ctx.with_dice),
                                             ws.data_ptr(), gs.data_ptr(), dl.data_ptr(), B, H * W, ctx.ignore_index,
                                             stream_ptr()), "ce_dice_backward")
        return dl, None, None, None, None


def _check_inputs(preds, lbl):
    if preds.dim() != 4 or preds.shape[1] != 3:
        raise ValueError(f"Invalid input shape, we expect Bx3xHxW. Got: {tuple(preds.shape)}")
    if preds.shape[-2:] != lbl.shape[-2:]:
        raise ValueError(f"input and target shapes must be the same. Got: {tuple(preds.shape)} {tuple(lbl.shape)}")
    if lbl.dtype != torch.int64:
        raise ValueError(f"labels must be torch.int64. Got: {lbl.dtype}")


class _HipLoss(nn.Module):
    def __init__(self, weights, ignore_index, with_dice):
        super().__init__()
        w = torch.as_tensor(weights if weights is not None else [1.0, 1.0, 1.0], dtype=torch.float32)
        if w.numel() != 3:
            raise _lib.KsmiError("the HIP loss supports num_classes == 3 (reference configs/config.json:13)")
        self.register_buffer("weight", w)
        self.ignore_index = -100 if ignore_index is None else int(ignore_index)
        self.with_dice = with_dice
        self.last_parts = None

    def forward(self, preds, lbl):
        require_gpu(preds)
        _check_inputs(preds, lbl)
        if self.weight.device != preds.device:
            self.weight = self.weight.to(preds.device)
        return _CEDiceFn.apply(preds.contiguous().float(), lbl.contiguous(), self.weight, self.with_dice, self.ignore_index)


class BCEandDiceLoss(_HipLoss):
    """softmax-CE (weighted, ignore_index) + softmax-Dice; `use_softmax` must be True as in create_loss."""

    def __init__(self, weights=None, ignore_index=None, use_softmax=False):
        if not use_softmax:
            raise _lib.KsmiError("BCEandDiceLoss(HIP): only use_softmax=True (the reference's create_loss setting) is implemented")
        super().__init__(weights, ignore_index, True)


class CrossEntropyLoss(_HipLoss):
    def __init__(self, weight=None, ignore_index=-100):
        super().__init__(weight, ignore_index, False)


class _SegLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, cw, kind, gamma, ignore_index):
        lib = _lib.load()
        B, Cc, H, W = logits.shape
        out3 = torch.empty(3, dtype=torch.float32, device=logits.device)
        ws = torch.empty(lib.ksmi_seg_loss_workspace(kind, B, H * W), dtype=torch.uint8, device=logits.device)
        _lib.check(lib.ksmi_seg_loss_forward(kind, logits.data_ptr(), labels.data_ptr(), cw.data_ptr(), gamma, out3.data_ptr(),
                                             ws.data_ptr(), B, H * W, ignore_index, stream_ptr()), "seg_loss_forward")
        ctx.save_for_backward(logits, labels, cw, ws)
        ctx.kind, ctx.gamma, ctx.ignore_index = kind, gamma, ignore_index
        return out3[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        logits, labels, cw, ws = ctx.saved_tensors
        lib = _lib.load()
        B, Cc, H, W = logits.shape
        dl = torch.empty_like(logits)
        gs = grad_out.contiguous().float()
        _lib.check(lib.ksmi_seg_loss_backward(ctx.kind, logits.data_ptr(), labels.data_ptr(), cw.data_ptr(), ctx.gamma, ws.data_ptr(),
                                              gs.data_ptr(), dl.data_ptr(), B, H * W, ctx.ignore_index, stream_ptr()), "seg_loss_backward")
        return dl, None, None, None, None, None


def _multiclass_only(name, mode):
    if mode != "multiclass":
        raise _lib.KsmiError(f"{name}(HIP): only mode='multiclass' (the reference's create_loss setting) is implemented, got {mode!r}")


class _SegLoss(_HipLoss):
    """the losses of csrc/loss.hip: same input contract as _HipLoss, one ksmi_seg_loss_* kind"""

    def __init__(self, kind, weights=None, ignore_index=None, gamma=0.0):
        super().__init__(weights, ignore_index, False)
        self.kind, self.gamma = kind, float(gamma)

    def forward(self, preds, lbl):
        require_gpu(preds)
        _check_inputs(preds, lbl)
        if self.weight.device != preds.device:
            self.weight = self.weight.to(preds.device)
        return _SegLossFn.apply(preds.contiguous().float(), lbl.contiguous(), self.weight, self.kind, self.gamma, self.ignore_index)


class DiceLoss(_SegLoss):
    """smp.losses.DiceLoss(mode="multiclass", ignore_index): softmax Dice with the sums over the whole batch, absent classes masked
    (they count in the mean over the 3 classes).  Only the defaults smp's create_loss branch uses are implemented."""

    def __init__(self, mode="multiclass", classes=None, log_loss=False, from_logits=True, smooth=0.0, ignore_index=None, eps=1e-7):
        _multiclass_only("DiceLoss", mode)
        if classes is not None or log_loss or not from_logits or smooth != 0.0 or eps != 1e-7:
            raise _lib.KsmiError("DiceLoss(HIP): classes=None, log_loss=False, from_logits=True, smooth=0, eps=1e-7 only")
        super().__init__(_lib.LOSS_DICE, None, ignore_index)


class LovaszLoss(_SegLoss):
    """smp.losses.LovaszLoss(mode="multiclass", per_image=False, ignore_index): Lovasz-softmax over the flattened batch, mean over the
    present classes.  Ties of the error sort keep the flattened (b, h, w) order (a stable sort)."""

    def __init__(self, mode="multiclass", per_image=False, ignore_index=None, from_logits=True):
        _multiclass_only("LovaszLoss", mode)
        if per_image:
            raise _lib.KsmiError("LovaszLoss(HIP): per_image=True is not implemented (create_loss uses per_image=False)")
        if not from_logits:
            raise _lib.KsmiError("LovaszLoss(HIP): from_logits=True only")
        super().__init__(_lib.LOSS_LOVASZ, None, ignore_index)


class FocalLoss(_SegLoss):
    """adeelh FocalLoss(alpha, gamma, reduction="mean", ignore_index): sum alpha[y] (1 - pt)^gamma (-log pt) over the valid pixels,
    divided by their count (not by the sum of alpha); 0 when no pixel is valid."""

    def __init__(self, alpha=None, gamma=2.0, reduction="mean", ignore_index=-100):
        if reduction != "mean":
            raise _lib.KsmiError(f"FocalLoss(HIP): reduction='mean' only (create_loss's setting), got {reduction!r}")
        gamma = float(gamma)
        if not (gamma == 0.0 or gamma >= 1.0):
            raise _lib.KsmiError(f"FocalLoss(HIP): gamma must be 0 or >= 1 (the gradient of (1 - pt)^gamma is infinite at pt = 1 "
                                 f"for 0 < gamma < 1), got {gamma}")
        super().__init__(_lib.LOSS_FOCAL, alpha, ignore_index, gamma)


def create_loss(configs, mode="val"):
    lf = configs["loss_function"]
    cw = configs.get("class_weights", [1.0, 1.0, 1.0])
    dev = configs.get("device", "cuda")
    if lf == "cross_entropy":
        if mode == "train":
            print("Creating cross entropy loss with class weights")
            print(torch.tensor(cw))
            return CrossEntropyLoss(weight=cw, ignore_index=3).to(dev)
        return CrossEntropyLoss(ignore_index=3).to(dev)
    if lf == "iou":
        return LovaszLoss(mode="multiclass", ignore_index=3).to(dev)
    if lf == "dice":
        return DiceLoss(mode="multiclass", ignore_index=3).to(dev)
    if lf == "focal":
        return FocalLoss(alpha=cw, gamma=2, ignore_index=3, reduction="mean").to(dev)
    if lf == "ce+dice":
        return BCEandDiceLoss(weights=cw, ignore_index=3, use_softmax=True).to(dev)
    raise NotImplementedError(f"loss_function={lf!r}: the reference's create_loss knows cross_entropy, iou, dice, focal and ce+dice")
