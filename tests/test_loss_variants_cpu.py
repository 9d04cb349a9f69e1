"""CPU: the dice / iou (Lovasz-softmax) / focal branches of create_loss (kurosiwo_amd/loss.py; reference utilities/utilities.py:323-341):
module selection, refusal of the options the HIP kernels do not cover, the loud failure on a CPU tensor, and the float64 formula oracle
(tests/loss_variants_ref.py) against hand-worked 1 x 3 x 2 x 2 cases."""
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_variants_ref as LV  # noqa: E402

from kurosiwo_amd import _lib  # noqa: E402
from kurosiwo_amd import loss as L  # noqa: E402

CLASS_WEIGHTS = [0.3715753140309927, 14.009780283125977, 8.20405370357821]


def _cfg(lf):
    return {"loss_function": lf, "class_weights": CLASS_WEIGHTS, "device": "cpu"}


@pytest.mark.parametrize("mode", ["train", "val"])
def test_create_loss_builds_the_new_branches(mode):
    d = L.create_loss(_cfg("dice"), mode)
    assert isinstance(d, L.DiceLoss) and d.ignore_index == 3 and d.kind == _lib.LOSS_DICE
    i = L.create_loss(_cfg("iou"), mode)
    assert isinstance(i, L.LovaszLoss) and i.ignore_index == 3 and i.kind == _lib.LOSS_LOVASZ
    f = L.create_loss(_cfg("focal"), mode)
    assert isinstance(f, L.FocalLoss) and f.ignore_index == 3 and f.kind == _lib.LOSS_FOCAL and f.gamma == 2.0
    # focal carries the class weights in BOTH modes (utilities.py:327-341), unlike cross_entropy's val criterion
    assert torch.allclose(f.weight, torch.tensor(CLASS_WEIGHTS, dtype=torch.float32))
    with pytest.raises(NotImplementedError):
        L.create_loss(_cfg("no-such-loss"), mode)


def test_unsupported_options_raise():
    for mk in (lambda: L.DiceLoss(mode="binary"), lambda: L.DiceLoss(mode="multilabel"), lambda: L.DiceLoss(smooth=1.0),
               lambda: L.DiceLoss(log_loss=True), lambda: L.DiceLoss(classes=[0, 1]),
               lambda: L.LovaszLoss(per_image=True), lambda: L.LovaszLoss(mode="binary"), lambda: L.LovaszLoss(mode="multilabel"),
               lambda: L.FocalLoss(reduction="sum"), lambda: L.FocalLoss(reduction="none"), lambda: L.FocalLoss(gamma=0.5),
               lambda: L.FocalLoss(gamma=-1.0), lambda: L.FocalLoss(alpha=[1.0, 1.0])):
        with pytest.raises(_lib.KsmiError):
            mk()
    L.FocalLoss(gamma=0.0)            # gamma = 0 and gamma >= 1 are accepted
    L.FocalLoss(gamma=1.0)


def test_cpu_tensor_fails_loudly():
    x = torch.zeros(1, 3, 4, 4)
    t = torch.zeros(1, 4, 4, dtype=torch.int64)
    for crit in (L.DiceLoss(ignore_index=3), L.LovaszLoss(ignore_index=3), L.FocalLoss(alpha=CLASS_WEIGHTS, ignore_index=3)):
        with pytest.raises(_lib.KsmiError):
            crit(x, t)


def test_library_exports_the_loss_family():
    lib = _lib.load()
    assert lib.ksmi_seg_loss_workspace(_lib.LOSS_DICE, 2, 16) > 0 and lib.ksmi_seg_loss_workspace(_lib.LOSS_FOCAL, 2, 16) > 0
    # Lovasz: keys and payloads, double-buffered, for 3 classes -- O(B HW)
    assert lib.ksmi_seg_loss_workspace(_lib.LOSS_LOVASZ, 32, 224 * 224) >= 4 * 3 * 32 * 224 * 224 * 4
    assert lib.ksmi_seg_loss_workspace(0, 2, 16) == 0 and lib.ksmi_seg_loss_workspace(_lib.LOSS_DICE, 0, 16) == 0
    assert lib.ksmi_seg_loss_forward(7, None, None, None, 0.0, None, None, 1, 1, 3, None) != 0
    assert lib.ksmi_seg_loss_forward(_lib.LOSS_DICE, None, None, None, 0.0, None, None, 1, 1, 3, None) != 0
    assert lib.ksmi_seg_loss_backward(_lib.LOSS_FOCAL, None, None, None, 2.0, None, None, None, 1, 1, 3, None) != 0


# ------------------------------------------------------------------ the oracle against hand-worked cases
def _logp(rows):
    """1 x 3 x 2 x 2 log-probabilities (softmax gives the rows back) from 4 per-pixel probability triples in (h, w) order"""
    p = torch.tensor(rows, dtype=torch.float64)                  # [4, 3]
    return p.log().t().reshape(1, 3, 2, 2)


def test_oracle_dice_hand_worked():
    x = torch.zeros(1, 3, 2, 2, dtype=torch.float64)            # p = 1/3 everywhere
    # one pixel per class, one ignored: I = 1/3, D = 1 + 1, score 1/3 per class
    assert LV.dice_loss(x, torch.tensor([[[0, 1], [2, 3]]])).item() == pytest.approx(2.0 / 3.0, abs=1e-12)
    # class 2 absent (contributes 0 but counts in the mean of 3): c0: I = 2/3, D = 3 -> 5/9; c1: I = 1/3, D = 2 -> 2/3
    lbl = torch.tensor([[[0, 0], [1, 3]]])
    assert LV.dice_loss(x, lbl).item() == pytest.approx((5.0 / 9.0 + 2.0 / 3.0) / 3.0, abs=1e-12)
    loss, g = LV.loss_and_grad("dice", x, lbl)
    assert g[0, :, 1, 1].abs().max() == 0.0                     # the ignored pixel
    # every pixel ignored: every class absent -> 0, zero gradient
    loss, g = LV.loss_and_grad("dice", x, torch.full((1, 2, 2), 3))
    assert loss == 0.0 and g.abs().max() == 0.0


ROWS = [(0.5, 0.25, 0.25), (0.25, 0.5, 0.25), (0.25, 0.5, 0.25), (0.5, 0.25, 0.25)]


def test_oracle_lovasz_hand_worked():
    x = _logp(ROWS)
    lbl = torch.tensor([[[0, 0], [1, 2]]])
    # class 0: e = (.5, .75, .25, .5), fg = (1, 1, 0, 0) -> sorted fg (1, 1, 0, 0), g = (.5, .5, 0, 0): .75 * .5 + .5 * .5 = .625
    # class 1: e = (.25, .5, .5, .25), fg = (0, 0, 1, 0) -> the tie (.5, .5) keeps pixel 1 (bg) before pixel 2 (fg): g = (.5, .5, 0, 0): .5
    # class 2: e = (.25, .25, .25, .75), fg = (0, 0, 0, 1) -> g = (1, 0, 0, 0): .75
    assert LV._lovasz_grad(torch.tensor([1.0, 1.0, 0.0, 0.0], dtype=torch.float64)).tolist() == [0.5, 0.5, 0.0, 0.0]
    assert LV.lovasz_loss(x, lbl).item() == pytest.approx((0.625 + 0.5 + 0.75) / 3.0, abs=1e-12)
    # the tie rule shows in the gradient with respect to p_1: pixel 1 (bg, rank 0) gets +.5/3, pixel 2 (fg, rank 1) -.5/3
    # (an order that put pixel 2 first would give pixel 1 nothing and pixel 2 -1/3, with the same loss)
    p = torch.tensor(ROWS, dtype=torch.float64, requires_grad=True)
    LV.lovasz_softmax_flat(p, lbl.view(-1)).backward()
    assert p.grad[:, 1].tolist() == pytest.approx([0.0, 0.5 / 3.0, -0.5 / 3.0, 0.0], abs=1e-12)
    # a class absent from the valid pixels is skipped: classes 0 and 1 only
    lbl2 = torch.tensor([[[0, 0], [1, 3]]])
    v = LV.lovasz_loss(x, lbl2).item()
    # class 0 over pixels 0..2: e = (.5, .75, .25), fg (1, 1, 0) -> .75 * .5 + .5 * .5 = .625; class 1: e = (.25, .5, .5), fg (0, 0, 1),
    # sorted (pixel 1 bg, pixel 2 fg, pixel 0 bg): gts 1, J = (.5, 1, 1) -> g = (.5, .5, 0): .5
    assert v == pytest.approx((0.625 + 0.5) / 2.0, abs=1e-12)
    loss, g = LV.loss_and_grad("iou", x, torch.full((1, 2, 2), 3))
    assert loss == 0.0 and g.abs().max() == 0.0


def test_oracle_focal_hand_worked():
    x = _logp(ROWS)
    lbl = torch.tensor([[[0, 0], [1, 3]]])
    a0, a1 = CLASS_WEIGHTS[0], CLASS_WEIGHTS[1]
    # pt = .5 (alpha0), .25 (alpha0), .5 (alpha1); pixel 3 ignored; the mean runs over the 3 valid pixels
    ref = (a0 * 0.25 * math.log(2) + a0 * 0.5625 * math.log(4) + a1 * 0.25 * math.log(2)) / 3.0
    assert LV.focal_loss(x, lbl, CLASS_WEIGHTS, 2.0).item() == pytest.approx(ref, rel=1e-12)
    # gamma = 0: the weighted NLL SUM over the valid count (not over the sum of alpha, unlike weighted CE)
    g0 = LV.focal_loss(x, lbl, CLASS_WEIGHTS, 0.0).item()
    assert g0 == pytest.approx((a0 * math.log(2) + a0 * math.log(4) + a1 * math.log(2)) / 3.0, rel=1e-12)
    xs = x.permute(0, 2, 3, 1).reshape(-1, 3)[:3]
    nll = F.nll_loss(F.log_softmax(xs, -1), lbl.view(-1)[:3], weight=torch.tensor(CLASS_WEIGHTS, dtype=torch.float64), reduction="sum")
    assert g0 == pytest.approx(float(nll) / 3.0, rel=1e-12)
    loss, g = LV.loss_and_grad("focal", x, torch.full((1, 2, 2), 3), alpha=CLASS_WEIGHTS)
    assert loss == 0.0 and g.abs().max() == 0.0
    loss, g = LV.loss_and_grad("focal", x, lbl, alpha=CLASS_WEIGHTS)
    assert g[0, :, 1, 1].abs().max() == 0.0


def test_near_tie_mask_marks_mixed_runs_only():
    x = _logp(ROWS)
    m = LV.lovasz_near_tie_mask(x, torch.tensor([[[0, 0], [1, 2]]]))
    # class 1 ties pixel 1 (bg) with pixel 2 (fg); class 2's tie (pixels 0, 1, 2) is all background; class 0's (.5, .5) is fg + bg
    assert m.view(-1).tolist() == [True, True, True, True]
    # every pixel of class 1: each class's ties join pixels of one kind (all background for 0 and 2, all foreground for 1)
    m = LV.lovasz_near_tie_mask(x, torch.tensor([[[1, 1], [1, 1]]]))
    assert m.view(-1).tolist() == [False, False, False, False]
