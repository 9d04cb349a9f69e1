"""Float64 formula oracle of the dice / Lovasz-softmax / focal losses (kurosiwo_amd.loss DiceLoss, LovaszLoss, FocalLoss).

A helper module of the loss tests, not a test file.  The reference builds these losses from segmentation-models-pytorch 0.3.2
(DiceLoss, LovaszLoss) and from the torch.hub repo adeelh/pytorch-multi-class-focal-loss (FocalLoss); neither is installed here, so
the oracle is FORMULA-PINNED: it restates their published code paths (include/ksmi.h states the contract) in float64, and the
gradients come from autograd.  The one deliberate difference from smp: the Lovasz error sort is stable (ties keep the flattened
(b, h, w) order), the tie rule of the HIP kernel; smp's unstable torch.sort gives the same loss value, but not the same gradient.
"""
import torch
import torch.nn.functional as F

IGNORE_INDEX = 3


# ---- smp DiceLoss(mode="multiclass", ignore_index, smooth=0, eps=1e-7, log_loss=False, from_logits=True) ----
def dice_loss(logits, labels, ignore_index=IGNORE_INDEX, smooth=0.0, eps=1e-7):
    y_pred = logits.double().log_softmax(dim=1).exp()
    bs, num_classes = y_pred.shape[:2]
    dims = (0, 2)
    y_true = labels.view(bs, -1)
    y_pred = y_pred.view(bs, num_classes, -1)
    mask = y_true != ignore_index
    y_pred = y_pred * mask.unsqueeze(1)
    y_true = F.one_hot((y_true * mask).to(torch.long), num_classes)
    y_true = y_true.permute(0, 2, 1) * mask.unsqueeze(1)
    y_true = y_true.type_as(y_pred)
    intersection = torch.sum(y_pred * y_true, dim=dims)
    cardinality = torch.sum(y_pred + y_true, dim=dims)
    scores = (2.0 * intersection + smooth) / (cardinality + smooth).clamp_min(eps)
    loss = 1.0 - scores
    loss = loss * (y_true.sum(dims) > 0).to(loss.dtype)
    return loss.mean()


# ---- smp LovaszLoss(mode="multiclass", per_image=False, ignore_index) ----
def _lovasz_grad(gt_sorted):
    p = len(gt_sorted)
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1.0 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if p > 1:
        jaccard[1:p] = jaccard[1:p] - jaccard[0:-1]
    return jaccard


def _flatten_probas(probas, labels, ignore=None):
    B, C, H, W = probas.shape
    probas = probas.permute(0, 2, 3, 1).contiguous().view(-1, C)     # (b, h, w) order
    labels = labels.view(-1)
    if ignore is None:
        return probas, labels
    valid = labels != ignore
    return probas[valid], labels[valid]


def _mean(values, empty=0.0):
    values = list(values)
    if not values:
        return empty
    acc = values[0]
    for v in values[1:]:
        acc = acc + v
    return acc / len(values)


def lovasz_softmax_flat(probas, labels):
    """probas [P, C] float64 (valid pixels only), labels [P]: mean over the present classes of <sorted errors, Lovasz gradient>"""
    if probas.numel() == 0:
        return probas.sum() * 0.0
    losses = []
    for c in range(probas.size(1)):
        fg = (labels == c).to(probas.dtype)
        if fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, dim=0, descending=True, stable=True)
        losses.append(torch.dot(errors_sorted, _lovasz_grad(fg[perm])))
    return _mean(losses, empty=probas.sum() * 0.0)


def lovasz_loss(logits, labels, ignore_index=IGNORE_INDEX):
    probas = logits.double().softmax(dim=1)
    return lovasz_softmax_flat(*_flatten_probas(probas, labels, ignore_index))


# ---- adeelh FocalLoss(alpha, gamma, reduction="mean", ignore_index) ----
def focal_loss(logits, labels, alpha=(1.0, 1.0, 1.0), gamma=2.0, ignore_index=IGNORE_INDEX):
    x = logits.double()
    c = x.shape[1]
    x = x.permute(0, *range(2, x.ndim), 1).reshape(-1, c)
    y = labels.reshape(-1)
    unignored = y != ignore_index
    y = y[unignored]
    if len(y) == 0:
        return logits.double().sum() * 0.0
    x = x[unignored]
    log_p = F.log_softmax(x, dim=-1)
    ce = F.nll_loss(log_p, y, weight=torch.as_tensor(alpha, dtype=torch.float64), reduction="none")
    log_pt = log_p[torch.arange(len(x)), y]
    pt = log_pt.exp()
    return ((1.0 - pt) ** gamma * ce).mean()


LOSSES = {"dice": dice_loss, "iou": lovasz_loss, "focal": focal_loss}


def loss_and_grad(name, logits, labels, **kw):
    """float64 loss value and d loss / d logits (autograd) of one of LOSSES"""
    x = logits.detach().double().cpu().requires_grad_(True)
    loss = LOSSES[name](x, labels.cpu(), **kw)
    (g,) = torch.autograd.grad(loss, x, allow_unused=True)
    return float(loss.detach()), (torch.zeros_like(x) if g is None else g)


def lovasz_near_tie_mask(logits, labels, ignore_index=IGNORE_INDEX, rtol=4e-7):
    """bool [B,H,W]: pixels whose Lovasz gradient an fp32 evaluation may legitimately order differently from this float64 oracle --
    members of a run of consecutive sorted errors (per class) that holds both foreground and background pixels, where neighbours join
    a run when their errors differ by less than rtol x the larger of their class probabilities (an fp32 softmax value carries a few
    ulps of rounding, and e = |fg - p| inherits it).  Swapping a foreground and a background neighbour moves both gradients by
    O(1 / union); swaps among pixels of one kind move nothing."""
    B, C, H, W = logits.shape
    probas = logits.double().softmax(dim=1).permute(0, 2, 3, 1).reshape(-1, C)
    lab = labels.reshape(-1)
    valid = lab != ignore_index
    idx = torch.nonzero(valid).flatten()
    mask = torch.zeros(lab.numel(), dtype=torch.bool)
    for c in range(C):
        fg = (lab[idx] == c).double()
        pc = probas[idx, c]
        e = (fg - pc).abs()
        es, perm = torch.sort(e, descending=True, stable=True)
        fgs, ps = fg[perm], pc[perm]
        if es.numel() < 2:
            continue
        close = (es[:-1] - es[1:]).abs() < rtol * torch.maximum(ps[:-1], ps[1:])
        run = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum((~close).long(), 0)])    # run id per sorted position
        nruns = int(run[-1]) + 1
        nfg = torch.zeros(nruns, dtype=torch.float64).index_add_(0, run, fgs)
        nall = torch.zeros(nruns, dtype=torch.float64).index_add_(0, run, torch.ones_like(fgs))
        mixed = (nfg > 0) & (nfg < nall)
        mask[idx[perm[mixed[run]]]] = True
    return mask.view(B, H, W)
