"""Augmentation views (the albumentations pipelines of the reference: utilities/augmentations.py get_augmentations for the supervised
Dataset, dataset/Dataset.py:866-870 for SSLDataset) without albumentations or cv2, neither of which is in any image of this project.

A view is drawn on the host and rendered where the tiles are: `Pipeline.sample_params` draws one int32 row {y0, x0, h, w, flip_h,
flip_v} per sample, `apply` renders a raw [B, C, 224, 224] batch with one launch of ksmi_augment_views (csrc/augment.hip: crop ->
INTER_AREA resize -> flips -> noise / dropout, fused with the Dataset's clamp -> nan_to_num -> Normalize), `apply_masks` renders the
label / valid planes with cv2.INTER_NEAREST.  `apply_cpu` / `apply_masks_cpu` restate the same formulas in numpy fp32 for the
per-sample SSLDataset.__getitem__ and for CPU-only users; the formulas themselves are derived in the header of csrc/augment.hip.

Random streams.  The geometric parameters come from a seeded `random.Random`; albumentations draws from Python's global `random`
(and numpy's global state for the noise ops), so no stream of ours can reproduce a reference run sample for sample -- the
distributions are what is kept.  The per-pixel ops (MultNoise, GaussianNoise, Cutout) draw on the device from the counter-based
stream of csrc/common.h keyed by the words {seed, step} of the dropout family."""
import math

import numpy as np

TILE = 224
SITE_AUG = 0x41554700
S_MULT_ON, S_MULT_VAL, S_GAUSS_ON, S_GAUSS_VAR, S_GAUSS_U1, S_GAUSS_U2, S_CUT_ON, S_CUT_POS = range(8)
OP_MULT, OP_GAUSS, OP_CUT = 1, 2, 3
KNOWN = ("RandomResizedCrop", "HorizontalFlip", "VerticalFlip", "GaussianBlur", "ElasticTransform", "Cutout", "GaussianNoise", "MultNoise",
         "ColorJitter")


def sample_resized_crop(rng, H, W, scale, ratio=(3 / 4, 4 / 3)):
    """albumentations 1.3.1 RandomResizedCrop.get_params_dependent_on_targets -> (y0, x0, h, w): ten attempts of
    area = uniform(*scale) * H * W, aspect = exp(uniform(log ratio)), w = round(sqrt(area * aspect)), h = round(sqrt(area / aspect)),
    accepted when 0 < w <= W and 0 < h <= H with the corner uniform over the positions that fit; else the centred crop clamped by
    `ratio`.  (albumentations turns the corner into a fraction and back, h_start = y0 / (H - h + 1e-10), y1 = int((H - h + 1) * h_start);
    that round trip returns y0 for every 0 <= y0 <= H - h.)  `rng` is a seeded random.Random: albumentations uses Python's global
    `random`, so the STREAM of a reference run cannot be matched, only its distribution."""
    area = H * W
    for _ in range(10):
        target = rng.uniform(*scale) * area
        aspect = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
        w = int(round(math.sqrt(target * aspect)))
        h = int(round(math.sqrt(target / aspect)))
        if 0 < w <= W and 0 < h <= H:
            y0 = rng.randint(0, H - h)
            x0 = rng.randint(0, W - w)
            return y0, x0, h, w
    in_ratio = W / H
    if in_ratio < min(ratio):
        w = W
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H
        w = int(round(h * max(ratio)))
    else:
        w, h = W, H
    h, w = max(1, min(h, H)), max(1, min(w, W))
    return (H - h) // 2, (W - w) // 2, h, w


def _threshold(p):
    """round(p * 2^32): a sample gets an op when its 32-bit draw is below it (the complement of conv_plan.drop_threshold's keep test)"""
    return 0 if p <= 0.0 else min(0xFFFFFFFF, int(round(p * 4294967296.0)))


class Pipeline:
    """What build_pipeline read from the json: crop = (p, scale, ratio) or None, flip probabilities, per-pixel ops in json order."""

    def __init__(self, crop=None, hflip=0.0, vflip=0.0, pixel_ops=()):
        self.crop, self.hflip, self.vflip = crop, float(hflip), float(vflip)
        self.pixel_ops = tuple(pixel_ops)                  # (OP_*, p, params...) with p > 0, at most one of each kind
        if len(self.pixel_ops) > 3 or len({o[0] for o in self.pixel_ops}) != len(self.pixel_ops):
            raise ValueError("at most one MultNoise, one GaussianNoise and one Cutout")

    def sample_params(self, rng, n, H=TILE, W=TILE):
        """int32 [n, 6] rows {y0, x0, h, w, flip_h, flip_v}; draws per sample in pipeline order (crop, horizontal, vertical)"""
        out = np.zeros((n, 6), dtype=np.int32)
        for i in range(n):
            box = (0, 0, H, W)
            if self.crop is not None and rng.random() < self.crop[0]:
                box = sample_resized_crop(rng, H, W, self.crop[1], self.crop[2])
            out[i, :4] = box
            out[i, 4] = rng.random() < self.hflip
            out[i, 5] = rng.random() < self.vflip
        return out

    def kernel_args(self):
        """(mult_thr, mult_lo, mult_hi, gauss_thr, var_lo, var_hi, cut_thr, holes, cut_h, cut_w, op_order) of ksmi_augment_views"""
        a = {OP_MULT: (0, 1.0, 1.0), OP_GAUSS: (0, 0.0, 0.0), OP_CUT: (0, 0, 1, 1)}
        order = 0
        for slot, op in enumerate(self.pixel_ops):
            a[op[0]] = (_threshold(op[1]),) + tuple(op[2:])
            order |= op[0] << (2 * slot)
        return a[OP_MULT] + a[OP_GAUSS] + a[OP_CUT] + (order,)


IDENTITY = Pipeline()


def build_pipeline(augmentations):
    """utilities/augmentations.py get_augmentations on the json schema of configs/augmentations/augmentation.json (pass
    configs["augmentations"]): the key order of the json is the op order.  An unknown key raises KeyError; GaussianBlur and
    ElasticTransform with p > 0 raise NotImplementedError by name; ColorJitter is in the json but get_augmentations has no branch
    for it, so it is ignored here as well.  Defaults not in the json are albumentations 1.3.1's: MultiplicativeNoise multiplier
    (0.9, 1.1) (one factor per image), GaussNoise var_limit (10, 50), CoarseDropout 8 holes of 8 x 8 filled with 0."""
    crop, hflip, vflip, ops = None, 0.0, 0.0, []
    for k, v in augmentations.items():
        if k not in KNOWN:
            raise KeyError(k)
        p = float(v.get("p", 0.5))
        if k == "RandomResizedCrop":
            if v["value"] != TILE or v.get("interpolation", 1) != 3:
                raise NotImplementedError("RandomResizedCrop: only 224 x 224 views with interpolation 3 (cv2.INTER_AREA)")
            if ops:
                raise NotImplementedError("RandomResizedCrop behind a noise op (the kernel resizes before it adds noise)")
            crop = (p, tuple(v["scale"]), tuple(v.get("ratio", (3 / 4, 4 / 3))))
        elif k == "HorizontalFlip":
            hflip = p
        elif k == "VerticalFlip":
            vflip = p
        elif k in ("GaussianBlur", "ElasticTransform"):
            if p > 0:
                raise NotImplementedError(f"{k} has no kernel here (p must be 0)")
        elif k == "MultNoise" and p > 0:
            lo, hi = v.get("multiplier", (0.9, 1.1))
            ops.append((OP_MULT, p, float(lo), float(hi)))
        elif k == "GaussianNoise" and p > 0:
            lo, hi = v.get("var_limit", (10.0, 50.0))
            ops.append((OP_GAUSS, p, float(lo), float(hi)))
        elif k == "Cutout" and p > 0:
            ops.append((OP_CUT, p, int(v.get("max_holes", 8)), int(v.get("max_height", 8)), int(v.get("max_width", 8))))
    return Pipeline(crop, hflip, vflip, ops)


def load_pipeline(path):
    """the json file itself (utilities/utilities.py:369-374 merges it into the configs)"""
    from .config import load_json5
    return build_pipeline(load_json5(path)["augmentations"])


# ---- counter-based stream of csrc/common.h, restated (ksmi_mix32 / ksmi_rng_key / ksmi_rng_u32) ------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _mix32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x21F0AAAD)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x735A2D97)) & _M32
    return x ^ (x >> np.uint64(15))


def _draws(seed, step, site, idx):
    key = _mix32(np.uint64(seed & 0xFFFFFFFF) ^ _mix32(np.uint64(step & 0xFFFFFFFF) ^ _mix32((site + 0x9E3779B9) & 0xFFFFFFFF)))
    return _mix32(_mix32(np.asarray(idx, dtype=np.uint64) & _M32) ^ key)


def _u01(r):
    return (r >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


# ---- the view, on the host ------------------------------------------------------------------------------------------------------------
def area_coefficients(n, size=TILE):
    """(source index int64 [size], second tap [size], fp32 weight of the second tap [size]) of the enlarging INTER_AREA resize from
    n to `size` pixels"""
    q = np.arange(size, dtype=np.int64) * n
    s, r = q // size, q % size
    f = np.maximum(0, r + n - size).astype(np.float32) / np.float32(n)
    edge = s >= n - 1
    s = np.where(edge, n - 1, s)
    f = np.where(edge, np.float32(0), f).astype(np.float32)
    return s, np.minimum(s + 1, n - 1), f


def nearest_indices(n, size=TILE):
    return np.minimum(np.arange(size, dtype=np.int64) * n // size, n - 1)


def _prep(x, clamp):
    if clamp is None or clamp < 0:
        return x
    c = np.float32(clamp)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), c, np.minimum(np.maximum(x, np.float32(0)), c)).astype(np.float32)


def _lerp(a, b, f):
    with np.errstate(invalid="ignore"):
        return np.where(f == 0, a, a * (np.float32(1) - f) + b * f).astype(np.float32)


def _rows(params, fallback, n, H, W):
    p = np.asarray(params, dtype=np.int64).reshape(n, 6).copy()
    ident = np.zeros(n, dtype=bool) if fallback is None else (np.asarray(fallback).reshape(n) == 0)
    p[ident] = (0, 0, H, W, 0, 0)
    p[:, 2], p[:, 3] = np.clip(p[:, 2], 1, H), np.clip(p[:, 3], 1, W)
    p[:, 0], p[:, 1] = np.clip(p[:, 0], 0, H - p[:, 2]), np.clip(p[:, 1], 0, W - p[:, 3])
    return p, ident


def apply_cpu(raw, params, mean, std, clamp_input, pipeline=None, fallback=None, rng_words=None):
    """ksmi_augment_views in numpy fp32: raw [B, C, H, W] (array or CPU tensor, NaN no-data included) -> normalised views (same type).
    fallback: None or B counts, 0 = identity for that sample; rng_words = (seed, step) when `pipeline` has per-pixel ops.  The
    geometric part and MultNoise / Cutout give the kernel's bits; GaussianNoise agrees to the rounding of logf / cosf."""
    import torch
    is_t = torch.is_tensor(raw)
    x = raw.numpy() if is_t else np.asarray(raw)
    x = np.ascontiguousarray(x, dtype=np.float32)
    B, C, H, W = x.shape
    p, ident = _rows(params, fallback, B, H, W)
    mean, std = np.asarray(mean, dtype=np.float32).reshape(C, 1, 1), np.asarray(std, dtype=np.float32).reshape(C, 1, 1)
    ops = () if pipeline is None else pipeline.pixel_ops
    if ops and rng_words is None:
        raise ValueError("per-pixel ops need rng_words = (seed, step)")
    out = np.empty_like(x)
    for b in range(B):
        y0, x0, h, w, fh, fv = (int(v) for v in p[b])
        src = _prep(x[b, :, y0:y0 + h, x0:x0 + w], clamp_input)
        sx, sxb, fx = area_coefficients(w, W)
        sy, syb, fy = area_coefficients(h, H)
        t = _lerp(src[:, :, sx], src[:, :, sxb], fx[None, None, :])                   # horizontal pass on every source row
        v = _lerp(t[:, sy, :], t[:, syb, :], fy[None, :, None])
        if fh:
            v = v[:, :, ::-1]
        if fv:
            v = v[:, ::-1, :]
        v = np.ascontiguousarray(v)
        if not ident[b]:
            for op in ops:
                v = _pixel_op(v, op, b, C, rng_words)
        out[b] = (v - mean) / std
    return torch.from_numpy(out) if is_t else out


def _pixel_op(v, op, b, C, words):
    seed, step = words
    kind, thr = op[0], _threshold(op[1])
    C_, H, W = v.shape
    on = {OP_MULT: S_MULT_ON, OP_GAUSS: S_GAUSS_ON, OP_CUT: S_CUT_ON}[kind]
    if not int(_draws(seed, step, SITE_AUG + on, [b])[0]) < thr:
        return v
    if kind == OP_MULT:
        lo, hi = np.float32(op[2]), np.float32(op[3])
        m = np.float32(lo + np.float32(hi - lo) * _u01(_draws(seed, step, SITE_AUG + S_MULT_VAL, [b]))[0])
        return (v * m).astype(np.float32)
    if kind == OP_GAUSS:
        lo, hi = np.float32(op[2]), np.float32(op[3])
        var = np.float32(lo + np.float32(hi - lo) * _u01(_draws(seed, step, SITE_AUG + S_GAUSS_VAR, [b]))[0])
        e = (np.uint64(b) * np.uint64(C) * np.uint64(H * W) + np.arange(C * H * W, dtype=np.uint64)).reshape(C, H, W)
        u1 = ((_draws(seed, step, SITE_AUG + S_GAUSS_U1, e) >> np.uint64(8)).astype(np.float32) + np.float32(1)) * np.float32(1.0 / 16777216.0)
        u2 = _u01(_draws(seed, step, SITE_AUG + S_GAUSS_U2, e))
        z = np.sqrt(np.float32(-2) * np.log(u1)) * np.cos(np.float32(6.28318530717958647692) * u2)
        return (v + np.sqrt(var) * z).astype(np.float32)
    holes, ch, cw = op[2], op[3], op[4]
    v = v.copy()
    r = _draws(seed, step, SITE_AUG + S_CUT_POS, b * 64 + np.arange(2 * holes))
    for k in range(holes):
        hy = int((int(r[2 * k]) * (H - ch + 1)) >> 32)
        hx = int((int(r[2 * k + 1]) * (W - cw + 1)) >> 32)
        v[:, hy:hy + ch, hx:hx + cw] = 0
    return v


def apply_masks_cpu(x, params, fallback=None):
    """ksmi_augment_masks on the host: x [B, H, W] of any dtype -> (views, non-zero count of every view int32 [B])"""
    import torch
    is_t = torch.is_tensor(x)
    a = x.numpy() if is_t else np.asarray(x)
    B, H, W = a.shape
    p, _ = _rows(params, fallback, B, H, W)
    out = np.empty_like(a)
    for b in range(B):
        y0, x0, h, w, fh, fv = (int(v) for v in p[b])
        v = a[b, y0:y0 + h, x0:x0 + w][nearest_indices(h, H)][:, nearest_indices(w, W)]
        if fh:
            v = v[:, ::-1]
        if fv:
            v = v[::-1, :]
        out[b] = v
    count = (out != 0).reshape(B, -1).sum(1).astype(np.int32)
    return (torch.from_numpy(out) if is_t else out), count


# ---- the view, on the device ------------------------------------------------------------------------------------------------------------
def _stream():
    from .runtime import stream_ptr
    return stream_ptr()


def apply(raw, params, mean, std, clamp_input, pipeline=None, fallback=None, rng_state=None, out=None):
    """ksmi_augment_views: raw [B, C, 224, 224] fp32 CUDA tensor, params int32 [B, 6] on the same device (mean / std: device fp32
    tensors or sequences), fallback: None or the int32 [B] counts apply_masks wrote, rng_state: int32 [2] device words {seed, step}
    when `pipeline` has per-pixel ops.  Runs on the current stream; nothing is synchronised."""
    import torch
    from . import _lib
    from .runtime import require_gpu
    require_gpu(raw)
    if raw.dtype != torch.float32 or not raw.is_contiguous() or raw.dim() != 4:
        raise ValueError("apply: contiguous fp32 [B, C, H, W]")
    B, C, H, W = raw.shape
    if params.dtype != torch.int32 or params.numel() != B * 6 or not params.is_contiguous() or params.device != raw.device:
        raise ValueError("apply: params is a contiguous int32 [B, 6] tensor on the device of the tiles")
    if fallback is not None and (fallback.dtype != torch.int32 or fallback.numel() != B or fallback.device != raw.device):
        raise ValueError("apply: fallback is an int32 [B] device tensor")
    m = mean if torch.is_tensor(mean) else torch.as_tensor(mean, dtype=torch.float32, device=raw.device)
    s = std if torch.is_tensor(std) else torch.as_tensor(std, dtype=torch.float32, device=raw.device)
    if m.numel() != C or s.numel() != C:
        raise ValueError("apply: one mean / std per channel")
    args = (pipeline or IDENTITY).kernel_args()
    if args[-1] and (rng_state is None or rng_state.dtype != torch.int32 or rng_state.numel() != 2 or rng_state.device != raw.device):
        raise ValueError("apply: rng_state int32[2] device tensor {seed, step} (the pipeline has per-pixel ops)")
    out = torch.empty_like(raw) if out is None else out
    _lib.check(_lib.load().ksmi_augment_views(raw.data_ptr(), params.data_ptr(), None if fallback is None else fallback.data_ptr(), m.data_ptr(),
                                              s.data_ptr(), out.data_ptr(), B, C, H, W, float(-1.0 if clamp_input is None else clamp_input), *args,
                                              None if rng_state is None else rng_state.data_ptr(), _stream()), "augment_views")
    return out


def apply_masks(x, params, fallback=None, count=False, write=True):
    """ksmi_augment_masks: x [B, 224, 224] uint8 / fp32 / int32 / int64 CUDA tensor -> (views or None, counts int32 [B] or None)"""
    import torch
    from . import _lib
    from .runtime import require_gpu
    require_gpu(x)
    if x.dim() != 3 or not x.is_contiguous() or x.element_size() not in (1, 4, 8):
        raise ValueError("apply_masks: contiguous [B, H, W] of 1-, 4- or 8-byte elements")
    B, H, W = x.shape
    if params.dtype != torch.int32 or params.numel() != B * 6 or not params.is_contiguous() or params.device != x.device:
        raise ValueError("apply_masks: params is a contiguous int32 [B, 6] tensor on the device of the masks")
    y = torch.empty_like(x) if write else None
    cnt = torch.empty(B, dtype=torch.int32, device=x.device) if count else None
    _lib.check(_lib.load().ksmi_augment_masks(x.data_ptr(), None if y is None else y.data_ptr(), params.data_ptr(),
                                              None if fallback is None else fallback.data_ptr(), None if cnt is None else cnt.data_ptr(), B, H, W,
                                              x.element_size(), _stream()), "augment_masks")
    return y, cnt
