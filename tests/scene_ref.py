"""numpy restatement of the whole-scene blend (kurosiwo_amd/scene.py, csrc/scene.hip), derived from the formulas and not from that
code: the window grid, the blend weights, the slice-loop blend and the finalisation.  Not a test; shared by tests/test_scene_cpu.py
and tests/test_gpu_scene.py."""
import math

import numpy as np


def axis_origins(L, win, stride):
    """origins of the windows of one axis: stride apart from 0 while a whole window fits, then one more pushed back to end at the
    border; a single origin 0 for an axis shorter than the window"""
    if stride < 1 or stride > win:
        raise ValueError("stride")
    if L < win:
        return [0]
    out, o = [], 0
    while o + win <= L:
        out.append(o)
        o += stride
    if out[-1] + win < L:
        out.append(L - win)
    return out


def window_grid(Hs, Ws, h, w, sy, sx):
    return axis_origins(Hs, h, sy), axis_origins(Ws, w, sx)


def blend_weights(h, w, kind):
    if kind == "uniform":
        return np.full((h, w), 1.0, np.float32)
    assert kind == "hann"
    ay = [0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 0.5) / h) for i in range(h)]
    ax = [0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 0.5) / w) for i in range(w)]
    return np.array([[np.float32(a * b) for b in ax] for a in ay], np.float32)


def blend(logits_by_window, ys, xs, weight, Hs, Ws):
    """logits_by_window [ny * nx, K, h, w] float32, window i = iy * nx + ix at (ys[iy], xs[ix]) -> (acc [K, Hs, Ws], wsum [Hs, Ws]):
    a plain loop over i ascending; numpy rounds the float32 product and the float32 sum separately.  Windows that overhang the scene
    are cropped to it."""
    lg = np.asarray(logits_by_window, np.float32)
    weight = np.asarray(weight, np.float32)
    n, K, h, w = lg.shape
    assert n == len(ys) * len(xs) and weight.shape == (h, w)
    acc = np.zeros((K, Hs, Ws), np.float32)
    wsum = np.zeros((Hs, Ws), np.float32)
    for i in range(n):
        y0, x0 = int(ys[i // len(xs)]), int(xs[i % len(xs)])
        hh, ww = min(h, Hs - y0), min(w, Ws - x0)
        wc = weight[:hh, :ww]
        acc[:, y0:y0 + hh, x0:x0 + ww] += wc * lg[i, :, :hh, :ww]
        wsum[y0:y0 + hh, x0:x0 + ww] += wc
    return acc, wsum


def finalize(acc, wsum, valid=None, invalid_class=3):
    """-> (classes uint8, mean logits float32, softmax float64 of the float32 means): float32 division, first-maximum argmax;
    invalid pixels: invalid_class and NaN scores"""
    assert acc.dtype == np.float32 and wsum.dtype == np.float32
    mean = acc / wsum[None]
    assert mean.dtype == np.float32
    cls = np.argmax(mean, axis=0).astype(np.uint8)                 # numpy: the first maximum
    m64 = mean.astype(np.float64)
    e = np.exp(m64 - m64.max(axis=0, keepdims=True))
    soft = e / e.sum(axis=0, keepdims=True)
    if valid is not None:
        bad = np.asarray(valid) == 0
        cls[bad] = invalid_class
        mean = mean.copy()
        mean[:, bad] = np.nan
        soft[:, bad] = np.nan
    return cls, mean, soft
