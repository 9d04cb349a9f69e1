"""numpy restatement of the test-time views of the whole-scene blend (kurosiwo_amd/scene.py: VIEW_SETS, predict_scene(tta=...);
csrc/scene.hip), written from the definition and not from that code.  A view code v in 0 .. 7: bit 2 transposes the tile (first),
bit 1 then flips y, bit 0 then flips x; the inverse undoes the flips, then the transpose.  Not a test; shared by
tests/test_scene_tta_cpu.py and tests/test_gpu_scene_tta.py."""
import numpy as np

VIEW_SETS = {"hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def view(t, v):
    """view v of every [h, w] tile of t [..., h, w]"""
    assert 0 <= v <= 7
    u = t.swapaxes(-1, -2) if v & 4 else t
    if v & 2:
        u = u[..., ::-1, :]
    if v & 1:
        u = u[..., ::-1]
    return np.ascontiguousarray(u)


def unview(u, v):
    """the tile whose view v is u"""
    assert 0 <= v <= 7
    t = u
    if v & 1:
        t = t[..., ::-1]
    if v & 2:
        t = t[..., ::-1, :]
    if v & 4:
        t = t.swapaxes(-1, -2)
    return np.ascontiguousarray(t)


def blend_views(logits_by_view, ys, xs, weight, Hs, Ws):
    """logits_by_view [V, ny * nx, K, h, w] float32 in window orientation -> (acc [K, Hs, Ws], wsum [Hs, Ws]): the slice loop of
    scene_ref.blend over the windows i ascending with, inside it, the views v ascending; every view adds weight * logits to acc and
    weight to wsum, the float32 product and the float32 sum rounded separately"""
    lg = np.asarray(logits_by_view, np.float32)
    weight = np.asarray(weight, np.float32)
    V, n, K, h, w = lg.shape
    assert n == len(ys) * len(xs) and weight.shape == (h, w)
    acc = np.zeros((K, Hs, Ws), np.float32)
    wsum = np.zeros((Hs, Ws), np.float32)
    for i in range(n):
        y0, x0 = int(ys[i // len(xs)]), int(xs[i % len(xs)])
        hh, ww = min(h, Hs - y0), min(w, Ws - x0)
        wc = weight[:hh, :ww]
        for v in range(V):
            acc[:, y0:y0 + hh, x0:x0 + ww] += wc * lg[v, i, :, :hh, :ww]
            wsum[y0:y0 + hh, x0:x0 + ww] += wc
    return acc, wsum
