"""Whole-scene inference, host half (kurosiwo_amd/scene.py): the window grid, the blend weights and the numpy restatement of the blend
(tests/scene_ref.py) that the GPU tests hold the kernels to; the library exports and binds the four ksmi_scene_* entry points and
their argument checks launch nothing.  No GPU."""
import numpy as np
import pytest

import scene_ref

AXES = [(8, 8, 8), (5, 8, 4), (19, 8, 5), (16, 8, 8), (17, 8, 8), (224, 224, 112), (500, 224, 112)]


@pytest.mark.parametrize("axis", AXES, ids=lambda a: "-".join(map(str, a)))
def test_window_grid_covers_the_scene(axis):
    from kurosiwo_amd.scene import window_grid
    L, win, stride = axis
    other = (11, 4, 3)                                              # the two axes are independent: pair each case with a fixed one
    for (Hs, h, sy), (Ws, w, sx) in ((axis, other), (other, axis)):
        ys, xs = window_grid(Hs, Ws, h, w, sy, sx)
        assert ys.dtype == np.int32 and xs.dtype == np.int32
        rys, rxs = scene_ref.window_grid(Hs, Ws, h, w, sy, sx)
        assert ys.tolist() == rys and xs.tolist() == rxs
    o = window_grid(L, 11, win, 4, stride, 3)[0].tolist()
    covered = np.zeros(L, bool)
    for a in o:
        assert a >= 0
        covered[a:a + win] = True
    assert covered.all()                                            # every pixel is covered
    assert o == sorted(set(o))                                      # sorted and unique
    if L >= win:
        assert all(a + win <= L for a in o)                         # inside the scene
        assert o[-1] + win == L                                     # the last window is flush with the border
        assert all(b - a <= stride for a, b in zip(o, o[1:]))
    else:
        assert o == [0]
    for bad in (0, win + 1):
        with pytest.raises(ValueError):
            window_grid(L, 11, win, 4, bad, 3)
        with pytest.raises(ValueError):
            window_grid(11, L, 4, win, 3, bad)


def test_window_grid_known_cases():
    from kurosiwo_amd.scene import window_grid
    assert window_grid(19, 17, 8, 8, 5, 8)[0].tolist() == [0, 5, 10, 11] and window_grid(19, 17, 8, 8, 5, 8)[1].tolist() == [0, 8, 9]
    assert window_grid(500, 224, 224, 224, 112, 112)[0].tolist() == [0, 112, 224, 276]
    assert window_grid(500, 224, 224, 224, 112, 112)[1].tolist() == [0]


def test_blend_weights():
    from kurosiwo_amd.scene import blend_weights
    for h, w in ((8, 8), (5, 11), (224, 224), (1, 3)):
        u = blend_weights(h, w, "uniform")
        assert u.dtype == np.float32 and u.shape == (h, w) and (u.view(np.uint32) == np.float32(1.0).view(np.uint32)).all()
        k = blend_weights(h, w, "hann")
        assert k.dtype == np.float32 and k.shape == (h, w)
        assert (k > 0).all() and np.isfinite(k).all()               # strictly positive: no pixel of a covered scene has wsum == 0
        assert np.array_equal(k, k[::-1, :]) and np.array_equal(k, k[:, ::-1])
        if h == w:
            assert np.array_equal(k, k.T)
        # the independent restatement (math.cos per element): libm and numpy's vector cosine may differ in the last float64 bit,
        # which moves the once-rounded float32 product by at most one unit in the last place
        r = scene_ref.blend_weights(h, w, "hann")
        assert np.abs(k.view(np.int32).astype(np.int64) - r.view(np.int32).astype(np.int64)).max() <= 1
    a = 0.5 - 0.5 * np.cos(2 * np.pi * 0.5 / 8)
    assert blend_weights(8, 8, "hann")[0, 0] == np.float32(a * a) and blend_weights(8, 8, "hann").max() < 1.0
    with pytest.raises(ValueError):
        blend_weights(8, 8, "tukey")


def test_reference_blend_of_disjoint_windows_is_the_identity():
    """uniform weights, stride == window, scene (16, 16): every pixel has one window with weight 1.0f, so 0 + 1 * x and x / 1 return
    the window logits unchanged, bit for bit"""
    rng = np.random.default_rng(5)
    ys, xs = scene_ref.window_grid(16, 16, 8, 8, 8, 8)
    assert (ys, xs) == ([0, 8], [0, 8])
    lg = rng.uniform(-8, 8, size=(4, 3, 8, 8)).astype(np.float32)
    acc, wsum = scene_ref.blend(lg, ys, xs, scene_ref.blend_weights(8, 8, "uniform"), 16, 16)
    assert (wsum == 1.0).all()
    cls, mean, soft = scene_ref.finalize(acc, wsum)
    for i in range(4):
        y0, x0 = ys[i // 2], xs[i % 2]
        assert np.array_equal(mean[:, y0:y0 + 8, x0:x0 + 8].view(np.uint32), lg[i].view(np.uint32))
        assert np.array_equal(cls[y0:y0 + 8, x0:x0 + 8], np.argmax(lg[i], axis=0))
    assert np.allclose(soft.sum(axis=0), 1.0, atol=1e-12)


def test_reference_blend_crops_overhanging_windows_and_rounds_in_window_order():
    ys, xs = scene_ref.window_grid(5, 11, 8, 8, 4, 4)
    assert (ys, xs) == ([0], [0, 3])
    lg = np.random.default_rng(6).uniform(-8, 8, size=(2, 1, 8, 8)).astype(np.float32)
    wt = scene_ref.blend_weights(8, 8, "hann")
    acc, wsum = scene_ref.blend(lg, ys, xs, wt, 5, 11)
    assert acc.shape == (1, 5, 11) and (wsum > 0).all()
    y, x = 2, 5                                                      # covered by both windows: ((0 + p0) + p1), each step rounded
    p0, p1 = np.float32(wt[2, 5] * lg[0, 0, 2, 5]), np.float32(wt[2, 2] * lg[1, 0, 2, 2])
    assert acc[0, y, x] == np.float32(np.float32(np.float32(0) + p0) + p1)
    assert wsum[y, x] == np.float32(wt[2, 5] + wt[2, 2])


def test_library_exports_the_scene_entry_points():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    for name in ("ksmi_scene_valid", "ksmi_scene_gather", "ksmi_scene_accumulate", "ksmi_scene_finalize"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and args[-1] is _lib.C.c_void_p      # a launch-list entry: int status, the stream last
    assert lib.ksmi_abi_version() == 8


def test_scene_argument_errors_need_no_device():
    """the checks run before any launch: with made-up non-null addresses a refused call returns before touching them"""
    from kurosiwo_amd import _lib
    lib = _lib.load()
    P, nan = 4096, float("nan")
    assert lib.ksmi_scene_accumulate(P, P, 2, P, 2, 0, 4, 9, 8, 8, P, P, P, 16, 16, None) < 0              # K = 9
    assert b"scene_accumulate" in lib.ksmi_last_error()
    assert lib.ksmi_scene_accumulate(P, P, 2, P, 2, 0, 4, 0, 8, 8, P, P, P, 16, 16, None) < 0              # K = 0
    assert lib.ksmi_scene_accumulate(P, P, 2, P, 2, 0, 4, 3, 0, 8, P, P, P, 16, 16, None) < 0              # h < 1
    assert lib.ksmi_scene_accumulate(P, P, 2, P, 2, 0, -1, 3, 8, 8, P, P, P, 16, 16, None) < 0             # n < 0
    assert lib.ksmi_scene_accumulate(P, P, 2, P, 2, 2, 3, 3, 8, 8, P, P, P, 16, 16, None) < 0              # i0 + n past ny * nx
    assert lib.ksmi_scene_accumulate(None, P, 2, P, 2, 0, 4, 3, 8, 8, P, P, P, 16, 16, None) < 0
    assert lib.ksmi_scene_accumulate(P, P, 2, P, 2, 0, 0, 3, 8, 8, P, P, P, 16, 16, None) == 0             # n = 0
    assert lib.ksmi_scene_gather(P, 2, 16, 16, P, 2, P, 2, 0, 4, 8, 0, None, None, None, nan, P, None) < 0  # w < 1
    assert b"scene_gather" in lib.ksmi_last_error()
    assert lib.ksmi_scene_gather(P, 2, 16, 16, P, 2, P, 2, 3, 2, 8, 8, None, None, None, nan, P, None) < 0
    assert lib.ksmi_scene_gather(P, 2, 16, 16, P, 2, P, 2, 0, 4, 8, 8, P, None, P, nan, P, None) < 0        # mean without std
    assert lib.ksmi_scene_gather(P, 2, 16, 16, None, 2, P, 2, 0, 4, 8, 8, None, None, None, nan, P, None) < 0
    assert lib.ksmi_scene_gather(P, 2, 16, 16, P, 2, P, 2, 4, 0, 8, 8, None, None, None, nan, P, None) == 0
    assert lib.ksmi_scene_valid(None, 2, 256, nan, P, 1, None) < 0
    assert lib.ksmi_scene_valid(P, 0, 256, nan, P, 1, None) < 0
    assert lib.ksmi_scene_valid(P, 2, 0, nan, P, 1, None) == 0
    assert lib.ksmi_scene_finalize(P, P, None, 9, 256, 3, P, None, 0, None) < 0
    assert b"scene_finalize" in lib.ksmi_last_error()
    assert lib.ksmi_scene_finalize(P, P, None, 3, 256, 3, None, None, 0, None) < 0
    assert lib.ksmi_scene_finalize(P, P, None, 3, 256, 3, P, None, 2, None) < 0                            # score_mode
    assert lib.ksmi_scene_finalize(P, P, None, 3, 256, 256, P, None, 0, None) < 0                          # a class that uint8 cannot hold
    assert lib.ksmi_scene_finalize(P, P, None, 3, 0, 3, P, None, 0, None) == 0


def test_predict_scene_refuses_cpu_tensors_and_bad_arguments():
    import torch
    from kurosiwo_amd import _lib
    from kurosiwo_amd.scene import predict_scene, scene_finalize, scene_gather
    x = torch.zeros(2, 16, 16)
    norm = ([0.0, 0.0], [1.0, 1.0], [0.15, 0.15])
    with pytest.raises(_lib.KsmiError):
        predict_scene(lambda xs: xs[0], [x], [norm], window=8, stride=8)
    with pytest.raises(_lib.KsmiError):
        scene_gather(x, torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), 0, 1, 8, 8)
    with pytest.raises(_lib.KsmiError):
        scene_finalize(torch.zeros(3, 4, 4), torch.ones(4, 4))
    with pytest.raises(ValueError):
        predict_scene(lambda xs: xs[0], [x], [norm], score="probabilities")
    with pytest.raises(ValueError):
        predict_scene(lambda xs: xs[0], [x], [norm, norm])
    with pytest.raises(ValueError):
        predict_scene(lambda xs: xs[0], [], [])
