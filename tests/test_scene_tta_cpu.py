"""Test-time views of the whole-scene blend, host half: the numpy restatement (tests/scene_tta_ref.py) is a group of eight different
symmetries with the inverses it claims, the package's view sets, predict_scene's refusal of unknown sets, the argument checks of
the three ksmi_scene_*view* entry points (they launch nothing) and predict.py's --tta option.  No GPU."""
import numpy as np
import pytest

import scene_tta_ref as ref


def _tile(h, w, seed=3):
    """an asymmetric tile: no symmetry of the square maps it onto itself"""
    return np.random.default_rng(seed).uniform(-8, 8, size=(2, h, w)).astype(np.float32)


def test_unview_inverts_every_view():
    t = _tile(7, 7)
    for v in range(8):
        u = ref.view(t, v)
        assert u.shape == t.shape and np.array_equal(ref.unview(u, v).view(np.uint32), t.view(np.uint32)), v
        assert np.array_equal(ref.view(ref.unview(t, v), v), t), v
    r = _tile(5, 9)                                                    # the flips need no square
    for v in range(4):
        assert ref.view(r, v).shape == r.shape and np.array_equal(ref.unview(ref.view(r, v), v), r), v


def test_the_eight_views_are_pairwise_different_and_follow_the_definition():
    t = _tile(6, 6)
    views = [ref.view(t, v) for v in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert not np.array_equal(views[a], views[b]), (a, b)
    h = w = 6
    for v in range(8):                                                 # cell by cell: the transpose first, then flip y, then flip x
        for uy in range(h):
            for ux in range(w):
                ay, ax = (h - 1 - uy if v & 2 else uy), (w - 1 - ux if v & 1 else ux)
                ly, lx = (ax, ay) if v & 4 else (ay, ax)
                assert views[v][0, uy, ux] == t[0, ly, lx]
    assert np.array_equal(views[1], t[..., ::-1]) and np.array_equal(views[2], t[..., ::-1, :]) and np.array_equal(views[4], t.swapaxes(-1, -2))
    assert np.array_equal(views[5], np.rot90(t, -1, axes=(-2, -1)))   # transpose, then flip x: a quarter turn clockwise


def test_view_sets_are_ascending_and_match_the_reference():
    from kurosiwo_amd.scene import VIEW_SETS
    assert VIEW_SETS == ref.VIEW_SETS == {"hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": tuple(range(8))}
    for codes in VIEW_SETS.values():
        assert list(codes) == sorted(set(codes)) and codes[0] == 0


def test_reference_blend_of_one_view_is_the_plain_blend_and_views_sit_inside_the_window_loop():
    import scene_ref
    rng = np.random.default_rng(11)
    ys, xs = scene_ref.window_grid(5, 11, 8, 8, 4, 4)
    lg = rng.uniform(-8, 8, size=(3, 2, 1, 8, 8)).astype(np.float32)
    wt = scene_ref.blend_weights(8, 8, "hann")
    one = ref.blend_views(lg[:1], ys, xs, wt, 5, 11)
    plain = scene_ref.blend(lg[0], ys, xs, wt, 5, 11)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(one, plain))
    acc, wsum = ref.blend_views(lg, ys, xs, wt, 5, 11)
    f = np.float32
    step = f(0)
    for i, lx in ((0, 5), (1, 2)):                                     # pixel (2, 5): window 0 at column 5, window 1 (origin 3) at column 2
        for v in range(3):
            step = f(step + f(wt[2, lx] * lg[v, i, 0, 2, lx]))
    assert acc[0, 2, 5] == step
    assert wsum[2, 5] == f(f(f(f(f(wt[2, 5] + wt[2, 5]) + wt[2, 5]) + wt[2, 2]) + wt[2, 2]) + wt[2, 2])


def test_predict_scene_refuses_unknown_view_sets():
    import torch
    from kurosiwo_amd import _lib
    from kurosiwo_amd.scene import predict_scene
    x = torch.zeros(2, 16, 16)
    norm = ([0.0, 0.0], [1.0, 1.0], [0.15, 0.15])
    for bad in ("rot", (8,), (-1,), (), (0, 0), (0.5,), 3, "D4"):
        with pytest.raises(ValueError):
            predict_scene(lambda xs: xs[0], [x], [norm], window=8, stride=8, tta=bad)
    for good in (None, "none", "hflip", "flips", "d4", (0,), (5, 0), [1, 2]):      # accepted: the next refusal is the CPU tensor's
        with pytest.raises(_lib.KsmiError):
            predict_scene(lambda xs: xs[0], [x], [norm], window=8, stride=8, tta=good)


def test_wrappers_refuse_cpu_tensors_and_bad_views():
    import torch
    from kurosiwo_amd import _lib
    from kurosiwo_amd.scene import scene_accumulate_views, scene_gather_view, scene_unview
    o = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(_lib.KsmiError):
        scene_gather_view(torch.zeros(2, 16, 16), o, o, 0, 1, 8, 8, 1)
    with pytest.raises(_lib.KsmiError):
        scene_unview(torch.zeros(3, 8, 8), 1)
    with pytest.raises(_lib.KsmiError):
        scene_accumulate_views(torch.zeros(2, 1, 3, 8, 8), o, o, 0, torch.ones(8, 8), torch.zeros(3, 16, 16), torch.zeros(16, 16))
    for view in (8, -1, 1.0, None, True):
        with pytest.raises(ValueError):
            scene_gather_view(torch.zeros(2, 16, 16), o, o, 0, 1, 8, 8, view)
    with pytest.raises(ValueError):
        scene_gather_view(torch.zeros(2, 16, 16), o, o, 0, 1, 8, 6, 4)         # a transposed view of a window that is not square


def test_library_exports_the_view_entry_points():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    for name in ("ksmi_scene_gather_view", "ksmi_scene_unview", "ksmi_scene_accumulate_views"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and args[-1] is _lib.C.c_void_p
    assert lib.ksmi_abi_version() == 8


def test_view_argument_errors_need_no_device():
    """the checks run before any launch: with made-up non-null addresses a refused call returns before touching them"""
    from kurosiwo_amd import _lib
    lib = _lib.load()
    P, nan = 4096, float("nan")
    gather = lambda raster=P, i0=0, n=4, h=8, w=8, view=1, out=P: lib.ksmi_scene_gather_view(
        raster, 2, 16, 16, P, 2, P, 2, i0, n, h, w, None, None, None, nan, view, out, None)
    for refused in (dict(view=8), dict(view=-1), dict(view=4, h=8, w=6), dict(view=7, h=6, w=8), dict(raster=None), dict(out=None),
                    dict(n=-1), dict(i0=2, n=3), dict(h=0), dict(view=8, n=0), dict(view=5, h=8, w=6, n=0)):
        assert gather(**refused) < 0, refused
        assert b"scene_gather_view" in lib.ksmi_last_error(), refused
    assert lib.ksmi_scene_gather_view(P, 2, 16, 16, P, 2, P, 2, 0, 4, 8, 8, P, None, P, nan, 1, P, None) < 0        # mean without std
    assert gather(n=0) == 0 and gather(i0=4, n=0, view=7) == 0 and gather(n=0, h=8, w=6, view=3) == 0

    unview = lambda src=P, dst=2 * P, planes=5, h=8, w=8, view=1: lib.ksmi_scene_unview(src, dst, planes, h, w, view, None)
    for refused in (dict(view=8), dict(view=-1), dict(view=4, h=8, w=6), dict(view=6, h=6, w=8), dict(planes=-1), dict(src=None),
                    dict(dst=None), dict(dst=P), dict(h=0), dict(w=0), dict(view=8, planes=0), dict(view=4, h=8, w=6, planes=0)):
        assert unview(**refused) < 0, refused
        assert b"scene_unview" in lib.ksmi_last_error(), refused
    assert unview(planes=0) == 0 and unview(planes=0, view=7) == 0 and unview(planes=0, h=8, w=13, view=3) == 0

    blend = lambda lg=P, V=2, i0=0, n=4, K=3, h=8, acc=P: lib.ksmi_scene_accumulate_views(
        lg, V, P, 2, P, 2, i0, n, K, h, 8, P, acc, P, 16, 16, None)
    for refused in (dict(V=0), dict(V=9), dict(V=-1), dict(K=0), dict(K=9), dict(lg=None), dict(acc=None), dict(n=-1), dict(i0=2, n=3),
                    dict(h=0), dict(V=9, n=0), dict(K=9, n=0)):
        assert blend(**refused) < 0, refused
        assert b"scene_accumulate_views" in lib.ksmi_last_error(), refused
    assert blend(n=0) == 0 and blend(n=0, V=8, K=8) == 0 and blend(i0=4, n=0, V=1) == 0


def test_predict_parser_takes_the_view_sets():
    import predict
    for name in ("none", "hflip", "flips", "d4"):
        args = predict.parser.parse_args(["--method", "snunet", "--checkpoint", "c.pt", "--post", "p.tif", "--out", "o.tif", "--tta", name])
        assert args.tta == name
    assert predict.parser.parse_args(["--method", "snunet", "--checkpoint", "c.pt", "--post", "p.tif", "--out", "o.tif"]).tta == "none"
    with pytest.raises(SystemExit):
        predict.parser.parse_args(["--method", "snunet", "--checkpoint", "c.pt", "--post", "p.tif", "--out", "o.tif", "--tta", "rot"])
    for name in ("hflip", "flips", "d4"):                              # the docstring names what the option takes
        assert name in predict.__doc__
