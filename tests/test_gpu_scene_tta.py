"""Test-time views of the whole-scene blend on the device (csrc/scene.hip: ksmi_scene_gather_view, ksmi_scene_unview,
ksmi_scene_accumulate_views; kurosiwo_amd/scene.py: predict_scene(tta=...); predict.py --tta) against the numpy restatement of
tests/scene_tta_ref.py.  Every comparison is of uint32 patterns unless stated."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_ref
import scene_tta_ref as ref
from test_gpu_scene import GRID_IDS, GRIDS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIN = 8
SAR_MEAN, SAR_STD, CLAMP = [0.0953, 0.0264, 0.0611], [0.0427, 0.0215, 0.0333], 0.15
GUARD = 777.0
SENTINEL = -9999.0
# (window, scene, stride): windows below, at, one past and no multiple of the 64-cell tile of the transposed views, each on a scene a
# few pixels larger than the window and not stride-aligned (the last window of an axis is pushed back to end at the border); then
# scenes smaller than the window, where the overhang's zeros must land at the viewed positions
GATHER_CASES = [(8, (13, 17), 5), (64, (69, 73), 33), (65, (70, 74), 33), (133, (138, 142), 67), (8, (5, 11), 5), (64, (40, 70), 33)]
GATHER_IDS = ["w8", "w64", "w65", "w133", "w8-small", "w64-small"]
UNVIEW_SIZES = [(8, 8), (64, 64), (65, 65), (133, 133), (8, 13), (64, 70)]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    a = t.cpu().numpy() if torch.is_tensor(t) else np.ascontiguousarray(t)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _differ(got, want):
    """cells whose bit patterns differ, NaN payloads included"""
    got, want = _bits(got), _bits(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    return int((got != want).sum())


def _grid(scene, stride, win):
    from kurosiwo_amd.scene import window_grid
    ys, xs = window_grid(scene[0], scene[1], win, win, stride, stride)
    assert (ys.tolist(), xs.tolist()) == scene_ref.window_grid(scene[0], scene[1], win, win, stride, stride)
    return ys, xs


def _raster(C, Hs, Ws, seed):
    """backscatter-like values below 0 and above the clamp, NaN and the sentinel on corners and inside"""
    z = np.random.default_rng(seed).normal(0.06, 0.08, size=(C, Hs, Ws)).astype(np.float32)
    z[0, 0, 0] = z[C - 1, Hs - 1, Ws - 1] = z[0, Hs // 2, Ws // 3] = np.nan
    z[C - 1, 0, Ws - 1] = z[0, Hs - 1, 0] = z[0, Hs // 3, Ws // 2] = SENTINEL
    return z


# ---------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize("win,scene,stride", GATHER_CASES, ids=GATHER_IDS)
def test_gather_view_equals_the_view_of_the_gather(win, scene, stride):
    from kurosiwo_amd.scene import scene_gather, scene_gather_view
    Hs, Ws = scene
    ys, xs = _grid(scene, stride, win)
    if Hs > win:
        assert len(ys) >= 2 and ys[-1] + win == Hs and xs[-1] + win == Ws and xs[-1] % stride != 0    # a pushed-back last window
    dys, dxs = _dev(ys), _dev(xs)
    N = len(ys) * len(xs)
    for C in (1, 3):
        norm = tuple(torch.tensor(v[:C], dtype=torch.float32, device="cuda") for v in (SAR_MEAN, SAR_STD, [CLAMP] * 3))
        z = _raster(C, Hs, Ws, seed=1000 * win + C)
        dz = _dev(z)
        for nm, sentinel in ((norm, None), (norm, SENTINEL), (None, SENTINEL)):
            plain = scene_gather(dz, dys, dxs, 0, N, win, win, nm, sentinel).cpu().numpy()
            assert np.isnan(plain).any() == (nm is None)
            outside = np.ones((N, 1, win, win), bool)                                   # the cells of a window outside the scene
            for i in range(N):
                outside[i, :, :max(min(win, Hs - int(ys[i // len(xs)])), 0), :max(min(win, Ws - int(xs[i % len(xs)])), 0)] = False
            assert outside.any() == (Hs < win or Ws < win)
            for v in range(8):
                got = scene_gather_view(dz, dys, dxs, 0, N, win, win, v, nm, sentinel)
                assert got.shape == (N, C, win, win) and got.dtype == torch.float32
                got = got.cpu().numpy()
                bad = _differ(got, ref.view(plain, v))
                print(f"window {win} scene {scene} C {C} norm {nm is not None} sentinel {sentinel} view {v}: {bad} of {got.size} cells differ")
                assert bad == 0, (win, C, sentinel, v)
                gone = np.broadcast_to(ref.view(outside, v), got.shape)
                assert (got.view(np.uint32)[gone] == 0).all()                           # exactly +0.0f, at the viewed positions
            assert _differ(scene_gather_view(dz, dys, dxs, 0, N, win, win, 0, nm, sentinel), plain) == 0
        # sub-ranges write exactly their slots; one flipped and one transposed view
        want = {v: ref.view(scene_gather(dz, dys, dxs, 0, N, win, win, norm, SENTINEL).cpu().numpy(), v) for v in (3, 6)}
        for v in (3, 6):
            for n in sorted({1, min(3, N), N}):
                for i0 in sorted({0, N - n, (N - n) // 2}):
                    guard = torch.full((N, C, win, win), GUARD, dtype=torch.float32, device="cuda")
                    out = scene_gather_view(dz, dys, dxs, i0, n, win, win, v, norm, SENTINEL, out=guard[i0:i0 + n])
                    assert out.data_ptr() == guard[i0:].data_ptr()
                    g = guard.cpu().numpy()
                    assert _differ(g[i0:i0 + n], want[v][i0:i0 + n]) == 0, (v, i0, n)
                    assert (g[:i0] == GUARD).all() and (g[i0 + n:] == GUARD).all(), (v, i0, n)
        assert _differ(dz, z) == 0                                                      # the raster is left alone


# ---------------------------------------------------------------------------------------------------- unview
@pytest.mark.parametrize("size", UNVIEW_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_unview_inverts_the_reference_view_bit_for_bit(size):
    from kurosiwo_amd.scene import scene_unview
    h, w = size
    pad = 3 * w + 5
    for planes in (1, 5):
        x = np.random.default_rng(h * w + planes).uniform(-8, 8, size=(planes, h, w)).astype(np.float32)
        xb = x.view(np.uint32)
        for j, payload in enumerate((0x7FC00000, 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF)):     # quiet, signalling, negative
            xb[j % planes, (j * 3) % h, (j * 5 + 1) % w] = payload
        xb[planes - 1, h - 1, w - 1] = 0x7FD55555
        xb[0, 0, 0] = 0x80000000                                                        # -0.0f
        assert np.isnan(x).sum() == 6
        for v in range(8 if h == w else 4):
            u = ref.view(x, v)
            du = _dev(u)
            buf = torch.full((pad + x.size + pad,), GUARD, dtype=torch.float32, device="cuda")
            out = buf[pad:pad + x.size].view(planes, h, w)
            assert scene_unview(du, v, out=out).data_ptr() == out.data_ptr()
            b = buf.cpu().numpy()
            bad = _differ(b[pad:pad + x.size].reshape(x.shape), x)
            print(f"{h} x {w} planes {planes} view {v}: {bad} of {x.size} cells differ")
            assert bad == 0, (size, planes, v)
            assert (b[:pad] == GUARD).all() and (b[pad + x.size:] == GUARD).all()
            assert _differ(du, u) == 0                                                  # the input is left alone
            assert _differ(scene_unview(du, v), x) == 0                                 # and a buffer of its own
    for bad in (lambda: scene_unview(du, 8), lambda: scene_unview(du.double(), 1), lambda: scene_unview(du, 1, out=du[:1]),
                lambda: scene_unview(du.transpose(1, 2), 1)):
        with pytest.raises(ValueError):
            bad()
    if h != w:
        with pytest.raises(ValueError):
            scene_unview(du, 4)


# ---------------------------------------------------------------------------------------------------- blend
def _splits(N):
    """launch boundaries over [0, N): every uniform batch size, and two ragged splits"""
    cuts = [list(range(0, N, b)) + [N] for b in range(1, N + 1)]
    if N >= 4:
        cuts += [[0, 1, N], [0, N - 1, N], [0, 2, 3, N]]
    return [c for j, c in enumerate(cuts) if c not in cuts[:j]]


@pytest.mark.parametrize("scene,stride", GRIDS, ids=GRID_IDS)
def test_accumulate_views_equals_the_numpy_loop_whatever_the_launches(scene, stride):
    from kurosiwo_amd.scene import blend_weights, scene_accumulate, scene_accumulate_views
    Hs, Ws = scene
    ys, xs = _grid(scene, stride, WIN)
    dys, dxs = _dev(ys), _dev(xs)
    N = len(ys) * len(xs)
    rng = np.random.default_rng(13 * Hs + Ws)
    for kind in ("hann", "uniform"):
        wt_h = blend_weights(WIN, WIN, kind)
        wt = _dev(wt_h)
        for K in (1, 3, 8):
            full = rng.uniform(-8, 8, size=(8, N, K, WIN, WIN)).astype(np.float32)
            for V in (1, 2, 4, 8):
                if kind == "uniform" and (V, K) != (4, 3):
                    continue
                lg = full[:V]
                want_acc, want_wsum = ref.blend_views(lg, ys, xs, wt_h, Hs, Ws)
                dlg = _dev(lg)
                runs = []
                for cuts in _splits(N):
                    acc = torch.zeros((K, Hs, Ws), dtype=torch.float32, device="cuda")
                    wsum = torch.zeros((Hs, Ws), dtype=torch.float32, device="cuda")
                    for a, b in zip(cuts, cuts[1:]):
                        scene_accumulate_views(dlg[:, a:b].contiguous(), dys, dxs, a, wt, acc, wsum)
                    runs.append((acc.cpu().numpy(), wsum.cpu().numpy()))
                bad = [_differ(runs[0][0], want_acc), _differ(runs[0][1], want_wsum)]
                print(f"scene {scene} {kind} K {K} V {V}: acc / wsum cells that differ: {bad}; {len(runs)} splits")
                assert bad == [0, 0], (scene, kind, K, V)
                for acc_h, wsum_h in runs[1:]:                                          # the launches do not change a bit
                    assert _differ(acc_h, runs[0][0]) == 0 and _differ(wsum_h, runs[0][1]) == 0
                if V == 1:
                    acc = torch.zeros((K, Hs, Ws), dtype=torch.float32, device="cuda")
                    wsum = torch.zeros((Hs, Ws), dtype=torch.float32, device="cuda")
                    scene_accumulate(dlg[0], dys, dxs, 0, wt, acc, wsum)
                    assert _differ(acc, runs[0][0]) == 0 and _differ(wsum, runs[0][1]) == 0


def test_view_wrappers_hand_on_refusals_and_launch_nothing():
    from kurosiwo_amd import _lib
    from kurosiwo_amd.scene import scene_accumulate_views, scene_gather_view
    ys, xs = _dev(np.array([0, 8], np.int32)), _dev(np.array([0, 8], np.int32))
    z = torch.zeros((2, 16, 16), dtype=torch.float32, device="cuda")
    lg = torch.ones((2, 4, 3, 8, 8), dtype=torch.float32, device="cuda")
    wt = torch.ones((8, 8), dtype=torch.float32, device="cuda")
    acc = torch.full((3, 16, 16), GUARD, dtype=torch.float32, device="cuda")
    wsum = torch.full((16, 16), GUARD, dtype=torch.float32, device="cuda")
    with pytest.raises(_lib.KsmiError):
        scene_gather_view(z, ys, xs, 2, 3, 8, 8, 5)                                     # i0 + n past the grid
    with pytest.raises(_lib.KsmiError):
        scene_accumulate_views(lg, ys, xs, 2, wt, acc, wsum)
    for bad in (lambda: scene_accumulate_views(lg[0], ys, xs, 0, wt, acc, wsum), lambda: scene_accumulate_views(lg, ys, xs, 0, wt, acc[:2], wsum),
                lambda: scene_accumulate_views(lg.double(), ys, xs, 0, wt, acc, wsum), lambda: scene_gather_view(z, ys, xs, 0, 4, 8, 8, 8),
                lambda: scene_gather_view(z, ys, xs, 0, 4, 8, 6, 4)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert bool((acc == GUARD).all()) and bool((wsum == GUARD).all())


# ---------------------------------------------------------------------------------------------------- predict_scene
def _ramp(h, w):
    """an asymmetric ramp over the window cell, exact in float32: no symmetry of the square keeps it"""
    ly, lx = np.arange(h, dtype=np.float32)[:, None], np.arange(w, dtype=np.float32)[None, :]
    return (np.float32(0.5) + ly * np.float32(1 / 16) + lx * np.float32(1 / 64)).astype(np.float32)


def _ramp_stub(xs):
    """logits that depend on where in the window a cell sits: the input times the ramp, one rounding per operation.  Works on the
    torch batches of predict_scene and on numpy arrays alike."""
    x = xs[0]
    a, b = x[:, 0], x[:, 1]
    r = _ramp(x.shape[-2], x.shape[-1])
    if torch.is_tensor(x):
        r = torch.from_numpy(r).to(x.device)
        return torch.stack((a * r, b * r, (a - b) * 0.5 * r), dim=1)
    return np.stack((a * r, b * r, (a - b) * np.float32(0.5) * r), axis=1).astype(np.float32)


def _pointwise_stub(xs):
    a, b = xs[0][:, 0], xs[0][:, 1]
    return torch.stack((a - b, b * b, a * 0.5), dim=1)


@pytest.fixture(scope="module")
def stub_scene():
    """a 19 x 23 scene of two channels (window 8, stride 5: 16 windows, the last of each axis pushed back), its normalised windows
    from scene_gather, and per view set the reference pipeline: view, stub, unview, blend_views, finalize"""
    from kurosiwo_amd.scene import blend_weights, scene_gather
    Hs, Ws = 19, 23
    z = np.random.default_rng(19).normal(0.06, 0.08, size=(2, Hs, Ws)).astype(np.float32)
    z[1, 9, 3] = np.nan
    z[0, 1, 21] = SENTINEL
    norm = (SAR_MEAN[:2], SAR_STD[:2], [CLAMP, CLAMP])
    ys, xs = _grid((Hs, Ws), 5, WIN)
    dev_norm = tuple(torch.tensor(v, dtype=torch.float32, device="cuda") for v in norm)
    tiles = scene_gather(_dev(z), _dev(ys), _dev(xs), 0, len(ys) * len(xs), WIN, WIN, dev_norm, SENTINEL).cpu().numpy()
    valid = np.ones((Hs, Ws), np.uint8)
    valid[9, 3] = valid[1, 21] = 0
    wt = blend_weights(WIN, WIN, "hann")
    want = {}
    for name, views in ref.VIEW_SETS.items():
        lg = np.stack([ref.unview(_ramp_stub([ref.view(tiles, v)]), v) for v in views])
        want[name] = scene_ref.finalize(*ref.blend_views(lg, ys, xs, wt, Hs, Ws), valid, invalid_class=3)
    return z, norm, valid, want


def _predict(z, norm, stub=_ramp_stub, **kw):
    from kurosiwo_amd.scene import predict_scene
    kw = {**dict(window=WIN, stride=5, batch=3, weight="hann", nodata=SENTINEL, score="logits"), **kw}
    cls, score = predict_scene(stub, [_dev(z)], [norm], **kw)
    return cls.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("name", ["hflip", "flips", "d4"])
def test_predict_scene_view_sets_equal_the_reference_pipeline(stub_scene, name):
    z, norm, valid, want = stub_scene
    want_cls, want_mean, want_soft = want[name]
    cls, mean = _predict(z, norm, tta=name)
    bad = [_differ(mean, want_mean), int((cls != want_cls).sum())]
    print(f"tta {name}: mean-logit / class cells that differ: {bad}; classes {np.bincount(cls.ravel(), minlength=4).tolist()}")
    assert bad == [0, 0]
    ok = valid != 0
    assert (cls[~ok] == 3).all() and np.isnan(mean[:, ~ok]).all() and not np.isnan(mean[:, ok]).any()
    # a missing inverse or a swapped order would show: the views differ from one another and from the single pass
    assert _differ(mean, _predict(z, norm)[1]) > 0 and _differ(want_mean, want["d4" if name != "d4" else "flips"][1]) > 0
    # softmax as tests/test_gpu_scene.py compares it: |m| <= 8 and K = 3, so the float32 steps stay below 3e-6 of the float64 value
    assert np.abs(mean[:, ok]).max() <= 8
    cls_s, soft = _predict(z, norm, tta=name, score="softmax")
    err = float(np.abs(soft[:, ok].astype(np.float64) - want_soft[:, ok]).max())
    print(f"tta {name}: softmax max abs error {err:.3e} (bound 3e-6)")
    assert np.array_equal(cls_s, cls) and np.isnan(soft[:, ~ok]).all() and err <= 3e-6


def test_predict_scene_views_do_not_depend_on_the_batch_size(stub_scene):
    z, norm, _, want = stub_scene
    for name in ("hflip", "d4"):
        runs = [_predict(z, norm, tta=name, batch=b) for b in (1, 3, 32)]
        for cls, mean in runs:
            assert _differ(mean, want[name][1]) == 0 and np.array_equal(cls, want[name][0])


def test_predict_scene_identity_view_gives_the_bits_of_the_single_pass(stub_scene):
    z, norm, _, _ = stub_scene
    base = _predict(z, norm, tta=None)
    for tta in ("none", (0,), [0]):
        cls, mean = _predict(z, norm, tta=tta)
        assert np.array_equal(cls, base[0]) and _differ(mean, base[1]) == 0, tta
    cls, mean = _predict(z, norm, tta=(3, 0, 1, 2))                                     # a tuple is taken in ascending code
    assert np.array_equal(cls, _predict(z, norm, tta="flips")[0]) and _differ(mean, _predict(z, norm, tta="flips")[1]) == 0


def test_hflip_of_a_pointwise_model_on_disjoint_windows_is_the_single_pass():
    """uniform weight and stride == window: every pixel has one window, so the two views give l + l over 1 + 1, and 2l / 2 is l
    (the larger sets pass through 3l, which rounds)"""
    z = np.random.default_rng(16).normal(0.06, 0.08, size=(2, 16, 24)).astype(np.float32)
    z[1, 8, 3] = np.nan
    norm = (SAR_MEAN[:2], SAR_STD[:2], [CLAMP, CLAMP])
    kw = dict(stub=_pointwise_stub, stride=WIN, batch=4, weight="uniform")
    base = _predict(z, norm, **kw)
    cls, mean = _predict(z, norm, tta="hflip", **kw)
    assert np.array_equal(cls, base[0]) and _differ(mean, base[1]) == 0


# ---------------------------------------------------------------------------------------------------- a real model
def test_predict_scene_flips_with_a_real_model_equal_the_torch_restatement():
    """SNUNet-ECAM (fp32, eval) over an 80 x 72 scene, window 32, stride 16, batches of 5: torch.flip of the scene_gather tiles, the
    same model on the same batch composition, the torch un-flip, then the numpy blend"""
    from oracle import snunet_ref as R
    from oracle.seeded import seeded_fill_
    from kurosiwo_amd.scene import blend_weights, cd_forward, predict_scene, scene_gather
    from kurosiwo_amd.snunet import SNUNet_ECAM
    model = SNUNet_ECAM(2, 3, base_channel=16, precision="fp32")
    model.load_state_dict(seeded_fill_(R.new_state_dict(2, 3, 16)))
    model = model.cuda().eval()
    rng = np.random.default_rng(80)
    pre, post = (rng.normal(0.06, 0.08, size=(2, 80, 72)).astype(np.float32) for _ in range(2))
    pre[0, 0, 0] = post[1, 79, 71] = post[0, 16, 33] = pre[1, 40, 40] = np.nan
    norm = (SAR_MEAN[:2], SAR_STD[:2], [CLAMP, CLAMP])
    dev_norm = tuple(torch.tensor(v, dtype=torch.float32, device="cuda") for v in norm)
    ys, xs = _grid((80, 72), 16, 32)
    dys, dxs = _dev(ys), _dev(xs)
    rasters = [_dev(pre), _dev(post)]
    dims = {0: None, 1: (-1,), 2: (-2,), 3: (-2, -1)}
    flip = lambda t, v: t if dims[v] is None else torch.flip(t, dims[v])
    direct = [[] for _ in range(4)]
    with torch.no_grad():
        for i0 in range(0, 16, 5):                                                      # 5, 5, 5 and a ragged batch of 1
            n = min(5, 16 - i0)
            xa, xb = (scene_gather(r, dys, dxs, i0, n, 32, 32, dev_norm, None) for r in rasters)
            for v in range(4):
                out = model(flip(xa, v).contiguous(), flip(xb, v).contiguous()).float()
                direct[v].append(flip(out, v).cpu().numpy())
    lg = np.stack([np.concatenate(d) for d in direct])
    assert lg.shape == (4, 16, 3, 32, 32) and _differ(lg[0], lg[1]) > 0
    want_acc, want_wsum = ref.blend_views(lg, ys, xs, blend_weights(32, 32, "hann"), 80, 72)
    valid = (~(np.isnan(pre).any(axis=0) | np.isnan(post).any(axis=0))).astype(np.uint8)
    want_cls, want_mean, _ = scene_ref.finalize(want_acc, want_wsum, valid)
    cls, mean = predict_scene(cd_forward(model, "snunet"), rasters, [norm, norm], window=32, stride=16, batch=5, weight="hann", score="logits",
                              tta="flips")
    cls, mean = cls.cpu().numpy(), mean.cpu().numpy()
    bad = [_differ(mean, want_mean), int((cls != want_cls).sum())]
    print(f"SNUNet-ECAM scene 80 x 72, flips: mean-logit / class cells that differ: {bad}; classes {np.bincount(cls.ravel(), minlength=4).tolist()}")
    assert bad == [0, 0]
    assert (cls[valid == 0] == 3).all() and (cls[valid != 0] < 3).all() and (valid == 0).sum() == 4


# ---------------------------------------------------------------------------------------------------- predict.py
def test_predict_script_with_views(tmp_path):
    from oracle import snunet_ref as R
    from oracle.seeded import seeded_fill_
    from kurosiwo_amd import geotiff
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.scene import cd_forward, predict_scene
    from kurosiwo_amd.snunet import SNUNet_ECAM
    data = load_json5(os.path.join(ROOT, "configs", "train", "data_config.json"))
    bc = load_json5(os.path.join(ROOT, "configs", "method", "snunet", "snunet.json"))["base_channel"]
    rng = np.random.default_rng(82)
    pre, post = (rng.normal(0.06, 0.08, size=(2, 80, 72)).astype(np.float32) for _ in range(2))
    post[0, 5, 7] = np.nan
    post[1, 50, 60] = pre[0, 33, 1] = SENTINEL
    geotiff.write(str(tmp_path / "post.tif"), post, nodata=SENTINEL, pixel_scale=(10.0, 10.0), origin=(500000.0, 4100000.0))
    geotiff.write(str(tmp_path / "pre.tif"), pre, nodata=SENTINEL, pixel_scale=(10.0, 10.0), origin=(500000.0, 4100000.0))
    model = SNUNet_ECAM(2, 3, base_channel=bc, precision="fp32")
    model.load_state_dict(seeded_fill_(R.new_state_dict(2, 3, bc)))
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, str(tmp_path / "best.pt"))
    model = model.cuda().eval()
    norm = (data["data_mean"], data["data_std"], [data["clamp_input"]] * 2)
    want, _ = predict_scene(cd_forward(model, "snunet"), [_dev(pre), _dev(post)], [norm, norm], window=32, stride=16, batch=5, weight="hann",
                            nodata=SENTINEL, tta="hflip")
    want = want.cpu().numpy()
    assert (want == 3).sum() == 3
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--task", "cd", "--method", "snunet", "--checkpoint", str(tmp_path / "best.pt"),
           "--post", str(tmp_path / "post.tif"), "--pre1", str(tmp_path / "pre.tif"), "--window", "32", "--stride", "16", "--batch_size", "5",
           "--precision", "fp32"]
    run = subprocess.run(cmd + ["--out", str(tmp_path / "hflip.tif"), "--tta", "hflip"], cwd=str(tmp_path), capture_output=True, text=True,
                         timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got, meta = geotiff.read(str(tmp_path / "hflip.tif"))
    assert got.dtype == np.uint8 and np.array_equal(got, want) and meta["nodata"] == 3.0
    run = subprocess.run(cmd + ["--out", str(tmp_path / "d4.tif"), "--tta", "d4"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got, _ = geotiff.read(str(tmp_path / "d4.tif"))
    assert got.dtype == np.uint8 and got.shape == (80, 72) and (got[[5, 50, 33], [7, 60, 1]] == 3).all() and (got == 3).sum() == 3
