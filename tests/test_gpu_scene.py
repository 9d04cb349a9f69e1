"""Whole-scene inference on the device (csrc/scene.hip, kurosiwo_amd/scene.py, predict.py): the window gather against
data.preprocess_gpu on torch crops, the gather-form blend and the finalisation against the numpy slice loop of tests/scene_ref.py,
predict_scene with a stub and with a real SNUNet-ECAM, and predict.py end to end.  Bit-exact unless stated."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIN = 8
GRIDS = [((8, 8), 5), ((5, 11), 5), ((19, 23), 5), ((17, 9), 8)]            # (scene, stride), window 8 x 8
GRID_IDS = ["8x8s5", "5x11s5", "19x23s5", "17x9s8"]
SAR_MEAN, SAR_STD, CLAMP = [0.0953, 0.0264, 0.0611], [0.0427, 0.0215, 0.0333], 0.15
DEM_MEAN, DEM_STD = 93.4313, 1410.8382
GUARD = 777.0


def _bits_differ(got, want):
    """cells whose uint32 patterns differ; a NaN meets a NaN in the same cell (payloads are not compared)"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (got.shape, want.shape)
    gn, wn = np.isnan(got), np.isnan(want)
    return int((gn != wn).sum() + (got.view(np.uint32)[~gn & ~wn] != want.view(np.uint32)[~gn & ~wn]).sum())


def _grid(scene, stride, win=WIN):
    from kurosiwo_amd.scene import window_grid
    ys, xs = window_grid(scene[0], scene[1], win, win, stride, stride)
    assert (ys.tolist(), xs.tolist()) == scene_ref.window_grid(scene[0], scene[1], win, win, stride, stride)
    return ys, xs


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _scene(C, Hs, Ws, clamps, sentinel, ys, xs, seed):
    """backscatter-like values that reach below 0 and above the clamp (terrain-like ones in an unclamped channel), with NaN on two
    scene corners, on a window border and in an interior cell, and the sentinel (where there is one) in three other such cells"""
    rng = np.random.default_rng(seed)
    z = rng.normal(0.06, 0.08, size=(C, Hs, Ws)).astype(np.float32)
    for c in range(C):
        if clamps[c] < 0:
            z[c] = rng.normal(93, 300, size=(Hs, Ws)).astype(np.float32)
    by, bx = int(ys[min(1, len(ys) - 1)]), int(xs[min(1, len(xs) - 1)])          # a window's first row / column
    z[0, 0, 0] = np.nan
    z[C - 1, Hs - 1, Ws - 1] = np.nan
    z[0, by, min(bx + 1, Ws - 1)] = np.nan
    z[C - 1, Hs // 2, Ws // 2] = np.nan
    if sentinel is not None:
        z[C - 1, 0, Ws - 1] = sentinel
        z[0, min(by + WIN - 1, Hs - 1), bx] = sentinel
        z[0, Hs // 2, max(Ws // 2 - 1, 0)] = sentinel
    return z


def _expected_windows(z, ys, xs, clamps, mean, std, sentinel):
    """[N, C, 8, 8]: inside the scene the existing preprocess kernel on the torch crop (clamped channels; the sentinel replaced by
    NaN first) or the numpy float32 expression (the unclamped channel); 0.0f outside the scene"""
    from kurosiwo_amd.data import preprocess_gpu
    C, Hs, Ws = z.shape
    zn = z.copy()
    if sentinel is not None:
        zn[zn == np.float32(sentinel)] = np.nan
    out = np.zeros((len(ys) * len(xs), C, WIN, WIN), np.float32)
    hard = [c for c in range(C) if clamps[c] >= 0]
    for i in range(out.shape[0]):
        y0, x0 = int(ys[i // len(xs)]), int(xs[i % len(xs)])
        crop = zn[:, y0:y0 + WIN, x0:x0 + WIN]
        hh, ww = crop.shape[1:]
        if hard:
            got = preprocess_gpu(_dev(crop[hard])[None], [mean[c] for c in hard], [std[c] for c in hard], CLAMP)
            out[i, hard, :hh, :ww] = got[0].cpu().numpy()
        for c in range(C):
            if clamps[c] < 0:
                m, s = np.float32(mean[c]), np.float32(std[c])
                v = np.where(np.isnan(crop[c]), m, crop[c]).astype(np.float32)
                out[i, c, :hh, :ww] = (v - m) / s
    return out, zn


@pytest.mark.parametrize("scene,stride", GRIDS, ids=GRID_IDS)
def test_gather_equals_preprocess_of_the_torch_crops(scene, stride):
    from kurosiwo_amd.scene import scene_gather
    Hs, Ws = scene
    ys, xs = _grid(scene, stride)
    dys, dxs = _dev(ys), _dev(xs)
    N = len(ys) * len(xs)
    for C in (1, 2, 3):
        variants = [[CLAMP], [-1.0]] if C == 1 else [[CLAMP] * (C - 1) + [-1.0]]
        for clamps in variants:
            mean = [DEM_MEAN if k < 0 else SAR_MEAN[c] for c, k in enumerate(clamps)]
            std = [DEM_STD if k < 0 else SAR_STD[c] for c, k in enumerate(clamps)]
            norm = tuple(torch.tensor(v, dtype=torch.float32, device="cuda") for v in (mean, std, clamps))
            for sentinel in (None, -9999.0, 0.0):
                z = _scene(C, Hs, Ws, clamps, sentinel, ys, xs, seed=100 * Hs + 10 * C + len(variants))
                want, zn = _expected_windows(z, ys, xs, clamps, mean, std, sentinel)
                dz = _dev(z)
                got = scene_gather(dz, dys, dxs, 0, N, WIN, WIN, norm, sentinel)
                assert got.shape == (N, C, WIN, WIN) and got.dtype == torch.float32
                bad = _bits_differ(got.cpu().numpy(), want)
                print(f"scene {scene} C {C} clamps {clamps} sentinel {sentinel}: {bad} of {want.size} cells differ")
                assert bad == 0, (scene, C, clamps, sentinel)
                assert torch.equal(dz.cpu().view(torch.int32), torch.from_numpy(z).view(torch.int32))       # the raster is left alone
                # outside the scene: exactly +0.0f
                raw = scene_gather(dz, dys, dxs, 0, N, WIN, WIN, None, sentinel).cpu().numpy()
                for i in range(N):
                    y0, x0 = int(ys[i // len(xs)]), int(xs[i % len(xs)])
                    hh, ww = min(WIN, Hs - y0), min(WIN, Ws - x0)
                    outside = np.ones((WIN, WIN), bool)
                    outside[:hh, :ww] = False
                    for arr in (got.cpu().numpy(), raw):
                        assert (arr[i][:, outside].view(np.uint32) == 0).all()
                    # mean = None: the raw crop, NaN where the sentinel was
                    assert _bits_differ(raw[i, :, :hh, :ww], zn[:, y0:y0 + hh, x0:x0 + ww]) == 0
                # sub-ranges write exactly their slots
                for n in sorted({1, min(3, N), N}):
                    for i0 in sorted({0, N - n, (N - n) // 2}):
                        guard = torch.full((N, C, WIN, WIN), GUARD, dtype=torch.float32, device="cuda")
                        assert scene_gather(dz, dys, dxs, i0, n, WIN, WIN, norm, sentinel, out=guard[i0:i0 + n]).data_ptr() == guard[i0:].data_ptr()
                        g = guard.cpu().numpy()
                        assert _bits_differ(g[i0:i0 + n], want[i0:i0 + n]) == 0, (i0, n)
                        assert (g[:i0] == GUARD).all() and (g[i0 + n:] == GUARD).all(), (i0, n)


def _blend_on_device(lg, dys, dxs, wt, Hs, Ws, batch):
    from kurosiwo_amd.scene import scene_accumulate
    N, K = lg.shape[:2]
    acc = torch.zeros((K, Hs, Ws), dtype=torch.float32, device="cuda")
    wsum = torch.zeros((Hs, Ws), dtype=torch.float32, device="cuda")
    for i0 in range(0, N, batch):
        scene_accumulate(lg[i0:i0 + batch].contiguous(), dys, dxs, i0, wt, acc, wsum)
    return acc, wsum


@pytest.mark.parametrize("scene,stride", GRIDS, ids=GRID_IDS)
def test_accumulate_and_finalize_equal_the_numpy_slice_loop(scene, stride):
    from kurosiwo_amd.scene import blend_weights, scene_finalize
    Hs, Ws = scene
    ys, xs = _grid(scene, stride)
    dys, dxs = _dev(ys), _dev(xs)
    N = len(ys) * len(xs)
    rng = np.random.default_rng(7 * Hs + Ws)
    for K in (1, 3, 4):
        lg = rng.uniform(-8, 8, size=(N, K, WIN, WIN)).astype(np.float32)
        cases = [("random", lg)]
        if K == 3:
            low, high = lg.copy(), lg.copy()
            low[:, 1], low[:, 2] = low[:, 0], low[:, 0] - np.float32(1)          # channels 0 and 1 tie on top everywhere: class 0
            high[:, 2], high[:, 0] = high[:, 1], high[:, 1] - np.float32(1)      # channels 1 and 2 tie on top everywhere: class 1
            cases += [("tie01", low), ("tie12", high)]
        for kind in ("uniform", "hann"):
            wt_h = blend_weights(WIN, WIN, kind)
            wt = _dev(wt_h)
            for name, logits in cases:
                want_acc, want_wsum = scene_ref.blend(logits, ys, xs, wt_h, Hs, Ws)
                assert (want_wsum > 0).all()
                valid_h = np.ones((Hs, Ws), np.uint8)
                valid_h[0, 0] = valid_h[Hs - 1, Ws // 2] = valid_h[Hs // 2, Ws - 1] = 0
                want_cls, want_mean, want_soft = scene_ref.finalize(want_acc, want_wsum, valid_h, invalid_class=3)
                runs = []
                for batch in (1, 3, N):
                    acc, wsum = _blend_on_device(_dev(logits), dys, dxs, wt, Hs, Ws, batch)
                    cls, mean = scene_finalize(acc, wsum, _dev(valid_h), "logits", 3)
                    runs.append([t.cpu().numpy() for t in (acc, wsum, mean, cls)])
                for r in runs[1:]:                                               # the batch size does not change a bit
                    assert all(_bits_differ(a.astype(np.float32), b.astype(np.float32)) == 0 for a, b in zip(runs[0], r))
                acc, wsum, mean, cls = runs[0]
                bad = [_bits_differ(acc, want_acc), _bits_differ(wsum, want_wsum), _bits_differ(mean, want_mean), int((cls != want_cls).sum())]
                print(f"scene {scene} K {K} {kind} {name}: acc / wsum / mean / class cells that differ: {bad}")
                assert bad == [0, 0, 0, 0], (scene, K, kind, name)
                ok = valid_h != 0
                assert (cls[~ok] == 3).all() and np.isnan(mean[:, ~ok]).all() and not np.isnan(mean[:, ok]).any()
                if name == "tie01":
                    assert (mean[0] == mean[1])[ok].all() and (cls[ok] == 0).all()
                if name == "tie12":
                    assert (mean[1] == mean[2])[ok].all() and (cls[ok] == 1).all()
                # without a validity map every pixel is classified, and no score is written
                cls_all, none = scene_finalize(_dev(acc), _dev(wsum), None, None, 3)
                assert none is None and np.array_equal(cls_all.cpu().numpy(), scene_ref.finalize(want_acc, want_wsum)[0])
                if K == 3:
                    # softmax of the float32 means against float64: |m| <= 8 so |t| = |m - max| <= 16 and the one rounding of the
                    # subtraction is <= 2^-24 * 16 = 9.6e-7 in the exponent, i.e. relative in e; expf <= 2 ulp = 2.4e-7; the sum of
                    # three positive terms and the division add <= 2.4e-7: relative error of p = e / S below 2.8e-6, and p <= 1
                    _, soft = scene_finalize(_dev(acc), _dev(wsum), _dev(valid_h), "softmax", 3)
                    soft = soft.cpu().numpy()
                    err = float(np.abs(soft[:, ok].astype(np.float64) - want_soft[:, ok]).max())
                    print(f"scene {scene} K 3 {kind} {name}: softmax max abs error {err:.3e} (bound 3e-6)")
                    assert np.isnan(soft[:, ~ok]).all() and err <= 3e-6


def test_scene_kernel_argument_errors():
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import stream_ptr
    from kurosiwo_amd.scene import scene_accumulate, scene_finalize, scene_gather, scene_valid
    lib = _lib.load()
    nan, st = float("nan"), stream_ptr()
    ys, xs = _dev(np.array([0, 8], np.int32)), _dev(np.array([0, 8], np.int32))
    z = torch.zeros((2, 16, 16), dtype=torch.float32, device="cuda")
    lg = torch.ones((4, 3, 8, 8), dtype=torch.float32, device="cuda")
    wt = torch.ones((8, 8), dtype=torch.float32, device="cuda")
    out = torch.full((4, 2, 8, 8), GUARD, dtype=torch.float32, device="cuda")
    acc = torch.full((3, 16, 16), GUARD, dtype=torch.float32, device="cuda")
    acc9 = torch.full((9, 16, 16), GUARD, dtype=torch.float32, device="cuda")
    wsum = torch.full((16, 16), GUARD, dtype=torch.float32, device="cuda")
    cls = torch.full((16, 16), 77, dtype=torch.uint8, device="cuda")
    valid = torch.full((16, 16), 77, dtype=torch.uint8, device="cuda")
    p = lambda t: t.data_ptr()
    gather = lambda raster=p(z), ysp=p(ys), xsp=p(xs), i0=0, n=4, h=8, w=8, o=p(out): lib.ksmi_scene_gather(
        raster, 2, 16, 16, ysp, 2, xsp, 2, i0, n, h, w, None, None, None, nan, o, st)
    assert gather(raster=None) < 0 and gather(ysp=None) < 0 and gather(xsp=None) < 0 and gather(o=None) < 0
    assert gather(h=0) < 0 and gather(w=0) < 0 and gather(n=-1) < 0 and gather(i0=-1) < 0 and gather(i0=1) < 0 and gather(i0=4, n=1) < 0
    assert gather(n=0) == 0 and gather(i0=4, n=0) == 0
    accum = lambda lgp=p(lg), ysp=p(ys), xsp=p(xs), i0=0, n=4, K=3, h=8, w=8, wp=p(wt), ap=p(acc), sp=p(wsum): lib.ksmi_scene_accumulate(
        lgp, ysp, 2, xsp, 2, i0, n, K, h, w, wp, ap, sp, 16, 16, st)
    assert accum(lgp=None) < 0 and accum(ysp=None) < 0 and accum(xsp=None) < 0 and accum(wp=None) < 0 and accum(ap=None) < 0 and accum(sp=None) < 0
    assert accum(K=9, ap=p(acc9)) < 0 and accum(K=0) < 0 and accum(h=0) < 0 and accum(n=-1) < 0 and accum(i0=2, n=3) < 0
    assert accum(n=0) == 0
    assert lib.ksmi_scene_valid(None, 2, 256, nan, p(valid), 1, st) < 0 and lib.ksmi_scene_valid(p(z), 2, 256, nan, None, 1, st) < 0
    assert lib.ksmi_scene_valid(p(z), 0, 256, nan, p(valid), 1, st) < 0 and lib.ksmi_scene_valid(p(z), 2, 0, nan, p(valid), 1, st) == 0
    fin = lambda ap=p(acc), sp=p(wsum), K=3, cp=p(cls), mode=0: lib.ksmi_scene_finalize(ap, sp, None, K, 256, 3, cp, None, mode, st)
    assert fin(ap=None) < 0 and fin(sp=None) < 0 and fin(cp=None) < 0 and fin(K=9, ap=p(acc9)) < 0 and fin(mode=2) < 0
    torch.cuda.synchronize()
    for t, v in ((out, GUARD), (acc, GUARD), (acc9, GUARD), (wsum, GUARD), (cls, 77), (valid, 77)):
        assert bool((t == v).all())                    # nothing was launched
    with pytest.raises(_lib.KsmiError):
        scene_valid(z.cpu())
    with pytest.raises(_lib.KsmiError):
        scene_accumulate(lg.cpu(), ys, xs, 0, wt, acc, wsum)
    for bad in (lambda: scene_valid(z.double()), lambda: scene_valid(z.transpose(1, 2)), lambda: scene_valid(z[0]),
                lambda: scene_gather(z, ys.long(), xs, 0, 4, 8, 8), lambda: scene_gather(z, ys, xs, 0, 4, 8, 8, out=out[:3]),
                lambda: scene_accumulate(lg, ys, xs, 0, wt, acc[:2], wsum), lambda: scene_accumulate(lg.double(), ys, xs, 0, wt, acc, wsum),
                lambda: scene_finalize(acc, wsum[:8]), lambda: scene_finalize(acc, wsum, score="both")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(_lib.KsmiError):               # the wrapper hands the library's refusal on
        scene_gather(z, ys, xs, 2, 3, 8, 8)


def _stub(xs):
    """a fixed per-pixel function of the normalised inputs, one rounding per operation -> [B, 3, h, w]"""
    a, b = xs[0][:, 0], xs[0][:, 1]
    return torch.stack((a - b, b * b, a * 0.5), dim=1)


def test_predict_scene_with_a_stub_equals_the_stub_on_the_whole_scene():
    from kurosiwo_amd.data import preprocess_gpu
    from kurosiwo_amd.scene import predict_scene
    norm = (SAR_MEAN[:2], SAR_STD[:2], [CLAMP, CLAMP])
    for (Hs, Ws), stride in (((16, 24), 8), ((5, 11), 8)):
        z = np.random.default_rng(Hs).normal(0.06, 0.08, size=(2, Hs, Ws)).astype(np.float32)
        z[1, Hs // 2, 3] = np.nan
        z[0, 1, Ws - 2] = -9999.0
        zn = z.copy()
        zn[zn == -9999.0] = np.nan
        whole = _stub([preprocess_gpu(_dev(zn)[None], norm[0], norm[1], CLAMP)])[0].cpu().numpy()
        cls, mean = predict_scene(_stub, [_dev(z)], [norm], window=WIN, stride=stride, batch=4, weight="uniform", nodata=-9999.0, score="logits")
        assert cls.shape == (Hs, Ws) and cls.dtype == torch.uint8 and mean.shape == (3, Hs, Ws)          # only in-scene cells come back
        ok = ~np.isnan(zn).any(axis=0)
        assert (~ok).sum() == 2
        cls, mean = cls.cpu().numpy(), mean.cpu().numpy()
        assert _bits_differ(mean[:, ok], whole[:, ok]) == 0
        assert np.array_equal(cls[ok], np.argmax(whole, axis=0)[ok]) and (cls[~ok] == 3).all() and np.isnan(mean[:, ~ok]).all()
        cls7, none = predict_scene(_stub, [_dev(z)], [norm], window=WIN, stride=stride, weight="uniform", nodata=-9999.0, invalid_class=7)
        assert none is None and (cls7.cpu().numpy()[~ok] == 7).all() and np.array_equal(cls7.cpu().numpy()[ok], cls[ok])


@pytest.fixture(scope="module")
def snunet_scene():
    """the seeded SNUNet-ECAM (fp32, eval) and two dates of an 80 x 72 scene with planted NaNs; window 32, stride 16: 16 windows"""
    from oracle import snunet_ref as R
    from oracle.seeded import seeded_fill_
    from kurosiwo_amd.snunet import SNUNet_ECAM
    model = SNUNet_ECAM(2, 3, base_channel=16, precision="fp32")
    model.load_state_dict(seeded_fill_(R.new_state_dict(2, 3, 16)))
    model = model.cuda().eval()
    rng = np.random.default_rng(80)
    pre, post = (rng.normal(0.06, 0.08, size=(2, 80, 72)).astype(np.float32) for _ in range(2))
    pre[0, 0, 0] = post[1, 79, 71] = post[0, 16, 33] = pre[1, 40, 40] = np.nan
    return model, pre, post


def test_predict_scene_with_a_real_model_equals_the_blend_of_its_direct_outputs(snunet_scene):
    from kurosiwo_amd.data import preprocess_gpu
    from kurosiwo_amd.scene import blend_weights, cd_forward, predict_scene
    model, pre, post = snunet_scene
    norm = (SAR_MEAN[:2], SAR_STD[:2], [CLAMP, CLAMP])
    ys, xs = _grid((80, 72), 16, 32)
    assert len(ys) * len(xs) == 16
    origins = [(int(y), int(x)) for y in ys for x in xs]
    direct = []
    with torch.no_grad():
        for i0 in range(0, 16, 5):                                               # 5, 5, 5 and a ragged batch of 1
            crops = [torch.stack([_dev(r[:, y:y + 32, x:x + 32]) for y, x in origins[i0:i0 + 5]]) for r in (pre, post)]
            xa, xb = (preprocess_gpu(c, norm[0], norm[1], CLAMP) for c in crops)
            direct.append(model(xa, xb).float().cpu().numpy())
    wt = blend_weights(32, 32, "hann")
    want_acc, want_wsum = scene_ref.blend(np.concatenate(direct), ys, xs, wt, 80, 72)
    valid = (~(np.isnan(pre).any(axis=0) | np.isnan(post).any(axis=0))).astype(np.uint8)
    want_cls, want_mean, _ = scene_ref.finalize(want_acc, want_wsum, valid)
    rasters = [_dev(pre), _dev(post)]
    cls, mean = predict_scene(cd_forward(model, "snunet"), rasters, [norm, norm], window=32, stride=16, batch=5, weight="hann", score="logits")
    cls, mean = cls.cpu().numpy(), mean.cpu().numpy()
    bad = [_bits_differ(mean, want_mean), int((cls != want_cls).sum())]
    print(f"SNUNet-ECAM scene 80 x 72: mean-logit / class cells that differ: {bad}; classes {np.bincount(cls.ravel(), minlength=4).tolist()}")
    assert bad == [0, 0]
    for y, x in ((0, 0), (79, 71), (16, 33), (40, 40)):
        assert cls[y, x] == 3
    assert (cls[valid != 0] < 3).all() and (valid == 0).sum() == 4
    try:                                                                         # the model normalises inside its first convolution
        raw_cls, _ = predict_scene(cd_forward(model, "snunet", [norm, norm]), rasters, [norm, norm], window=32, stride=16, batch=5, weight="hann",
                                   raw=True)
    finally:
        model.set_input_pipeline()
    assert np.array_equal(raw_cls.cpu().numpy(), cls)


def test_predict_script_end_to_end(tmp_path):
    from oracle import snunet_ref as R
    from oracle.seeded import seeded_fill_
    from kurosiwo_amd import geotiff
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.scene import cd_forward, predict_scene
    from kurosiwo_amd.snunet import SNUNet_ECAM
    data = load_json5(os.path.join(ROOT, "configs", "train", "data_config.json"))
    bc = load_json5(os.path.join(ROOT, "configs", "method", "snunet", "snunet.json"))["base_channel"]
    rng = np.random.default_rng(81)
    pre, post = (rng.normal(0.06, 0.08, size=(2, 80, 72)).astype(np.float32) for _ in range(2))
    post[0, 5, 7] = np.nan
    post[1, 50, 60] = pre[0, 33, 1] = -9999.0
    geo = dict(pixel_scale=(10.0, 10.0), origin=(500000.0, 4100000.0))
    geotiff.write(str(tmp_path / "post_vv.tif"), post[0], nodata=-9999.0, **geo)
    geotiff.write(str(tmp_path / "post_vh.tif"), post[1], nodata=-9999.0, **geo)
    geotiff.write(str(tmp_path / "pre.tif"), pre, nodata=-9999.0, compression="deflate", pixel_scale=(20.0, 20.0), origin=(1.0, 2.0))
    model = SNUNet_ECAM(2, 3, base_channel=bc, precision="fp32")
    model.load_state_dict(seeded_fill_(R.new_state_dict(2, 3, bc)))
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, str(tmp_path / "best.pt"))
    model = model.cuda().eval()
    norm = (data["data_mean"], data["data_std"], [data["clamp_input"]] * 2)
    want, _ = predict_scene(cd_forward(model, "snunet"), [_dev(pre), _dev(post)], [norm, norm], window=32, stride=16, batch=5, weight="hann",
                            nodata=-9999.0)
    want = want.cpu().numpy()
    assert (want[[5, 50, 33], [7, 60, 1]] == 3).all() and (want == 3).sum() == 3
    cmd = [sys.executable, os.path.join(ROOT, "predict.py"), "--task", "cd", "--method", "snunet", "--checkpoint", str(tmp_path / "best.pt"),
           "--post", str(tmp_path / "post_vv.tif"), str(tmp_path / "post_vh.tif"), "--pre1", str(tmp_path / "pre.tif"),
           "--out", str(tmp_path / "flood.tif"), "--window", "32", "--stride", "16", "--batch_size", "5", "--precision", "fp32"]
    run = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got, meta = geotiff.read(str(tmp_path / "flood.tif"))
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert meta["pixel_scale"] == (10.0, 10.0) and meta["origin"] == (500000.0, 4100000.0) and meta["nodata"] == 3.0
    assert meta["compression"] == 8 and meta["tiled"] == 1
    refused = subprocess.run(cmd + ["--slope"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--slope is not supported" in refused.stderr
