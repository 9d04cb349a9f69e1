"""--dem --slope on the device: the stencil kernel (csrc/terrain.hip: ksmi_dem_slope) against kurosiwo_amd.dataset.slope_riserun, bit for
bit (tests/test_slope_cpu.py pins that function by hand); the batch loaders with slope against the per-sample Dataset classes; the
routing of prepare_loaders and the fused first convolution of SNUNet on the slope channel.  Bit-exact throughout."""
import gzip
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))

from test_dataset_cpu import TRAIN, VAL, TEST, _configs            # noqa: E402

F32_SENTINEL = float(np.float32(3.4e38))
SHAPES = [(1, 1, 1), (2, 1, 5), (2, 5, 1), (3, 2, 2), (3, 5, 7), (2, 17, 23), (1, 224, 224)]
SENTINELS = [None, F32_SENTINEL, 3.4e38, -9999.0]
SLOPE_MEAN, SLOPE_STD = 2.1277, 67.5048


def _tiles(n, H, W, sentinel):
    """normal(93, 300) as fp32 with: NaN in the first cell of tile 0 and the last cell of the last tile, a NaN block [1:4, 2:5] in
    tile 1 where it fits, the fp32 value of the sentinel in two cells (one on a tile border, one inside; fewer where the tile has no
    room), and for n == 3 an all-NaN tile 2"""
    rng = np.random.default_rng(1000 * n + 10 * H + W)
    z = rng.normal(93, 300, size=(n, H, W)).astype(np.float32)
    mark = np.float32(3.4e38 if sentinel is None else sentinel)
    if W >= 2:
        z[0, 0, W - 1] = mark
    if n >= 2 and H >= 5 and W >= 7:
        z[1, H // 2 + 2, W // 2 + 3] = mark
    elif H >= 2:
        z[min(1, n - 1), H // 2, 0] = mark
    z[0, 0, 0] = np.nan
    z[n - 1, H - 1, W - 1] = np.nan
    if n >= 2 and H >= 4 and W >= 5:
        z[1, 1:4, 2:5] = np.nan
    if n == 3:
        z[2] = np.nan
    return z


def _expected(z, sentinel, standardise):
    from kurosiwo_amd.dataset import slope_riserun
    with np.errstate(all="ignore"):
        e = torch.from_numpy(np.stack([slope_riserun(t, sentinel) for t in z]))
    if standardise:                                   # the per-sample classes' torch expression (dataset.py: read_dem)
        e = (e - torch.as_tensor([SLOPE_MEAN], dtype=torch.float32).view(-1, 1, 1)) / torch.as_tensor([SLOPE_STD], dtype=torch.float32).view(-1, 1, 1)
    return e.numpy()


def _same_bits(got, want):
    """uint32 patterns equal; a NaN meets a NaN in the same cell (payloads are not compared) -> number of differing cells"""
    got, want = np.ascontiguousarray(got, dtype=np.float32), np.ascontiguousarray(want, dtype=np.float32)
    gn, wn = np.isnan(got), np.isnan(want)
    return int((gn != wn).sum() + (got.view(np.uint32)[~gn & ~wn] != want.view(np.uint32)[~gn & ~wn]).sum())


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_slope_kernel_equals_the_host_function_bit_for_bit(shape):
    from kurosiwo_amd.functional import dem_slope
    n, H, W = shape
    for sentinel in SENTINELS:
        z = _tiles(n, H, W, sentinel)
        dev = torch.from_numpy(z).cuda()
        for standardise in (False, True):
            want = _expected(z, sentinel, standardise)
            got = dem_slope(dev, sentinel, *((SLOPE_MEAN, [SLOPE_STD]) if standardise else (None, None)))
            assert got.shape == dev.shape and got.dtype == torch.float32 and got.data_ptr() != dev.data_ptr()
            bad = _same_bits(got.cpu().numpy(), want)
            print(f"shape {shape} sentinel {sentinel} standardise {standardise}: {bad} of {z.size} cells differ")
            assert bad == 0, (shape, sentinel, standardise)
        assert torch.equal(dev.cpu().view(torch.int32), torch.from_numpy(z).view(torch.int32))           # the input is left alone
        if n == 3:                                    # a stencil that reads the tile next in memory shows here
            whole = dem_slope(dev, sentinel)
            for t in range(n):
                alone = dem_slope(dev[t].clone(), sentinel)
                assert _same_bits(whole[t].cpu().numpy(), alone.cpu().numpy()) == 0, (shape, sentinel, t)
    # leading dimensions fold into the tile count; out= is written in place
    z = _tiles(n, H, W, -9999.0)
    dev = torch.from_numpy(z).cuda()
    out = torch.empty_like(dev).view(n, 1, H, W)
    assert dem_slope(dev.view(n, 1, H, W), -9999.0, [SLOPE_MEAN], SLOPE_STD, out=out) is out
    assert _same_bits(out.cpu().numpy().reshape(n, H, W), _expected(z, -9999.0, True)) == 0


def test_slope_kernel_argument_errors():
    from kurosiwo_amd import _lib
    from kurosiwo_amd.functional import dem_slope
    from kurosiwo_amd.runtime import stream_ptr
    lib = _lib.load()
    x = torch.zeros((2, 3, 5), dtype=torch.float32, device="cuda")
    y = torch.full_like(x, 7.0)
    nan, st = float("nan"), stream_ptr()
    assert lib.ksmi_dem_slope(x.data_ptr(), x.data_ptr(), 2, 3, 5, nan, 0.0, 1.0, 0, st) < 0
    assert lib.ksmi_dem_slope(x.data_ptr(), x.data_ptr() + 4, 2, 3, 5, nan, 0.0, 1.0, 0, st) < 0                  # a partial overlap
    assert lib.ksmi_dem_slope(x.data_ptr(), y.data_ptr(), 2, 0, 5, nan, 0.0, 1.0, 0, st) < 0
    assert lib.ksmi_dem_slope(x.data_ptr(), y.data_ptr(), 2, 3, 0, nan, 0.0, 1.0, 0, st) < 0
    assert lib.ksmi_dem_slope(x.data_ptr(), y.data_ptr(), -1, 3, 5, nan, 0.0, 1.0, 0, st) < 0
    assert lib.ksmi_dem_slope(None, y.data_ptr(), 2, 3, 5, nan, 0.0, 1.0, 0, st) < 0
    assert lib.ksmi_dem_slope(x.data_ptr(), None, 2, 3, 5, nan, 0.0, 1.0, 0, st) < 0
    assert lib.ksmi_dem_slope(x.data_ptr(), y.data_ptr(), 0, 3, 5, nan, 0.0, 1.0, 0, st) == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                     # nothing was launched
    with pytest.raises(_lib.KsmiError):
        dem_slope(x, out=x)
    with pytest.raises(_lib.KsmiError):
        dem_slope(x.cpu())
    for bad in (lambda: dem_slope(x.double()), lambda: dem_slope(x.transpose(1, 2)), lambda: dem_slope(x, mean=1.0),
                lambda: dem_slope(x, mean=[1.0, 2.0], std=[1.0, 2.0]), lambda: dem_slope(x, out=y[:1])):
        with pytest.raises(ValueError):
            bad()
    assert dem_slope(x[:0]).shape == (0, 3, 5)


@pytest.fixture(scope="module")
def archive(tmp_path_factory):
    from make_synthetic_archive import make
    root = str(tmp_path_factory.mktemp("ks"))
    os.makedirs(os.path.join(root, "pickle"))
    tr, _ = make(root, TRAIN, tiles_per_act=4, seed=1)
    te, _ = make(root, VAL + TEST, tiles_per_act=4, seed=2)
    pickle.dump(tr, gzip.open(os.path.join(root, "pickle", "train.gz"), "wb"))
    pickle.dump(te, gzip.open(os.path.join(root, "pickle", "test.gz"), "wb"))
    return root


def _slope_configs(root, **over):
    return _configs(root, dem=True, slope=True, slope_mean=[SLOPE_MEAN], slope_std=[SLOPE_STD], device="cuda", **over)


def test_batch_loader_with_slope_equals_the_per_sample_dataset(archive):
    """(the archive's DEM has a NaN gap: the slope is taken from the gap-filled tile on both sides)"""
    from kurosiwo_amd.dataset import Dataset, TileBatchLoader
    ds = Dataset("train", _slope_configs(archive))
    ref = list(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False))
    got = list(TileBatchLoader(ds, 4, device="cuda", threads=4))
    unbuffered = list(TileBatchLoader(ds, 4, device="cuda", threads=4, prefetch=0))
    assert len(ref) == len(got) == len(unbuffered) == 2
    plain = Dataset("train", _configs(archive, dem=True, device="cuda"))
    dem = next(iter(TileBatchLoader(plain, 4, device="cuda", threads=4)))[10]
    for r, g, u in zip(ref, got, unbuffered):
        for b in (g, u):
            assert len(r) == len(b) == 13
            assert b[10].is_cuda and b[10].shape == (4, 1, 224, 224) and torch.equal(b[10].cpu(), r[10])
            for pos in (2, 6, 9):
                assert b[pos].is_cuda and torch.equal(b[pos].cpu(), r[pos]), pos
            assert torch.equal(b[3].cpu(), r[3]) and torch.equal(b[11], r[11]) and torch.equal(b[12], r[12])
            for pos in (0, 1, 4, 5, 7, 8):
                assert all(torch.equal(a, c) for a, c in zip(b[pos], r[pos]))
    assert torch.isfinite(got[0][10]).all() and not torch.equal(got[0][10], dem)         # the slope, not the DEM


def test_slope_without_dem_is_refused_when_the_loader_is_built(archive, capsys):
    from kurosiwo_amd.dataset import Dataset, TileBatchLoader
    ds = Dataset("train", _configs(archive, dem=False, slope=True, device="cuda"))
    with pytest.raises(SystemExit) as e:
        TileBatchLoader(ds, 4, device="cuda")
    assert e.value.code == 2 and "DEM option must be enabled" in capsys.readouterr().out
    with pytest.raises(ValueError):
        TileBatchLoader(Dataset("train", _slope_configs(archive, uint8=True)), 4, device="cuda")


def test_slc_batch_loader_with_slope_equals_the_per_sample_dataset(tmp_path):
    """the SLC archive writes the sentinel 3.4e38 into its DEM: both paths turn the fp32 value into gaps and fill them, and neither
    recognises the double 3.4e38 in slope_riserun"""
    from make_synthetic_archive import make
    from kurosiwo_amd.dataset import SLCDataset, TileBatchLoader
    root = str(tmp_path / "slc")
    os.makedirs(os.path.join(root, "pickle"))
    tr, _ = make(root, TRAIN, tiles_per_act=4, seed=5, slc=True)
    te, _ = make(root, VAL + TEST, tiles_per_act=4, seed=6, slc=True)
    json.dump(tr, open(os.path.join(root, "pickle", "train.json"), "w"))
    json.dump(te, open(os.path.join(root, "pickle", "test.json"), "w"))
    slc = dict(slc=True, slc_root_path=root, train_json=os.path.join(root, "pickle", "train.json"), test_json=os.path.join(root, "pickle", "test.json"),
               slc_mean=[0.022367, 39.242, 81.13, 0.043526], slc_std=[1.2843, 25.6152, 58.0151, 1.2844], slc_dem_mean=82.96, slc_dem_std=153.71,
               slc_slope_mean=0.3977, slc_slope_std=0.4946)
    ds = SLCDataset("train", _slope_configs(root, **slc))
    ref = list(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False))
    got = list(TileBatchLoader(ds, 4, device="cuda", threads=4))
    assert len(ref) == len(got) == 2
    for r, g in zip(ref, got):
        assert len(r) == len(g) == 13
        assert g[10].is_cuda and torch.equal(g[10].cpu(), r[10]) and torch.isfinite(g[10]).all()
        for pos in (2, 6, 9):
            assert torch.equal(g[pos].cpu(), r[pos]), pos
        assert torch.equal(g[3].cpu(), r[3]) and torch.equal(g[11], r[11]) and torch.equal(g[12], r[12])


def test_prepare_loaders_routes_slope_to_the_batch_loader(archive, monkeypatch):
    from kurosiwo_amd.data import prepare_loaders
    from kurosiwo_amd.dataset import TileBatchLoader
    from kurosiwo_amd.snunet import SNUNet_ECAM
    from kurosiwo_amd.training.change_detection_trainer import fuse_input_pipeline
    monkeypatch.setenv("KSMI_DATA", "archive")
    monkeypatch.delenv("KSMI_FUSE_INPUT", raising=False)
    cfg = _slope_configs(archive)
    loaders = prepare_loaders(cfg)
    assert len(loaders) == 3 and all(isinstance(ld, TileBatchLoader) and not ld.raw for ld in loaders)
    model = SNUNet_ECAM(3, 3, base_channel=16).cuda()
    assert fuse_input_pipeline(model, loaders, cfg) is True
    assert all(ld.raw for ld in loaders)


def test_raw_tiles_with_slope_into_snunet_equal_the_normalised_path(archive):
    """tests/test_gpu_dataset.py:test_raw_tiles_into_snunet_equal_the_normalised_path with the slope in the terrain channel"""
    from kurosiwo_amd.dataset import Dataset, TileBatchLoader
    from kurosiwo_amd.snunet import SNUNet_ECAM
    from kurosiwo_amd.synthetic import cd_inputs
    cfg = _slope_configs(archive)
    ds = Dataset("train", cfg)
    norm = next(iter(torch.utils.data.DataLoader(ds, batch_size=4, shuffle=False)))
    raw = next(iter(TileBatchLoader(ds, 4, device="cuda", raw=True)))
    torch.manual_seed(0)
    model = SNUNet_ECAM(3, 3, base_channel=16, precision="bf16").cuda().train()

    def step(fn):
        for p in model.parameters():
            p.grad = None
        out = fn()
        torch.nn.functional.cross_entropy(out, norm[3].cuda(), ignore_index=3).backward()
        return out.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]
    (xa, xb), _ = cd_inputs(norm, ("pre_event_1", "post_event"), True)
    out0, g0 = step(lambda: model(xa.cuda(), xb.cuda()))
    model.set_input_pipeline(cfg["data_mean"] + [0.0], cfg["data_std"] + [1.0], [cfg["clamp_input"]] * 2 + [-1.0])
    out1, g1 = step(lambda: model(raw[6], raw[2], raw[10]))
    assert torch.equal(raw[10].cpu(), norm[10])
    assert torch.isnan(raw[2]).any() and torch.isfinite(out1).all()
    assert torch.equal(out0, out1)
    assert all(torch.equal(a, b) for a, b in zip(g0, g1))
