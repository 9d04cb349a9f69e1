"""Flood depth on the device (csrc/depth.hip, kurosiwo_amd/scene.py: nearest_feature_columns, nearest_feature_rows, nearest_feature,
shore, flood_depth; predict.py --depth_out) against tests/depth_ref.py, equal bit for bit: the column pass and the row pass each
against its half of the reference and the transform end to end, on shapes off every power of two, wave and tile edge and on rows and
columns longer than anything the kernels stage; ties at the tile corners; `where`; two runs give equal bits; the depth of a basin, of
lakes cut by the border or walled in by invalid pixels, with NaN in the DEM; predict.py --mmu --depth_out --report end to end."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import depth_ref
from depth_ref import TIES, tie_map
from kurosiwo_amd.scene import (EDT_COLUMN_TILE, EDT_FAR, EDT_ROW_WINDOW, flood_depth, nearest_feature, nearest_feature_columns, nearest_feature_rows,
                                select_classes, shore)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 130), (130, 1), (67, 133), (150, 300))
CONTENTS = ("none", "corner0", "corner1", "corner2", "corner3", "all", "checkerboard", "random0.1", "random30")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _mask(shape, content):
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    m = np.zeros((H, W), np.uint8)
    if content.startswith("corner"):
        m[{"0": 0, "1": 0, "2": H - 1, "3": H - 1}[content[-1]], {"0": 0, "1": W - 1, "2": 0, "3": W - 1}[content[-1]]] = 200
    elif content == "all":
        m[:] = 1
    elif content == "checkerboard":
        yy, xx = np.mgrid[0:H, 0:W]
        m = ((yy + xx) & 1).astype(np.uint8)
    elif content.startswith("random"):
        m = (rng.random((H, W)) < float(content[6:]) / 100).astype(np.uint8)
    return m


@functools.lru_cache(maxsize=None)
def _want(shape, content):
    """(near_y, dist2, nearest) of a case, computed once; left unchanged"""
    m = _mask(shape, content)
    near_y = depth_ref.nearest_in_column(m)
    return (near_y,) + depth_ref.nearest_from_columns(near_y)


def _differ(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    return int((got != want).sum())


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_columns_rows_and_the_transform(shape, content):
    m = _mask(shape, content)
    near_y, dist2, nearest = _want(shape, content)
    d = _dev(m)
    got_y = nearest_feature_columns(d)
    got_d, got_n = nearest_feature_rows(_dev(near_y))               # the row pass on the reference's columns: its own half
    end_d, end_n = nearest_feature(d)
    assert all(t.is_cuda and t.dtype == torch.int32 and t.shape == d.shape for t in (got_y, got_d, got_n, end_d, end_n))
    bad = [_differ(_bits(g), w) for g, w in ((got_y, near_y), (got_d, dist2), (got_n, nearest), (end_d, dist2), (end_n, nearest))]
    print(f"{shape} {content}: {int((m != 0).sum())} features, largest dist2 {int(dist2.max())}; cells that differ "
          f"(near_y, rows dist2, rows nearest, dist2, nearest): {bad}")
    assert not any(bad)
    assert torch.equal(d.cpu(), torch.from_numpy(m))                # the input is left alone
    again_d, again_n = nearest_feature(d)                           # two runs, equal bits
    assert torch.equal(again_d, end_d) and torch.equal(again_n, end_n)
    if content == "none":
        assert (dist2 == EDT_FAR).all() and (nearest == -1).all() and (near_y == -1).all()
    if content == "all":
        assert not dist2.any() and np.array_equal(nearest.ravel(), np.arange(m.size))


def test_the_separable_reference_is_the_definition_on_the_shapes_used_here():
    for shape, content in (((67, 133), "random0.1"), ((67, 133), "random30"), ((67, 133), "corner3"), ((1, 130), "random30"), ((130, 1), "random30")):
        d, n = depth_ref.nearest_feature_direct(_mask(shape, content))
        assert np.array_equal(d, _want(shape, content)[1]) and np.array_equal(n, _want(shape, content)[2])


def test_the_row_pass_on_columns_that_no_mask_gave():
    """any near_y with values -1 .. Hs - 1 has a lexicographic minimum: random rows, a third of the columns empty"""
    H, W = 67, 133
    rng = np.random.default_rng(9)
    near_y = np.where(rng.random((H, W)) < 0.33, -1, rng.integers(0, H, size=(H, W))).astype(np.int32)
    want_d, want_n = depth_ref.nearest_from_columns(near_y)
    got_d, got_n = nearest_feature_rows(_dev(near_y))
    assert _differ(_bits(got_d), want_d) == 0 and _differ(_bits(got_n), want_n) == 0


@pytest.mark.parametrize("y0", (13, 60, 61))
@pytest.mark.parametrize("x0", (60, 61, 252, 253))
@pytest.mark.parametrize("name", sorted(TIES))
def test_ties_at_the_tile_corners(name, x0, y0):
    """the tied pixel in the last column of a workgroup of either pass and in the first column of the next; in the last row of a
    y-tile of the column pass and in the first row of the next, so that one of the tied features comes in as the carry"""
    tile = EDT_ROW_WINDOW[0]
    assert tile == 256 and x0 + 3 in (63, 64, tile - 1, tile) and EDT_COLUMN_TILE == 64 and y0 + 3 in (16, 63, 64)
    _, (py, px), (qy, qx), want = TIES[name]
    H, W = 80, 300
    m = tie_map(name, H, W, y0, x0)
    got_d, got_n = (_bits(t) for t in nearest_feature(_dev(m)))
    ref_d, ref_n = depth_ref.nearest_feature_direct(m)
    assert got_d[y0 + py, x0 + px] == want and got_n[y0 + py, x0 + px] == (y0 + qy) * W + x0 + qx
    assert np.array_equal(got_d, ref_d) and np.array_equal(got_n, ref_n)
    assert np.array_equal(_bits(nearest_feature_columns(_dev(m))), depth_ref.nearest_in_column(m))


@pytest.mark.parametrize("shape,feature", (((3, 5000), (2, 4999)), ((3, 5000), (1, 0)), ((5000, 3), (4999, 2)), ((5000, 3), (0, 1))),
                         ids=("3x5000far", "3x5000near", "5000x3far", "5000x3near"))
def test_a_single_feature_at_the_far_end_of_a_long_row_and_a_long_column(shape, feature):
    """a row longer than the staged window, the longest search there is, and a column sweep of 5000 rows"""
    H, W = shape
    assert max(H, W) > EDT_ROW_WINDOW[0] + 2 * EDT_ROW_WINDOW[1]
    m = np.zeros(shape, np.uint8)
    m[feature] = 7
    yy, xx = np.mgrid[0:H, 0:W]
    want_d = ((yy - feature[0]) ** 2 + (xx - feature[1]) ** 2).astype(np.int32)
    ref_d, ref_n = depth_ref.nearest_feature_direct(m)
    assert np.array_equal(ref_d, want_d) and (ref_n == feature[0] * W + feature[1]).all()
    d = _dev(m)
    near_y = _bits(nearest_feature_columns(d))
    assert (near_y[:, feature[1]] == feature[0]).all() and (np.delete(near_y, feature[1], axis=1) == -1).all()
    got_d, got_n = (_bits(t) for t in nearest_feature(d))
    print(f"{shape} feature {feature}: largest dist2 {int(got_d.max())}; cells that differ: {_differ(got_d, ref_d)}, {_differ(got_n, ref_n)}")
    assert np.array_equal(got_d, ref_d) and np.array_equal(got_n, ref_n)


def test_a_column_of_more_rows_than_128_tiles_of_64():
    """past 8192 rows the y-tiles of the column pass grow: 8300 rows are 128 tiles of 65; sparse features, so carries cross many tiles"""
    H, W = 128 * EDT_COLUMN_TILE + 108, 5
    rng = np.random.default_rng(8300)
    m = (rng.random((H, W)) < 0.002).astype(np.uint8)
    m[:, 3] = 0
    m[[0, H - 1, 4160, 4225], [0, 1, 2, 2]] = 1
    assert 3 <= m[:, 0].sum() and not m[:, 3].any()
    near_y = depth_ref.nearest_in_column(m)
    want_d, want_n = depth_ref.nearest_from_columns(near_y)
    d = _dev(m)
    assert _differ(_bits(nearest_feature_columns(d)), near_y) == 0
    got_d, got_n = nearest_feature(d)
    assert _differ(_bits(got_d), want_d) == 0 and _differ(_bits(got_n), want_n) == 0


@pytest.mark.parametrize("shape,content", (((67, 133), "random30"), ((150, 300), "random0.1"), ((150, 300), "corner2"), ((1, 130), "random30")))
def test_where_skips_pixels_and_changes_no_other(shape, content):
    m = _mask(shape, content)
    _, dist2, nearest = _want(shape, content)
    rng = np.random.default_rng(5)
    blocks = np.kron((rng.random((-(-shape[0] // 8), -(-shape[1] // 64))) < 0.5).astype(np.uint8), np.ones((8, 64), np.uint8))[:shape[0], :shape[1]]
    for where in ((rng.random(shape) < 0.5).astype(np.uint8) * 9, blocks.astype(np.uint8), np.zeros(shape, np.uint8), np.ones(shape, np.uint8)):
        got_d, got_n = (_bits(t) for t in nearest_feature(_dev(m), where=_dev(where)))
        on = where != 0
        assert (got_d[~on] == EDT_FAR).all() and (got_n[~on] == -1).all()
        assert np.array_equal(got_d[on], dist2[on]) and np.array_equal(got_n[on], nearest[on])
        ref_d, ref_n = depth_ref.nearest_from_columns(_want(shape, content)[0], where)
        assert np.array_equal(got_d, ref_d) and np.array_equal(got_n, ref_n)


def test_an_empty_scene_gives_empty_tensors():
    for shape in ((0, 5), (5, 0)):
        d, n = nearest_feature(torch.empty(shape, dtype=torch.uint8, device="cuda"))
        assert d.shape == n.shape == shape and d.dtype == n.dtype == torch.int32
        assert flood_depth(torch.empty(shape, dtype=torch.uint8, device="cuda"), torch.empty(shape, device="cuda")).shape == shape


def test_wrappers_refuse_bad_shapes_and_dtypes_on_the_device():
    m, dem = torch.zeros((4, 4), dtype=torch.uint8, device="cuda"), torch.zeros((4, 4), device="cuda")
    for bad in (lambda: nearest_feature(m.int()), lambda: nearest_feature(m[:, ::2]), lambda: nearest_feature(m[0]),
                lambda: nearest_feature(m, where=m.int()), lambda: nearest_feature(m, where=m[:2]), lambda: nearest_feature(m, where=m.cpu()),
                lambda: nearest_feature(torch.zeros((1, 32768), dtype=torch.uint8, device="cuda")), lambda: nearest_feature_rows(m),
                lambda: flood_depth(m, dem.double()), lambda: flood_depth(m, dem[:2]), lambda: flood_depth(m, dem, water=(63,)),
                lambda: shore(m, dem.cpu()), lambda: select_classes(m.int())):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------- flood depth
def _basin(H=96, W=120, cy=47.3, cx=58.6, level=9.0):
    """a paraboloid basin and the water below `level`: class 2 in its deep half, class 1 around it"""
    yy, xx = np.mgrid[0:H, 0:W]
    dem = (((yy - cy) ** 2 + 0.6 * (xx - cx) ** 2) / 40.0 + 0.37 * np.sin(yy * 0.9) * np.cos(xx * 0.7)).astype(np.float32)
    classes = np.where(dem < level, np.where(dem < level / 2, 2, 1), 0).astype(np.uint8)
    return classes, dem


def _check_depth(classes, dem, **kw):
    """depth, wse and dist2 of the device against the reference, as bits; -> the three reference arrays"""
    want = depth_ref.flood_depth(classes, dem, **kw)
    c, z = _dev(classes), _dev(dem)
    got = flood_depth(c, z, return_wse=True, distance=True, **kw)
    assert [t.dtype for t in got] == [torch.float32, torch.float32, torch.int32] and all(t.is_cuda and t.shape == c.shape for t in got)
    bad = [int((_bits(g).view(np.uint32) != w.view(np.uint32)).sum()) for g, w in zip(got, want)]
    depth = want[0]
    print(f"{classes.shape}: water {int(depth_ref.in_set(classes, kw.get('water', (1, 2))).sum())}, shore "
          f"{int(depth_ref.shore(classes, dem, **kw).sum())}, finite depth > 0 at {int((depth > 0).sum())}, deepest "
          f"{float(np.nanmax(depth)) if np.isfinite(depth).any() else None}; cells that differ (depth, wse, dist2): {bad}")
    assert not any(bad)
    assert not (_bits(got[0]).view(np.uint32) == 0x80000000).any()          # the sign bit of every zero is clear
    alone = flood_depth(c, z, **kw)                                          # the other return forms; two runs, equal bits
    assert torch.is_tensor(alone) and torch.equal(alone.view(torch.int32), got[0].view(torch.int32))
    pair = flood_depth(c, z, return_wse=True, **kw)
    assert len(pair) == 2 and torch.equal(pair[1].view(torch.int32), got[1].view(torch.int32))
    assert np.array_equal(_bits(shore(c, z, **kw)), depth_ref.shore(classes, dem, **kw))
    assert torch.equal(c.cpu(), torch.from_numpy(classes)) and torch.equal(z.cpu().view(torch.int32), torch.from_numpy(dem).view(torch.int32))
    return want


def test_the_depth_of_a_basin():
    classes, dem = _basin()
    depth, wse, dist2 = _check_depth(classes, dem)
    wet = classes != 0
    assert wet.sum() > 1000 and (classes == 2).sum() > 300 and np.isfinite(depth).all()
    assert (depth[~wet] == 0).all() and np.isnan(wse[~wet]).all() and (depth[wet] > 0).sum() > wet.sum() // 2
    assert dist2[wet].max() > 100                                            # the middle is more than ten pixels from the shore


def test_a_lake_cut_by_the_scene_border():
    classes, dem = _basin(cy=3.0, cx=110.0)                                  # the basin's middle near the top right corner
    assert classes[0, -1] != 0 and classes[0].any() and classes[:, -1].any() and not classes[-1].any()
    depth, wse, _ = _check_depth(classes, dem)
    s = depth_ref.shore(classes, dem)
    assert classes[0, -2] and classes[1, -1] and s[0, -1] == 0 and s.any()     # the corner pixel: water inside, the border outside
    assert np.isfinite(depth[classes != 0]).all()


def test_a_lake_walled_in_by_invalid_pixels_is_all_nan():
    classes, dem = _basin()
    wet = classes != 0
    ring = np.zeros_like(wet)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ring |= np.roll(wet, (dy, dx), axis=(0, 1))
    classes[ring & ~wet] = 3
    depth, wse, dist2 = _check_depth(classes, dem)
    assert np.isnan(depth[wet]).all() and np.isnan(depth[classes == 3]).all() and (depth[classes == 0] == 0).all()
    assert np.isnan(wse).all() and (dist2 == EDT_FAR).all()


def test_no_water_at_all():
    classes, dem = _basin(level=-5.0)
    assert not classes.any()
    classes[4, 5] = 3
    depth, wse, dist2 = _check_depth(classes, dem)
    assert np.isnan(depth[4, 5]) and np.isnan(depth).sum() == 1 and not depth[np.isfinite(depth)].any()
    assert np.isnan(wse).all() and (dist2 == EDT_FAR).all()


def test_nan_in_the_dem_on_the_shore_and_inside_the_water():
    classes, dem = _basin()
    s = np.argwhere(depth_ref.shore(classes, dem))
    deep = np.argwhere(classes == 2)
    rng = np.random.default_rng(3)
    on_shore, inside = s[rng.choice(len(s), 25, replace=False)], deep[rng.choice(len(deep), 25, replace=False)]
    dem[on_shore[:, 0], on_shore[:, 1]] = np.nan
    dem[inside[:20, 0], inside[:20, 1]] = np.nan
    dem[inside[20:, 0], inside[20:, 1]] = np.inf
    dem[0, 0] = -np.inf                                                      # dry land: depth 0 whatever the DEM says
    depth, wse, dist2 = _check_depth(classes, dem)
    assert not depth_ref.shore(classes, dem)[on_shore[:, 0], on_shore[:, 1]].any()
    assert np.isnan(depth[on_shore[:, 0], on_shore[:, 1]]).all() and np.isnan(depth[inside[:, 0], inside[:, 1]]).all()
    assert np.isfinite(wse[inside[:, 0], inside[:, 1]]).all() and (dist2[on_shore[:, 0], on_shore[:, 1]] > 0).all() and depth[0, 0] == 0


def test_another_water_set_and_another_invalid_class():
    classes, dem = _basin()
    classes[10:14, 20:90] = 5
    for kw in (dict(water=(2,)), dict(water=(2,), invalid_class=5), dict(water=(1,), invalid_class=0), dict(water=(0, 5), invalid_class=2),
               dict(water=())):
        depth, _, _ = _check_depth(classes, dem, **kw)
        assert np.isnan(depth[classes == kw.get("invalid_class", 3)]).all()


# ---------------------------------------------------------------------------------------------------- predict.py
def _tiny_scene(tmp_path):
    """a tiny SNUNet checkpoint and georeferenced rasters, as the end-to-end tests of tests/test_gpu_sieve.py and
    tests/test_gpu_polygon.py build them, and a raw DEM in metres with a NaN and a cell at its nodata tag"""
    from oracle import snunet_ref as R
    from oracle.seeded import seeded_fill_
    from kurosiwo_amd import geotiff
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.snunet import SNUNet_ECAM
    bc = load_json5(os.path.join(ROOT, "configs", "method", "snunet", "snunet.json"))["base_channel"]
    rng = np.random.default_rng(81)
    pre, post = (rng.normal(0.06, 0.08, size=(2, 80, 72)).astype(np.float32) for _ in range(2))
    post[0, 5, 7] = np.nan
    post[1, 50, 60] = pre[0, 33, 1] = -9999.0
    geo = dict(pixel_scale=(10.0, 10.0), origin=(500000.0, 4100000.0))
    geotiff.write(str(tmp_path / "post_vv.tif"), post[0], nodata=-9999.0, **geo)
    geotiff.write(str(tmp_path / "post_vh.tif"), post[1], nodata=-9999.0, **geo)
    geotiff.write(str(tmp_path / "pre.tif"), pre, nodata=-9999.0, compression="deflate", pixel_scale=(20.0, 20.0), origin=(1.0, 2.0))
    yy, xx = np.mgrid[0:80, 0:72]
    dem = (120.0 + 3.0 * np.sin(yy / 7.0) * np.cos(xx / 5.0) + rng.normal(0.0, 0.4, size=(80, 72))).astype(np.float32)
    dem[40, 30] = np.nan
    dem[12, 50] = dem[60, 9] = -32768.0
    geotiff.write(str(tmp_path / "dem.tif"), dem, nodata=-32768.0, **geo)
    model = SNUNet_ECAM(2, 3, base_channel=bc, precision="fp32")
    model.load_state_dict(seeded_fill_(R.new_state_dict(2, 3, bc)))
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, str(tmp_path / "best.pt"))
    dem[dem == np.float32(-32768.0)] = np.nan
    return dem, [sys.executable, os.path.join(ROOT, "predict.py"), "--task", "cd", "--method", "snunet", "--checkpoint", str(tmp_path / "best.pt"),
                 "--post", str(tmp_path / "post_vv.tif"), str(tmp_path / "post_vh.tif"), "--pre1", str(tmp_path / "pre.tif"),
                 "--window", "32", "--stride", "16", "--batch_size", "5", "--precision", "fp32"]


def test_predict_script_with_mmu_depth_and_report(tmp_path):
    from kurosiwo_amd import geotiff
    dem, cmd = _tiny_scene(tmp_path)
    refused = subprocess.run(cmd + ["--out", str(tmp_path / "none.tif"), "--depth_out", str(tmp_path / "d.tif")], cwd=str(tmp_path),
                             capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--depth_out needs a DEM" in refused.stderr and not os.path.exists(str(tmp_path / "none.tif"))
    run = subprocess.run(cmd + ["--out", str(tmp_path / "flood.tif"), "--mmu", "6", "--depth_out", str(tmp_path / "d.tif"), "--depth_dem",
                                str(tmp_path / "dem.tif"), "--report", "r.json"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    classes, meta = geotiff.read(str(tmp_path / "flood.tif"))
    got, dmeta = geotiff.read(str(tmp_path / "d.tif"))
    assert got.dtype == np.float32 and got.shape == classes.shape == (80, 72)
    assert dmeta["pixel_scale"] == (10.0, 10.0) and dmeta["origin"] == (500000.0, 4100000.0) and np.isnan(dmeta["nodata"])
    want = flood_depth(_dev(classes), _dev(dem)).cpu().numpy()
    ref = depth_ref.flood_depth(classes, dem)[0]
    wet = (classes == 1) | (classes == 2)
    deep = got[wet & np.isfinite(got)].astype(np.float64)
    print(f"predict.py --mmu 6 --depth_out: classes {np.bincount(classes.ravel(), minlength=4).tolist()}, water {int(wet.sum())}, with depth "
          f"{deep.size}, deepest {deep.max() if deep.size else None}; cells that differ from flood_depth "
          f"{int((got.view(np.uint32) != want.view(np.uint32)).sum())}, from the reference {int((got.view(np.uint32) != ref.view(np.uint32)).sum())}")
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert wet.sum() > 0 and deep.size > 0 and np.isnan(got[classes == 3]).all() and f"wrote {tmp_path / 'd.tif'}" in run.stdout
    report = json.load(open(str(tmp_path / "r.json")))
    assert report["depth"] == {"water_pixels": int(wet.sum()), "with_depth": int(deep.size), "max": float(deep.max()), "mean": float(deep.mean()),
                               "volume": float(deep.sum()) * 100.0}
    counts = np.bincount(classes.ravel(), minlength=4).tolist()                 # the old keys, as tests/test_gpu_sieve.py reads them
    assert list(report) == ["pixel_counts", "pixel_area", "class_area", "mmu", "connectivity", "passes", "components_removed", "depth"]
    assert report["pixel_counts"] == counts and report["pixel_area"] == 100.0 and report["class_area"] == [100.0 * c for c in counts]
    assert (report["mmu"], report["connectivity"], report["passes"]) == (6, 4, 1) and report["components_removed"] >= 1
