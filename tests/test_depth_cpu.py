"""Flood depth, host half: the separable nearest-feature transform of tests/depth_ref.py against its definition, hand-made tie and
shore cases that the GPU tests hold csrc/depth.hip to, the five entry points in the library and the binding, their argument checks
(which launch nothing) and the refusals of the Python wrappers.  No GPU."""
import ctypes

import numpy as np
import pytest

import depth_ref
from depth_ref import TIES, tie_map
from kurosiwo_amd.scene import EDT_FAR, MAX_EDT_SIDE, flood_depth, nearest_feature, nearest_feature_columns, nearest_feature_rows, shore

ENTRIES = ("ksmi_scene_edt_cols", "ksmi_scene_edt_rows", "ksmi_scene_select", "ksmi_scene_shore", "ksmi_scene_depth")
NAN = np.float32(np.nan)


def _random_mask(rng, H, W, density):
    if density == "one":
        m = np.zeros((H, W), np.uint8)
        m[rng.integers(H), rng.integers(W)] = 1
        return m
    return (rng.random((H, W)) < density).astype(np.uint8) * rng.integers(1, 256, size=(H, W)).astype(np.uint8)   # any non-zero value


@pytest.mark.parametrize("density", (0.0, "one", 0.02, 0.5, 1.0))
def test_the_separable_form_is_the_definition(density):
    rng = np.random.default_rng(17)
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 12), (24, 31), (23, 17)):
        m = _random_mask(rng, H, W, density)
        where = (rng.random((H, W)) < 0.6).astype(np.uint8)
        for wh in (None, where):
            d_direct, n_direct = depth_ref.nearest_feature_direct(m, wh)
            d_sep, n_sep = depth_ref.nearest_feature(m, wh)
            assert d_sep.dtype == n_sep.dtype == d_direct.dtype == np.int32
            assert np.array_equal(d_sep, d_direct) and np.array_equal(n_sep, n_direct), (H, W, density)
        d, n = depth_ref.nearest_feature_direct(m)
        if not m.any():
            assert (d == depth_ref.FAR).all() and (n == -1).all()
        else:
            on = np.flatnonzero(m)
            assert (d.ravel()[on] == 0).all() and np.array_equal(n.ravel()[on], on) and m.ravel()[n.ravel()].all()
            ys, xs = np.divmod(n, W)
            yy, xx = np.mgrid[0:H, 0:W]
            assert np.array_equal((yy - ys) ** 2 + (xx - xs) ** 2, d)


@pytest.mark.parametrize("name", sorted(TIES))
def test_a_tie_goes_to_the_smallest_index(name):
    _, (py, px), (qy, qx), want = TIES[name]
    m = tie_map(name)
    for fn in (depth_ref.nearest_feature_direct, depth_ref.nearest_feature):
        d, n = fn(m)
        assert d[py, px] == want and n[py, px] == qy * 7 + qx
    if name == "above_and_below":
        assert depth_ref.nearest_in_column(m)[:, 3].tolist() == [1, 1, 1, 1, 5, 5, 5]      # row 3: the smaller row
    assert (depth_ref.nearest_in_column(m)[:, 0] == -1).all()


def _lake():
    """a 3 x 3 lake of class 1 in a 7 x 7 field of class 0, on a DEM that falls towards the lake's middle"""
    c = np.zeros((7, 7), np.uint8)
    c[2:5, 2:5] = 1
    yy, xx = np.mgrid[0:7, 0:7]
    dem = (10.0 + (yy - 3) ** 2 + (xx - 3) ** 2).astype(np.float32)
    return c, dem


def test_shore_and_depth_of_a_small_lake():
    c, dem = _lake()
    s = depth_ref.shore(c, dem)
    want = np.zeros((7, 7), np.uint8)
    want[2:5, 2:5] = 1
    want[3, 3] = 0
    assert np.array_equal(s, want)
    depth, wse, dist2 = depth_ref.flood_depth(c, dem)
    assert depth.dtype == wse.dtype == np.float32 and dist2.dtype == np.int32
    assert depth[3, 3] == 1.0 and wse[3, 3] == 11.0 and dist2[3, 3] == 1       # the level of an edge neighbour: dem 11 against 10
    assert dist2[2, 2] == 0 and depth[2, 2] == 0.0 and wse[2, 2] == 12.0       # a shore pixel is its own nearest feature
    assert (depth[c == 0] == 0).all() and np.isnan(wse[c == 0]).all() and (dist2[c == 0] == depth_ref.FAR).all()
    assert not np.signbit(depth[~np.isnan(depth)]).any()


def test_the_centre_takes_the_level_of_its_first_edge_neighbour():
    c, dem = _lake()
    dem[2, 3], dem[3, 2], dem[3, 4], dem[4, 3] = 14.0, 15.0, 16.0, 17.0        # four shore pixels at distance 1: (2, 3) has the smallest index
    depth, wse, _ = depth_ref.flood_depth(c, dem)
    assert wse[3, 3] == 14.0 and depth[3, 3] == 4.0


def test_water_on_the_scene_border_only_has_no_shore():
    c = np.ones((4, 5), np.uint8)                                              # water everywhere: every edge is the scene border
    dem = np.arange(20, dtype=np.float32).reshape(4, 5)
    assert not depth_ref.shore(c, dem).any()
    depth, wse, dist2 = depth_ref.flood_depth(c, dem)
    assert np.isnan(depth).all() and np.isnan(wse).all() and (dist2 == depth_ref.FAR).all()
    c[1, 1] = 0                                                                # one dry pixel: its four neighbours are the shore
    s = depth_ref.shore(c, dem)
    assert s.sum() == 4 and s[0, 1] == s[1, 0] == s[1, 2] == s[2, 1] == 1
    assert np.isfinite(depth_ref.flood_depth(c, dem)[0][c == 1]).all()


def test_water_touching_invalid_only_has_no_shore():
    c = np.full((6, 5), 3, np.uint8)
    c[2:5, 1:4] = 2
    dem = np.ones((6, 5), np.float32)
    assert not depth_ref.shore(c, dem).any()
    depth, wse, _ = depth_ref.flood_depth(c, dem)
    assert np.isnan(depth).all() and np.isnan(wse).all()                       # NaN on the invalid ring and in the lake alike
    c[0, :] = 0                                                                # valid land, but not an edge neighbour of the lake
    assert not depth_ref.shore(c, dem).any()
    assert (depth_ref.flood_depth(c, dem)[0][0] == 0).all()
    c[2, 0] = 0                                                                # beside (2, 1)
    assert depth_ref.shore(c, dem).sum() == 1 and depth_ref.shore(c, dem)[2, 1] == 1


def test_a_nan_dem_on_a_shore_pixel_and_on_a_water_pixel():
    c, dem = _lake()
    dem[2, 3] = NAN                                                            # a shore pixel: no shore there, and no depth
    s = depth_ref.shore(c, dem)
    assert s[2, 3] == 0 and s.sum() == 7
    depth, wse, dist2 = depth_ref.flood_depth(c, dem)
    assert np.isnan(depth[2, 3]) and dist2[2, 3] == 1 and wse[2, 3] == 12.0    # it still has a level: that of (2, 2)
    assert wse[3, 3] == 11.0 and depth[3, 3] == 1.0                            # the centre now takes (3, 2), the next index at distance 1
    c, dem = _lake()
    dem[3, 3] = np.float32(np.inf)                                             # inside the water
    depth, wse, _ = depth_ref.flood_depth(c, dem)
    assert np.isnan(depth[3, 3]) and wse[3, 3] == 11.0 and np.isfinite(depth[c == 1]).sum() == 8
    assert np.array_equal(depth_ref.shore(c, dem), depth_ref.shore(*_lake()))  # the centre was no shore anyway


def test_another_water_set_and_another_invalid_class():
    c = np.asarray([[0, 1, 2, 2, 0],
                    [0, 1, 2, 2, 5],
                    [0, 0, 0, 5, 5]], np.uint8)
    dem = np.asarray([[9, 8, 3, 4, 9], [9, 8, 2, 1, 9], [9, 9, 9, 9, 9]], np.float32)
    s = depth_ref.shore(c, dem, water=(2,), invalid_class=5)
    assert s.tolist() == [[0, 0, 1, 1, 0], [0, 0, 1, 0, 0], [0, 0, 0, 0, 0]]   # class 1 is land here; (1, 3) touches water and invalid only
    depth, wse, _ = depth_ref.flood_depth(c, dem, water=(2,), invalid_class=5)
    assert depth[1, 3] == 3.0 and wse[1, 3] == 4.0                             # (0, 3) and (1, 2) are equally far: the smaller index
    assert np.isnan(depth[c == 5]).all() and (depth[c == 1] == 0).all()


def test_library_exports_and_binds_the_depth_entry_points():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "ksmi.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p              # int status, the stream last
        declared = hdr.split(f"int {name}(")[1].split(");")[0]
        assert len(declared.split(",")) == len(args), name
    assert lib.ksmi_abi_version() == 8


def test_argument_errors_launch_nothing_and_name_the_entry_point():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    P = 0x1000                                                                  # never dereferenced: every case fails before a launch
    big = 1 << 31

    def refused(entry, rc):
        assert rc < 0
        assert entry in lib.ksmi_last_error().decode()

    cols = lambda m=P, Hs=16, Ws=16, out=P: lib.ksmi_scene_edt_cols(m, Hs, Ws, out, None)
    for kw in (dict(m=None), dict(out=None), dict(Hs=0), dict(Ws=0), dict(Hs=-1), dict(Ws=32768), dict(Hs=32768), dict(Hs=65536, Ws=32768)):
        refused("scene_edt_cols", cols(**kw))
    rows = lambda ny=P, wh=None, Hs=16, Ws=16, d=P, n=P: lib.ksmi_scene_edt_rows(ny, wh, Hs, Ws, d, n, None)
    for kw in (dict(ny=None), dict(d=None), dict(n=None), dict(Hs=0), dict(Ws=0), dict(Ws=-3), dict(Ws=32768), dict(Hs=32768)):
        refused("scene_edt_rows", rows(**kw))
    select = lambda c=P, mask=6, HW=256, out=P: lib.ksmi_scene_select(c, mask, HW, out, None)
    for kw in (dict(c=None), dict(out=None), dict(mask=-1), dict(HW=-1), dict(HW=big)):
        refused("scene_select", select(**kw))
    assert select(HW=0) == 0
    edge = lambda c=P, dem=P, mask=6, inv=3, Hs=16, Ws=16, out=P: lib.ksmi_scene_shore(c, dem, mask, inv, Hs, Ws, out, None)
    for kw in (dict(c=None), dict(dem=None), dict(out=None), dict(mask=-1), dict(inv=256), dict(inv=-1), dict(Hs=0), dict(Ws=0),
               dict(Hs=65536, Ws=32768)):
        refused("scene_shore", edge(**kw))
    depth = lambda c=P, dem=P, n=P, mask=6, inv=3, HW=256, out=P, wse=None: lib.ksmi_scene_depth(c, dem, n, mask, inv, HW, out, wse, None)
    for kw in (dict(c=None), dict(dem=None), dict(n=None), dict(out=None), dict(mask=-1), dict(inv=256), dict(HW=-1), dict(HW=big)):
        refused("scene_depth", depth(**kw))
    assert depth(HW=0) == 0
    assert MAX_EDT_SIDE == 32767 and EDT_FAR == depth_ref.FAR == 2 ** 31 - 1 and 2 * (MAX_EDT_SIDE - 1) ** 2 < EDT_FAR


def test_the_wrappers_refuse_cpu_tensors_wrong_dtypes_and_32768_columns():
    import torch
    from kurosiwo_amd import _lib
    m = torch.zeros((8, 8), dtype=torch.uint8)
    dem = torch.zeros((8, 8), dtype=torch.float32)
    for cpu in (lambda: nearest_feature(m), lambda: nearest_feature_columns(m), lambda: nearest_feature_rows(m.int()), lambda: shore(m, dem),
                lambda: flood_depth(m, dem)):
        with pytest.raises(_lib.KsmiError):
            cpu()
    wide, tall = torch.zeros((1, 32768), dtype=torch.uint8), torch.zeros((32768, 1), dtype=torch.uint8)
    for bad in (lambda: nearest_feature(m.int()), lambda: nearest_feature(m.bool()), lambda: nearest_feature(m[:, ::2]), lambda: nearest_feature(m[0]),
                lambda: nearest_feature(m.numpy()), lambda: nearest_feature(m, where=m.int()), lambda: nearest_feature(m, where=m[:4]),
                lambda: nearest_feature(wide), lambda: nearest_feature(tall), lambda: nearest_feature_columns(wide),
                lambda: nearest_feature_rows(wide.int()), lambda: nearest_feature_rows(m), lambda: nearest_feature_rows(m.int(), where=m.int()),
                lambda: shore(m, dem.double()), lambda: shore(m, dem[:4]), lambda: shore(m.int(), dem), lambda: shore(m, dem, water=(63,)),
                lambda: shore(m, dem, invalid_class=256), lambda: flood_depth(m, dem.half()), lambda: flood_depth(m, dem, water=(-1,)),
                lambda: flood_depth(wide, wide.float()), lambda: flood_depth(m, dem, invalid_class=-1)):
        with pytest.raises(ValueError):
            bad()
