"""Percentiles per zone, host half: the vectorised reference of tests/quantile_ref.py against its per-zone loop, the integer position
rule against np.percentile, the key order inside a zone, the percent to basis-point conversion and the column names, the host
combination of lower and higher, the entry points in the library and the binding, their argument checks (which launch nothing) and
the refusals of the Python wrappers.  No GPU."""
import ctypes

import numpy as np
import pytest

import quantile_ref
import zonal_ref
from kurosiwo_amd.scene import (MAX_PERCENTILES, MAX_ZONAL_BANDS, QUANTILE_METHODS, ZonalQuantiles, basis_points, component_quantiles,
                                percentile_name, quantile_values, zonal_quantiles, zonal_sorted)

ENTRIES = ("ksmi_scene_quantile_zones", "ksmi_scene_quantile_keys", "ksmi_scene_quantile_sort", "ksmi_scene_quantile_select",
           "ksmi_scene_quantile_segments")
QUERIES = ("ksmi_scene_quantile_passes", "ksmi_scene_quantile_scratch")
PERCENTS = (0, 0.01, 25, 50, 97.5, 99.99, 100)
F = np.float32


def _random_case(rng, H, W, B, zones_kind):
    HW = H * W
    if zones_kind == "few":
        zones = rng.choice(np.asarray([0, 3, HW - 1, HW // 2], np.int64), size=(H, W))
    elif zones_kind == "own":
        zones = np.arange(HW, dtype=np.int64).reshape(H, W)
    else:
        zones = rng.integers(0, HW, size=(H, W))
    zones = zones.astype(np.int32)
    skip = rng.random((H, W))
    zones[skip < 0.1] = -1 - rng.integers(0, 5, size=int((skip < 0.1).sum()))
    zones[(skip >= 0.1) & (skip < 0.2)] = HW + rng.integers(0, 5, size=int(((skip >= 0.1) & (skip < 0.2)).sum()))
    values = (rng.normal(0.0, 3.0, size=(B, H, W)) * 10.0 ** rng.integers(-6, 6, size=(B, H, W))).astype(F)
    levels = np.asarray([-2.5, -0.0, 0.0, 1.0, 7.25], F)
    values = np.where(rng.random((B, H, W)) < 0.4, levels[rng.integers(0, 5, size=(B, H, W))], values).astype(F)      # heavy ties
    odd = rng.random((B, H, W))
    values[odd < 0.05] = np.nan
    values[(odd >= 0.05) & (odd < 0.08)] = np.inf
    values[(odd >= 0.08) & (odd < 0.11)] = -np.inf
    values[(odd >= 0.11) & (odd < 0.14)] = F(3e38)
    values[(odd >= 0.14) & (odd < 0.17)] = F(-3e38)
    where = (rng.random((H, W)) < 0.7).astype(np.uint8) * 5
    return zones, np.ascontiguousarray(values), where


@pytest.mark.parametrize("zones_kind", ("few", "own", "any"))
def test_the_vectorised_reference_is_the_loop(zones_kind):
    rng = np.random.default_rng(31)
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 12), (13, 11)):
        for B in (1, 3):
            zones, values, where = _random_case(rng, H, W, B, zones_kind)
            for wh in (None, where):
                a = quantile_ref.zonal_quantiles(zones, values, PERCENTS, wh)
                b = quantile_ref.zonal_quantiles_loop(zones, values, PERCENTS, wh)
                assert quantile_ref.same(a, b) == [], (H, W, B, quantile_ref.same(a, b))
                assert a.zone.dtype == a.valid.dtype == np.int32 and a.lower.dtype == a.higher.dtype == F
                N = a.zone.size
                assert a.valid.shape == (B, N) and a.lower.shape == a.higher.shape == (B, len(PERCENTS), N)
                assert a.percentiles == (0, 1, 2500, 5000, 9750, 9999, 10000)
                stats = zonal_ref.zonal_stats(zones, values, wh)
                assert np.array_equal(a.zone, stats.zone) and np.array_equal(a.valid, stats.valid)
                some = a.valid > 0                                               # percentile 0 and 100 are the key-ordered extremes
                assert a.lower[:, 0][some].tobytes() == stats.vmin[some].tobytes() and a.higher[:, -1][some].tobytes() == stats.vmax[some].tobytes()
                assert np.isnan(a.lower[:, 0][~some]).all() and np.isnan(a.higher[:, 3][~some]).all()
                for band in range(B):
                    s, t = quantile_ref.zonal_sorted(zones, values[band], wh), quantile_ref.zonal_sorted_loop(zones, values[band], wh)
                    assert all(u.dtype == v.dtype and u.tobytes() == v.tobytes() for u, v in zip(s, t))
                    assert np.array_equal(np.diff(s[1]), a.valid[band]) and s[2].size == s[1][-1]
    one = quantile_ref.zonal_quantiles(np.zeros((3, 4), np.int32), np.arange(12, dtype=F).reshape(3, 4), (0, 50, 90, 100))      # by hand
    assert one.zone.tolist() == [0] and one.valid.tolist() == [[12]]
    assert one.lower[0, :, 0].tolist() == [0.0, 5.0, 9.0, 11.0] and one.higher[0, :, 0].tolist() == [0.0, 6.0, 10.0, 11.0]
    assert quantile_ref.values(one)[0, :, 0].tolist() == [0.0, 5.5, 9.0 + 0.9, 11.0]
    empty = quantile_ref.zonal_quantiles(np.full((3, 4), -1, np.int32), np.zeros((2, 3, 4), F), (50, 90))
    assert empty.zone.shape == (0,) and empty.valid.shape == (2, 0) and empty.lower.shape == (2, 2, 0)


def test_the_integer_position_is_numpy_percentile():
    """lower and higher against np.percentile(method="lower" / "higher") at the percents whose position numpy computes exactly;
    linear against np.percentile of the float64 values within 1e-12 * max(1, |x|)"""
    rng = np.random.default_rng(7)
    percents = (0, 25, 50, 75, 100)
    for n in list(range(1, 400)) + [1000, 2047, 2048, 2049, 65537, 100001]:
        v = (rng.normal(0.0, 50.0, size=n)).astype(F)
        if n > 3:
            v[rng.integers(0, n, size=n // 3)] = v[0]                            # ties
        q = quantile_ref.zonal_quantiles(np.zeros((1, n), np.int32), v.reshape(1, n), percents)
        assert q.valid.tolist() == [[n]]
        for j, p in enumerate(percents):
            assert q.lower[0, j, 0] == np.percentile(v, p, method="lower") and q.higher[0, j, 0] == np.percentile(v, p, method="higher"), (n, p)
        got = quantile_values(ZonalQuantiles(*q), "linear")[0, :, 0]
        want = np.percentile(v.astype(np.float64), percents)
        assert (np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))).all(), (n, got, want)
        for method in QUANTILE_METHODS:
            assert quantile_values(ZonalQuantiles(*q), method).tobytes() == quantile_ref.values(q, method).tobytes()
    with pytest.raises(ValueError):
        quantile_values(ZonalQuantiles(*q), "median")


def test_the_methods_combine_lower_and_higher_in_float64():
    v = np.asarray([[1.0, 2.0, 4.0, 8.0]], F)
    q = ZonalQuantiles(*quantile_ref.zonal_quantiles(np.zeros((1, 4), np.int32), v, (0, 10, 50, 90, 100)))
    # positions c * 3 / 10000: 0, 0.3, 1.5, 2.7, 3
    assert q.lower[0, :, 0].tolist() == [1.0, 1.0, 2.0, 4.0, 8.0] and q.higher[0, :, 0].tolist() == [1.0, 2.0, 4.0, 8.0, 8.0]
    assert quantile_values(q)[0, :, 0].tolist() == [1.0, 1.0 + 0.3, 2.0 + 2.0 * 0.5, 4.0 + 4.0 * 0.7, 8.0]
    assert quantile_values(q, "midpoint")[0, :, 0].tolist() == [1.0, 1.5, 3.0, 6.0, 8.0]
    assert quantile_values(q, "nearest")[0, :, 0].tolist() == [1.0, 1.0, 2.0, 8.0, 8.0]          # a half goes down: 2 * g <= 10000
    assert quantile_values(q, "lower").dtype == np.float64 and quantile_values(q, "higher")[0, :, 0].tolist() == [1.0, 2.0, 4.0, 8.0, 8.0]
    none = ZonalQuantiles(*quantile_ref.zonal_quantiles(np.zeros((1, 2), np.int32), np.asarray([[np.nan, np.inf]], F), (50,)))
    assert none.valid.tolist() == [[0]] and none.lower.view(np.uint32).tolist() == [[[0x7FC00000]]] == none.higher.view(np.uint32).tolist()
    assert all(np.isnan(quantile_values(none, m)).all() for m in QUANTILE_METHODS)


def test_the_key_order_inside_a_zone():
    flt_max, tiny = np.finfo(F).max, F(1e-45)
    v = np.asarray([[0.0, np.inf, -flt_max, np.nan, -0.0, tiny, flt_max, -np.inf, -tiny, 0.0, -0.0]], F)
    for zone, offsets, flat in (quantile_ref.zonal_sorted(np.zeros((1, 11), np.int32), v), quantile_ref.zonal_sorted_loop(np.zeros((1, 11), np.int32), v)):
        want = np.asarray([-flt_max, -tiny, -0.0, -0.0, 0.0, 0.0, tiny, flt_max], F)
        assert zone.tolist() == [0] and offsets.tolist() == [0, 8] and flat.tobytes() == want.tobytes()      # the zeros in order, as bits
    q = quantile_ref.zonal_quantiles(np.zeros((1, 11), np.int32), v, (0, 50, 100))
    assert q.valid.tolist() == [[8]] and q.lower[0, :, 0].tolist() == [-flt_max, 0.0, flt_max]
    assert np.signbit(q.lower[0, 1, 0]) and not np.signbit(q.higher[0, 1, 0])                                # position 3.5: -0.0 then +0.0
    assert quantile_ref.same(q, quantile_ref.zonal_quantiles_loop(np.zeros((1, 11), np.int32), v, (0, 50, 100))) == []


def test_percents_become_basis_points_or_are_refused():
    assert basis_points((50,)) == (5000,) and basis_points(50) == (5000,) and basis_points([0, 100]) == (0, 10000)
    assert basis_points(PERCENTS) == (0, 1, 2500, 5000, 9750, 9999, 10000) == quantile_ref.basis_points(PERCENTS)
    assert basis_points((np.float32(97.5), np.int64(3), 33.33, 0.1 + 0.2)) == (9750, 300, 3333, 30)        # 0.30000000000000004
    for c in range(0, 10001):
        assert basis_points((c / 100,)) == (c,)
    for bad in ((), [], (50.005,), (33.333,), (1e-3,), (-0.01,), (100.01,), (-1,), (101,), (float("nan"),), (float("inf"),), ("50",), (None,),
                (True,), tuple(range(MAX_PERCENTILES + 1)), None, "50", ((50,),)):
        with pytest.raises(ValueError, match="zonal_quantiles"):
            basis_points(bad)
    assert len(basis_points(tuple(range(MAX_PERCENTILES)))) == MAX_PERCENTILES == 16
    with pytest.raises(ValueError, match="somewhere"):
        basis_points((50.005,), "somewhere")


def test_the_column_names():
    assert [percentile_name(c) for c in (0, 1, 10, 100, 2500, 5000, 9000, 9750, 9999, 10000)] == [
        "p0", "p0_01", "p0_1", "p1", "p25", "p50", "p90", "p97_5", "p99_99", "p100"]
    assert len({percentile_name(c) for c in range(10001)}) == 10001                # one name per basis point
    for bad in (-1, 10001):
        with pytest.raises(ValueError):
            percentile_name(bad)
    import predict
    assert predict.percentile_columns((5000, 9750)) == ("depth_p50", "depth_p97_5")


def test_library_exports_and_binds_the_quantile_entry_points():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "ksmi.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and args[-1] is ctypes.c_void_p              # int status, the stream last
        declared = hdr.split(f"int {name}(")[1].split(");")[0]
        assert len(declared.split(",")) == len(args), name
        assert "the reference has no counterpart" in hdr.split(f"int {name}(")[0].rsplit("/*", 1)[1]
    for name in QUERIES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES and f" {name}(int64_t" in hdr
        assert f"{name}: the reference has no counterpart" in hdr
    assert lib.ksmi_abi_version() == 8


def test_the_pass_count_and_the_scratch_follow_the_sizes():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    passes = {0: 0, 1: 4, 2: 5, 256: 5, 257: 6, 45000: 6, 65536: 6, 65537: 7, 2 ** 24: 7, 2 ** 24 + 1: 8, 4100 * 4100: 8, 2 ** 31 - 1: 8}
    assert {N: lib.ksmi_scene_quantile_passes(N) for N in passes} == passes
    assert lib.ksmi_scene_quantile_passes(-1) == -1 and lib.ksmi_scene_quantile_passes(2 ** 31) == -1
    from kurosiwo_amd.scene import QUANTILE_TILE
    for HW, tiles in ((0, None), (1, 1), (QUANTILE_TILE, 1), (QUANTILE_TILE + 1, 2), (4480 * 4480, 4900), (2 ** 31 - 1, 2 ** 19)):
        assert lib.ksmi_scene_quantile_scratch(HW) == (0 if tiles is None else 256 * tiles + 256)
    assert lib.ksmi_scene_quantile_scratch(-1) == -1 and lib.ksmi_scene_quantile_scratch(2 ** 31) == -1


def test_argument_errors_launch_nothing_and_name_the_entry_point():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    P = 0x1000                                                                  # never dereferenced: every case fails before a launch
    big = 1 << 31

    def refused(entry, rc):
        assert rc == _lib.KSMI_E_ARG if hasattr(_lib, "KSMI_E_ARG") else rc < 0
        assert entry in lib.ksmi_last_error().decode()

    sizes = [dict(HW=-1), dict(HW=big), dict(N=-1), dict(N=257)]
    zones = lambda present=P, row=P, HW=256, N=7, zone=P: lib.ksmi_scene_quantile_zones(present, row, HW, N, zone, None)
    for kw in sizes + [dict(present=None), dict(row=None), dict(zone=None)]:
        refused("scene_quantile_zones", zones(**kw))
    assert zones(N=0) == 0 and zones(HW=0, N=0) == 0 and zones(N=0, zone=None) == 0
    keys = lambda z=P, wh=None, v=P, row=P, HW=256, N=7, out=P: lib.ksmi_scene_quantile_keys(z, wh, v, row, HW, N, out, None)
    for kw in sizes + [dict(z=None), dict(v=None), dict(row=None), dict(out=None)]:
        refused("scene_quantile_keys", keys(**kw))
    assert keys(N=0) == 0 and keys(HW=0, N=0) == 0
    need = lib.ksmi_scene_quantile_scratch(256)
    sort = lambda a=P, b=2 * P, HW=256, N=7, s=P, elems=need: lib.ksmi_scene_quantile_sort(a, b, HW, N, s, elems, None)
    for kw in sizes + [dict(a=None), dict(b=None), dict(s=None), dict(b=P), dict(elems=need - 1), dict(elems=0)]:
        refused("scene_quantile_sort", sort(**kw))
    assert sort(N=0) == 0 and sort(HW=0, N=0) == 0
    pcts = lambda *c: (ctypes.c_int32 * len(c))(*c)
    select = lambda k=P, HW=256, N=7, c=pcts(5000, 9000), n=2, valid=P, lo=P, hi=P: lib.ksmi_scene_quantile_select(k, HW, N, c, n, valid, lo, hi, None)
    for kw in sizes + [dict(k=None), dict(c=None), dict(valid=None), dict(lo=None), dict(hi=None), dict(n=0), dict(n=-1), dict(n=17),
                       dict(c=pcts(5000, 10001)), dict(c=pcts(-1, 5000)), dict(c=pcts(10001), n=1, N=0)]:
        refused("scene_quantile_select", select(**kw))
    assert select(N=0) == 0 and select(HW=0, N=0) == 0 and select(N=0, c=pcts(*range(16)), n=16) == 0
    segments = lambda k=P, HW=256, N=7, off=P, out=P: lib.ksmi_scene_quantile_segments(k, HW, N, off, out, None)
    for kw in sizes + [dict(k=None), dict(off=None), dict(out=None)]:
        refused("scene_quantile_segments", segments(**kw))
    assert segments(N=0) == 0 and segments(HW=0, N=0) == 0
    assert MAX_ZONAL_BANDS == 8 and MAX_PERCENTILES == 16


def test_the_wrappers_refuse_cpu_tensors_wrong_dtypes_and_too_much():
    import torch
    from kurosiwo_amd import _lib
    z = torch.zeros((8, 8), dtype=torch.int32)
    v = torch.zeros((2, 8, 8), dtype=torch.float32)
    c = torch.zeros((8, 8), dtype=torch.uint8)
    for cpu in (lambda: zonal_quantiles(z, v), lambda: zonal_quantiles(z, v[0], (50, 90), c), lambda: zonal_sorted(z, v[0]),
                lambda: zonal_sorted(z, v[1], c), lambda: component_quantiles(c, v), lambda: component_quantiles(c, v[0], (5,), labels=z)):
        with pytest.raises(_lib.KsmiError):
            cpu()
    many = tuple(range(MAX_PERCENTILES + 1))
    for name, bad in (("zonal_quantiles", (
            lambda: zonal_quantiles(z.long(), v), lambda: zonal_quantiles(z[:, ::2], v), lambda: zonal_quantiles(z.numpy(), v),
            lambda: zonal_quantiles(z, None), lambda: zonal_quantiles(z, v.double()), lambda: zonal_quantiles(z, v[:, :4]),
            lambda: zonal_quantiles(z, torch.zeros((9, 8, 8))), lambda: zonal_quantiles(z, torch.zeros((0, 8, 8))), lambda: zonal_quantiles(z, v[0, 0]),
            lambda: zonal_quantiles(z, v, where=c.int()), lambda: zonal_quantiles(z, v, where=c[:4]), lambda: zonal_quantiles(z, v, ()),
            lambda: zonal_quantiles(z, v, many), lambda: zonal_quantiles(z, v, (50.005,)), lambda: zonal_quantiles(z, v, (101,)),
            lambda: zonal_quantiles(z, v, ("50",)))),
                      ("zonal_sorted", (
            lambda: zonal_sorted(z.long(), v[0]), lambda: zonal_sorted(z, v), lambda: zonal_sorted(z, None), lambda: zonal_sorted(z, v[0].double()),
            lambda: zonal_sorted(z, v[0, :4]), lambda: zonal_sorted(z, v[0], c.int()), lambda: zonal_sorted(z, v[0].numpy()))),
                      ("component_quantiles", (
            lambda: component_quantiles(c.int(), v), lambda: component_quantiles(c[:, ::2], v), lambda: component_quantiles(c, None),
            lambda: component_quantiles(c, torch.zeros((9, 8, 8))), lambda: component_quantiles(c, v, ()), lambda: component_quantiles(c, v, many),
            lambda: component_quantiles(c, v, (0.001,)), lambda: component_quantiles(c, v, select=(63,)),
            lambda: component_quantiles(c, v, labels=z[:4])))):
        for call in bad:
            with pytest.raises(ValueError, match=name):
                call()


def test_predict_refuses_percentiles_without_a_depth_and_a_table_before_reading_a_file():
    import predict
    base = ["--method", "snunet", "--checkpoint", "/nonexistent/best.pt", "--post", "/nonexistent/post.tif", "--pre1", "/nonexistent/pre.tif",
            "--out", "/nonexistent/out.tif", "--percentiles", "50", "90"]
    for extra in ([], ["--depth_out", "/nonexistent/d.tif", "--depth_dem", "/nonexistent/dem.tif"], ["--components", "/nonexistent/c.csv"],
                  ["--polygons", "/nonexistent/p.geojson", "--report", "/nonexistent/r.json"]):
        with pytest.raises(SystemExit, match="--percentiles needs"):
            predict.main(base + extra)
    with pytest.raises(SystemExit, match="--percentiles"):
        predict.main(base[:-2] + ["33.333", "--depth_out", "/nonexistent/d.tif", "--depth_dem", "/nonexistent/dem.tif", "--report", "/nonexistent/r.json"])
