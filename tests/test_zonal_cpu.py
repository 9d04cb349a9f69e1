"""Zonal statistics, host half: the vectorised reference of tests/zonal_ref.py against its per-zone loop, the rounding and saturation
of the fixed-point rule, the key order of the extremes, the three entry points in the library and the binding, their argument checks
(which launch nothing), the refusals of the Python wrappers, and the join of a Zonal to the features of polygons_geojson.  No GPU."""
import ctypes
import json

import numpy as np
import pytest

import polygon_ref
import sieve_ref
import zonal_ref
from kurosiwo_amd.scene import MAX_ZONAL_BANDS, Zonal, component_stats, polygons_geojson, zonal_geometry, zonal_stats

ENTRIES = ("ksmi_scene_zonal_mark", "ksmi_scene_zonal_tables", "ksmi_scene_zonal_accumulate")
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
    zones[skip < 0.1] = -1 - rng.integers(0, 5, size=int((skip < 0.1).sum()))       # negative ids
    zones[(skip >= 0.1) & (skip < 0.2)] = HW + rng.integers(0, 5, size=int(((skip >= 0.1) & (skip < 0.2)).sum()))   # ids >= HW
    values = (rng.normal(0.0, 3.0, size=(B, H, W)) * 10.0 ** rng.integers(-6, 6, size=(B, H, W))).astype(F)
    odd = rng.random((B, H, W))
    values[odd < 0.05] = np.nan
    values[(odd >= 0.05) & (odd < 0.08)] = np.inf
    values[(odd >= 0.08) & (odd < 0.11)] = -np.inf
    values[(odd >= 0.11) & (odd < 0.16)] = -0.0
    values[(odd >= 0.16) & (odd < 0.21)] = 0.0
    values[(odd >= 0.21) & (odd < 0.24)] = F(3e10)                                   # beyond every clamp
    values[(odd >= 0.24) & (odd < 0.27)] = F(-3e10)
    where = (rng.random((H, W)) < 0.7).astype(np.uint8) * 5
    return zones, values, where


@pytest.mark.parametrize("zones_kind", ("few", "own", "any"))
def test_the_vectorised_reference_is_the_loop(zones_kind):
    rng = np.random.default_rng(23)
    for H, W in ((1, 1), (1, 9), (9, 1), (7, 12), (13, 11)):
        for B in (0, 1, 3):
            zones, values, where = _random_case(rng, H, W, B, zones_kind)
            for wh in (None, where):
                for fb in (0, 16, 30):
                    a = zonal_ref.zonal_stats(zones, values if B else None, wh, fb)
                    b = zonal_ref.zonal_stats_loop(zones, values if B else None, wh, fb)
                    assert zonal_ref.same(a, b) == [], (H, W, B, fb, zonal_ref.same(a, b))
                    assert a.zone.dtype == a.count.dtype == a.bbox.dtype == a.valid.dtype == np.int32
                    assert a.sum_x.dtype == a.sum_y.dtype == a.vsum.dtype == np.int64 and a.vmin.dtype == a.vmax.dtype == F
                    assert a.valid.shape == a.vmin.shape == a.vmax.shape == a.vsum.shape == (B, a.zone.size) and a.bbox.shape == (a.zone.size, 4)
                    assert (np.diff(a.zone) > 0).all() and (a.count > 0).all()
    one = zonal_ref.zonal_stats(np.zeros((3, 4), np.int32), np.arange(12, dtype=F).reshape(3, 4), None, 16)      # by hand
    assert one.zone.tolist() == [0] and one.count.tolist() == [12] and one.bbox.tolist() == [[0, 0, 3, 2]]
    assert one.sum_x.tolist() == [18] and one.sum_y.tolist() == [12] and one.vsum.tolist() == [[66 << 16]]
    assert one.vmin.tolist() == [[0.0]] and one.vmax.tolist() == [[11.0]] and zonal_ref.mean(one).tolist() == [5.5]
    empty = zonal_ref.zonal_stats(np.full((3, 4), -1, np.int32), np.zeros((2, 3, 4), F))
    assert empty.zone.shape == (0,) and empty.bbox.shape == (0, 4) and empty.vsum.shape == (2, 0)
    assert zonal_ref.zonal_stats(np.zeros((0, 4), np.int32)).valid.shape == (0, 0)


def test_halves_round_to_even_and_the_clamp_saturates_at_two_to_the_32():
    for fb in (0, 16, 30):
        unit = 2.0 ** -fb
        halves = np.asarray([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, -3.5], np.float64) * unit
        assert (halves.astype(F).astype(np.float64) == halves).all()             # exact in fp32
        assert zonal_ref.quantise(halves.astype(F), fb).tolist() == [0, 2, 2, 4, 0, -2, -2, -4]
        limit = 2.0 ** (32 - fb)
        edge = np.asarray([limit, -limit, limit * 4, -limit * 4, 3e38, -3e38, np.nextafter(F(limit), F(0))], F)
        q = zonal_ref.quantise(edge, fb)
        assert q.dtype == np.int64 and q[:6].tolist() == [2 ** 32, -2 ** 32] * 3 and 0 < q[6] < 2 ** 32
        tiny = np.asarray([unit / 2 * 0.99, -unit / 2 * 0.99, 1e-45, -1e-45], F)    # below half a unit, and a denormal: 0
        assert not zonal_ref.quantise(tiny, fb).any()
    with pytest.raises(ValueError):
        zonal_ref.quantise(F(1), 31)
    assert (2 ** 31 - 1) * 2 ** 32 < 2 ** 63                                       # the sum over a full scene fits int64


def test_the_key_order_and_the_extremes_of_a_zone_without_a_finite_value():
    v = np.asarray([-np.inf, -3e38, -1.0, -1e-45, -0.0, 0.0, 1e-45, 1.0, 3e38, np.inf], F)
    k = zonal_ref.key(v)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all() and k[4] + 1 == k[5]      # -0.0 just below +0.0
    assert zonal_ref.unkey(k).tobytes() == v.tobytes()
    zones = np.asarray([[0, 0, 1, 1, 2]], np.int32)
    values = np.asarray([[[0.0, -0.0, np.nan, np.nan, -0.0]], [[-0.0, 0.0, np.inf, -np.inf, 7.0]]], F)
    for z in (zonal_ref.zonal_stats(zones, values), zonal_ref.zonal_stats_loop(zones, values)):
        assert z.valid.tolist() == [[2, 0, 1], [2, 0, 1]]
        assert z.vmin[:, 1].tolist() == [np.inf, np.inf] and z.vmax[:, 1].tolist() == [-np.inf, -np.inf]
        assert np.signbit(z.vmin[:, 0]).all() and not np.signbit(z.vmax[:, 0]).any() and not z.vmin[:, 0].any() and not z.vmax[:, 0].any()
        assert np.signbit(z.vmin[0, 2]) and np.signbit(z.vmax[0, 2]) and z.vsum.tolist() == [[0, 0, 0], [0, 0, 7 << 16]]
        assert np.isnan(zonal_ref.mean(z, 0)[1]) and zonal_ref.mean(z, 1)[2] == 7.0


def test_library_exports_and_binds_the_zonal_entry_points():
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
    assert lib.ksmi_abi_version() == 8


def test_argument_errors_launch_nothing_and_name_the_entry_point():
    from kurosiwo_amd import _lib
    lib = _lib.load()
    P = 0x1000                                                                  # never dereferenced: every case fails before a launch
    big = 1 << 31

    def refused(entry, rc):
        assert rc < 0
        assert entry in lib.ksmi_last_error().decode()

    mark = lambda z=P, wh=None, HW=256, out=P: lib.ksmi_scene_zonal_mark(z, wh, HW, out, None)
    for kw in (dict(z=None), dict(out=None), dict(HW=-1), dict(HW=big)):
        refused("scene_zonal_mark", mark(**kw))
    assert mark(HW=0) == 0 and mark(HW=0, z=None) == 0
    names = ("present", "row", "zone", "count", "bbox", "sum_x", "sum_y", "valid", "vmin", "vmax", "vsum")

    def tables(HW=256, N=7, B=2, **ptrs):
        p = {k: ptrs.get(k, P) for k in names}
        return lib.ksmi_scene_zonal_tables(p["present"], p["row"], HW, N, B, p["zone"], p["count"], p["bbox"], p["sum_x"], p["sum_y"], p["valid"],
                                           p["vmin"], p["vmax"], p["vsum"], None)
    for kw in [dict(HW=-1), dict(HW=big), dict(N=-1), dict(N=257), dict(B=-1), dict(B=9)] + [{k: None} for k in names]:
        refused("scene_zonal_tables", tables(**kw))
    assert tables(N=0) == 0 and tables(HW=0, N=0) == 0

    def accumulate(B=2, Hs=16, Ws=16, fb=16, N=7, **ptrs):
        p = {k: ptrs.get(k, P) for k in ("zones", "values") + names[1:2] + names[3:]}
        return lib.ksmi_scene_zonal_accumulate(p["zones"], ptrs.get("where"), p["values"], B, Hs, Ws, fb, p["row"], N, p["count"], p["bbox"],
                                               p["sum_x"], p["sum_y"], p["valid"], p["vmin"], p["vmax"], p["vsum"], None)
    for kw in [dict(B=-1), dict(B=9), dict(fb=-1), dict(fb=31), dict(Hs=-1), dict(Ws=-1), dict(Hs=65536, Ws=32768), dict(N=-1), dict(N=257)] + [
            {k: None} for k in ("zones", "values", "row", "count", "bbox", "sum_x", "sum_y", "valid", "vmin", "vmax", "vsum")]:
        refused("scene_zonal_accumulate", accumulate(**kw))
    assert accumulate(N=0) == 0 and accumulate(Hs=0, N=0) == 0
    assert MAX_ZONAL_BANDS == zonal_ref.MAX_BANDS == 8


def test_the_wrappers_refuse_cpu_tensors_wrong_dtypes_and_too_many_bands():
    import torch
    from kurosiwo_amd import _lib
    z = torch.zeros((8, 8), dtype=torch.int32)
    v = torch.zeros((2, 8, 8), dtype=torch.float32)
    c = torch.zeros((8, 8), dtype=torch.uint8)
    for cpu in (lambda: zonal_stats(z), lambda: zonal_stats(z, v, c), lambda: component_stats(c), lambda: component_stats(c, values=v, labels=z)):
        with pytest.raises(_lib.KsmiError):
            cpu()
    for bad in (lambda: zonal_stats(z.long()), lambda: zonal_stats(z.float()), lambda: zonal_stats(z[:, ::2]), lambda: zonal_stats(z[0]),
                lambda: zonal_stats(z.numpy()), lambda: zonal_stats(z, v.double()), lambda: zonal_stats(z, v[:, :4]), lambda: zonal_stats(z, v[:, :, ::2]),
                lambda: zonal_stats(z, torch.zeros((9, 8, 8))), lambda: zonal_stats(z, v[0, 0]), lambda: zonal_stats(z, where=c.int()),
                lambda: zonal_stats(z, where=c[:4]), lambda: zonal_stats(z, where=c.t()[::1].t()[:, ::2]), lambda: zonal_stats(z, frac_bits=31),
                lambda: zonal_stats(z, frac_bits=-1), lambda: zonal_stats(z, frac_bits=16.0), lambda: component_stats(c.int()),
                lambda: component_stats(c[:, ::2]), lambda: component_stats(c, select=(63,)), lambda: component_stats(c, values=torch.zeros((9, 8, 8))),
                lambda: component_stats(c, frac_bits=31), lambda: component_stats(c, labels=z[:4])):
        with pytest.raises(ValueError):
            bad()


def _small_map():
    rng = np.random.default_rng(4)
    c = (rng.random((13, 17)) < 0.45).astype(np.uint8) * rng.integers(1, 3, size=(13, 17)).astype(np.uint8)
    c[5:9, 3:9] = 2
    c[6:8, 5:7] = 0                                                              # a hole
    c[0, 0] = 3
    return c


def test_geojson_without_attributes_is_what_it_was():
    c = _small_map()
    for kw in (dict(), dict(pixel_scale=(10.0, 20.0), origin=(500000.0, 4100000.0))):
        rings = polygon_ref.rings(c)
        plain = json.dumps(polygons_geojson(rings, c, **kw))
        assert plain == json.dumps(polygons_geojson(rings, c, attributes=None, **kw)) == json.dumps(polygon_ref.geojson(rings, c, **kw))
        assert "bbox" not in plain and "centroid" not in plain and len(json.loads(plain)["features"]) > 3


def test_attributes_join_by_label_with_a_bbox_around_every_vertex():
    c = _small_map()
    labels = sieve_ref.label(c, 4).astype(np.int32)
    where = polygon_ref.selected(c, (1, 2)).astype(np.uint8)
    depth = np.random.default_rng(5).random(c.shape).astype(F)
    z = zonal_ref.zonal_stats(labels, depth, where)
    rings = polygon_ref.rings(c)
    assert np.array_equal(z.zone, np.unique(rings.label)) and np.array_equal(4 * z.zone, rings.ring_id[np.isin(rings.ring_id, 4 * z.zone)])
    tag = [f"row{r}" for r in range(z.zone.size)]
    geo = dict(pixel_scale=(10.0, 20.0), origin=(500000.0, 4100000.0))
    for kw in (dict(), geo):
        plain = polygons_geojson(rings, c, **kw)["features"]
        got = polygons_geojson(rings, c, attributes=(Zonal(*z), {"tag": tag, "depth_pixels": z.valid[0]}), **kw)["features"]
        only = polygons_geojson(rings, c, attributes=Zonal(*z), **kw)["features"]
        boxes, cx, cy = zonal_geometry(z, **kw)
        assert len(got) == len(plain) == len(only) == z.zone.size
        sx, sy = kw.get("pixel_scale", (1.0, 1.0))
        ox, oy = kw.get("origin", (0.0, 0.0))
        for r, (f, p, o) in enumerate(zip(got, plain, only)):
            assert f["geometry"] == p["geometry"] == o["geometry"] and list(f["properties"])[:3] == list(p["properties"])
            assert list(f["properties"]) == ["class", "pixels", "area", "centroid_x", "centroid_y", "tag", "depth_pixels"]
            assert list(o["properties"]) == ["class", "pixels", "area", "centroid_x", "centroid_y"] and o["bbox"] == f["bbox"]
            assert f["properties"]["pixels"] == int(z.count[r]) and f["properties"]["tag"] == tag[r]
            assert f["properties"]["depth_pixels"] == int(z.valid[0, r]) == int(z.count[r])
            west, south, east, north = f["bbox"]
            x0, y0, x1, y1 = (int(v) for v in z.bbox[r])
            assert (west, south, east, north) == (ox + x0 * sx, oy - (y1 + 1) * sy, ox + (x1 + 1) * sx, oy - y0 * sy) == tuple(boxes[r])
            xs = [v[0] for ring in f["geometry"]["coordinates"] for v in ring]
            ys = [v[1] for ring in f["geometry"]["coordinates"] for v in ring]
            assert min(xs) == west and max(xs) == east and min(ys) == south and max(ys) == north      # tight: the exterior ring touches it
            n = int(z.count[r])
            assert f["properties"]["centroid_x"] == ox + (int(z.sum_x[r]) + n / 2) / n * sx == cx[r]
            assert f["properties"]["centroid_y"] == oy - (int(z.sum_y[r]) + n / 2) / n * sy == cy[r]
            assert west < f["properties"]["centroid_x"] < east and south < f["properties"]["centroid_y"] < north
        json.dumps(got)
    short = Zonal(*[t[..., 1:] if i in (5, 6, 7, 8) else t[1:] if i < 5 else t for i, t in enumerate(z)])     # the first row is missing
    feats = polygons_geojson(rings, c, attributes=(short, {"tag": tag[1:]}))["features"]
    assert "bbox" not in feats[0] and feats[0]["properties"]["tag"] is None and feats[0]["properties"]["centroid_x"] is None
    assert feats[0]["properties"]["pixels"] == int(z.count[0]) and [f["properties"]["tag"] for f in feats[1:]] == tag[1:]
    with pytest.raises(ValueError):
        polygons_geojson(rings, c, attributes=(Zonal(*z), {"tag": tag[1:]}))
