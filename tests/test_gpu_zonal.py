"""Zonal statistics on the device (csrc/zonal.hip, kurosiwo_amd/scene.py: zonal_stats, component_stats; predict.py --polygons
attributes, --components) against tests/zonal_ref.py, equal bit for bit in every field: zone maps that exercise the run combining
inside a wave, the slot table of a workgroup and its overflow, the cross-workgroup adds and the row ends; value rasters with NaN,
infinities, signed zeros, exact halves and values beyond the clamp; `where`; two runs give equal bits; empty scenes; the components
of a class map against component_sizes and polygonize; predict.py end to end."""
import csv
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import polygon_ref
import sieve_ref
import zonal_ref
from kurosiwo_amd.scene import (ZONAL_BLOCK, Zonal, component_sizes, component_stats, label_components, polygonize, polygons_geojson,
                                select_classes, zonal_stats)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 130), (130, 1), (67, 133), (150, 300))
MAPS = ("one", "own", "labels0.1", "labels30", "stripes1", "stripes63", "stripes64", "stripes65", "bands", "gaps", "collide")
# (B, frac_bits, with where): every B with every frac_bits, with and without where
RUNS = ((0, 16, False), (0, 0, True), (1, 0, False), (1, 16, True), (1, 30, False), (3, 0, True), (3, 16, False), (3, 30, True))
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _slot(z):
    """the slot of zone z in a workgroup's table: slot_of in csrc/zonal.hip, (z * 2654435761 mod 2^32) >> 26"""
    return ((int(z) * 2654435761) & 0xFFFFFFFF) >> 26


def _colliding(HW):
    """the two smallest distinct zone ids below HW that share a slot, found by walking the ids in ascending order and hashing each as
    the kernel does; with fewer than two ids, or no collision among them, the ids 0 and HW - 1"""
    seen = {}
    for z in range(HW):
        if _slot(z) in seen:
            return seen[_slot(z)], z
        seen[_slot(z)] = z
    return 0, max(HW - 1, 0)


@functools.lru_cache(maxsize=None)
def _zones(shape, kind):
    H, W = shape
    HW = H * W
    rng = np.random.default_rng(H * 1000 + W)
    yy, xx = np.mgrid[0:H, 0:W]
    if kind == "one":
        z = np.zeros(shape, np.int64)
    elif kind == "own":
        z = np.arange(HW).reshape(shape)
    elif kind.startswith("labels"):
        classes = (rng.random(shape) < float(kind[6:]) / 100).astype(np.uint8)
        return label_components(_dev(classes), 4).cpu().numpy()
    elif kind.startswith("stripes"):
        z = xx // int(kind[7:])                                               # run ends on, before and after a wave boundary
    elif kind == "bands":
        z = yy // 3 * 5 % HW                                                  # rows of one zone follow each other in memory
    elif kind == "gaps":
        ids = np.concatenate((rng.integers(0, HW, size=7), [0, HW - 1, -1, -7, HW, HW + 3, 2 ** 31 - 1, -2 ** 31]))
        z = ids[rng.integers(0, ids.size, size=shape)]
        z = np.where(rng.random(shape) < 0.5, z, np.roll(z, 1, axis=1))        # some runs, some lone pixels
    elif kind == "collide":
        a, b = _colliding(HW)
        assert HW < 65 or (a != b and _slot(a) == _slot(b))
        blocks = np.kron(rng.integers(0, 2, size=(-(-H // 4), -(-W // 16))), np.ones((4, 16), np.int64))[:H, :W]
        z = np.where(blocks == 1, a, b)
        z[rng.random(shape) < 0.1] = a
    return np.ascontiguousarray(z.astype(np.int32))


@functools.lru_cache(maxsize=None)
def _values(shape, B, frac_bits):
    """random fp32 around the clamp of `frac_bits`, with NaN, +-inf, -0.0, exact halves, values beyond the clamp; band 1 is all NaN"""
    H, W = shape
    rng = np.random.default_rng(H * 77 + W + frac_bits)
    v = (rng.normal(0.0, 1.0, size=(B, H, W)) * 2.0 ** (30 - frac_bits)).astype(F)
    odd = rng.random((B, H, W))
    v[odd < 0.05] = np.nan
    v[(odd >= 0.05) & (odd < 0.07)] = np.inf
    v[(odd >= 0.07) & (odd < 0.09)] = -np.inf
    v[(odd >= 0.09) & (odd < 0.13)] = -0.0
    v[(odd >= 0.13) & (odd < 0.16)] = 0.0
    halves = ((rng.integers(-9, 9, size=(B, H, W)) + 0.5) * 2.0 ** -frac_bits).astype(F)
    v = np.where((odd >= 0.16) & (odd < 0.4), halves, v)
    v[(odd >= 0.4) & (odd < 0.42)] = F(2.0 ** (33 - frac_bits))                # beyond the clamp
    v[(odd >= 0.42) & (odd < 0.44)] = F(-3e38)
    if B:
        v[0].flat[0] = F(3e38)                                                # one for sure
    if B > 1:
        v[1] = np.nan
    return np.ascontiguousarray(v.astype(F))


@functools.lru_cache(maxsize=None)
def _where(shape):
    rng = np.random.default_rng(shape[0] + shape[1])
    blocks = np.kron((rng.random((-(-shape[0] // 8), -(-shape[1] // 64))) < 0.5).astype(np.uint8), np.ones((8, 64), np.uint8))[:shape[0], :shape[1]]
    return np.ascontiguousarray(np.where(rng.random(shape) < 0.8, blocks, 1 - blocks).astype(np.uint8) * 201)


def _check(zones, values, where, frac_bits, what):
    """zonal_stats on the device against the reference, every field as bits; the inputs unchanged; two runs equal -> the reference"""
    want = zonal_ref.zonal_stats(zones, values, where, frac_bits)
    z, v, w = _dev(zones), None if values is None else _dev(values), None if where is None else _dev(where)
    got = zonal_stats(z, v, w, frac_bits)
    assert isinstance(got, Zonal) and all(t.is_cuda for t in got[:-1]) and got.frac_bits == frac_bits
    bad = zonal_ref.same(got, want)
    print(f"{what}: {want.zone.size} zones, largest {int(want.count.max()) if want.zone.size else 0} pixels, finite values "
          f"{want.valid.sum(axis=1).tolist()}; fields that differ: {bad}")
    assert bad == []
    assert torch.equal(z.cpu(), torch.from_numpy(zones))
    assert v is None or torch.equal(v.cpu().view(torch.int32), torch.from_numpy(values).view(torch.int32))
    assert w is None or torch.equal(w.cpu(), torch.from_numpy(where))
    assert zonal_ref.same(zonal_stats(z, v, w, frac_bits), got) == []
    return want


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_field_equals_the_reference(shape, kind):
    zones = _zones(shape, kind)
    for B, frac_bits, masked in RUNS:
        values = _values(shape, 3, frac_bits)[:B] if B else None
        want = _check(zones, values, _where(shape) if masked else None, frac_bits, f"{shape} {kind} B={B} frac_bits={frac_bits} where={masked}")
        if B == 3:
            assert not want.valid[1].any() and np.isposinf(want.vmin[1]).all() and np.isneginf(want.vmax[1]).all() and not want.vsum[1].any()
    plain = zonal_ref.zonal_stats(zones)
    if kind == "one":
        assert plain.zone.tolist() == [0] and plain.count.tolist() == [zones.size] and plain.bbox.tolist() == [[0, 0, shape[1] - 1, shape[0] - 1]]
    if kind == "own":
        assert plain.zone.size == zones.size and (plain.count == 1).all()
        assert shape == (1, 1) or zones.size > ZONAL_BLOCK[1]                  # more zones in a workgroup than slots: the overflow path
    if kind == "bands" and shape[1] in (133, 300):
        assert shape[1] % 64 and (plain.bbox[:, 0] == 0).all() and (plain.bbox[:, 2] == shape[1] - 1).all()  # rows end mid-wave
    if kind == "collide" and zones.size > 64:
        assert plain.zone.size == 2 and _slot(plain.zone[0]) == _slot(plain.zone[1])


def test_a_two_dimensional_value_raster_is_one_band():
    zones, values = _zones((67, 133), "labels30"), _values((67, 133), 3, 16)
    a, b = zonal_stats(_dev(zones), _dev(values[0])), zonal_stats(_dev(zones), _dev(values[:1]))
    assert a.valid.shape == (1, a.zone.numel()) and zonal_ref.same(a, b) == []


def test_an_empty_scene_and_a_scene_of_skipped_pixels_give_empty_tables():
    cases = [(torch.empty(s, dtype=torch.int32, device="cuda"), None) for s in ((0, 5), (5, 0))]
    cases += [(torch.full((9, 70), -1, dtype=torch.int32, device="cuda"), None), (torch.full((9, 70), 9 * 70, dtype=torch.int32, device="cuda"), None),
              (torch.zeros((9, 70), dtype=torch.int32, device="cuda"), torch.zeros((9, 70), dtype=torch.uint8, device="cuda"))]
    for zones, where in cases:
        for B in (0, 2):
            values = torch.ones((B,) + tuple(zones.shape), device="cuda") if B else None
            got = zonal_stats(zones, values, where)
            want = zonal_ref.zonal_stats(zones.cpu().numpy(), None if values is None else values.cpu().numpy(), None if where is None else where.cpu().numpy())
            assert zonal_ref.same(got, want) == [] and got.zone.shape == (0,) and got.bbox.shape == (0, 4) and got.vsum.shape == (B, 0)


@pytest.mark.parametrize("kind", ("one", "stripes1", "labels30", "bands"))
def test_a_tall_scene_of_short_rows(kind):
    """8200 rows of 3 pixels: a zone spans seven workgroups along y, and every run is cut after three lanes"""
    shape = (8200, 3)
    assert shape[0] * shape[1] > 6 * ZONAL_BLOCK[0]
    _check(_zones(shape, kind), _values(shape, 3, 16), _where(shape), 16, f"{shape} {kind}")
    _check(_zones(shape, kind), _values(shape, 3, 30)[:1], None, 30, f"{shape} {kind}")


def test_component_stats_lines_up_with_the_sizes_and_the_rings():
    rng = np.random.default_rng(12)
    classes = (rng.random((150, 300)) < 0.55).astype(np.uint8) * rng.integers(1, 4, size=(150, 300)).astype(np.uint8)
    values = _values((150, 300), 3, 16)
    c = _dev(classes)
    got = component_stats(c, values=_dev(values))
    labels = label_components(c, 4)
    chosen = polygon_ref.selected(classes, (1, 2))
    assert np.array_equal(got.zone.cpu().numpy(), np.unique(labels.cpu().numpy()[chosen]))
    assert np.array_equal(got.count.cpu().numpy(), component_sizes(labels).cpu().numpy().ravel()[got.zone.cpu().numpy()])
    rings = polygonize(c)
    exterior = rings.ring_id == 4 * rings.label
    assert torch.equal(rings.label[exterior], got.zone) and torch.equal(torch.unique(rings.label), got.zone)
    want = zonal_ref.zonal_stats(labels.cpu().numpy(), values, chosen.astype(np.uint8))
    assert zonal_ref.same(got, want) == []
    assert zonal_ref.same(component_stats(c, values=_dev(values), labels=labels), want) == []
    assert zonal_ref.same(zonal_stats(labels, _dev(values), select_classes(c, (1, 2))), want) == []
    feats = polygons_geojson(rings, c, attributes=got)["features"]
    assert [f["properties"]["pixels"] for f in feats] == got.count.tolist() and all("bbox" in f for f in feats)
    other = component_stats(c, select=(3,), frac_bits=0)
    assert zonal_ref.same(other, zonal_ref.zonal_stats(labels.cpu().numpy(), None, (classes == 3).astype(np.uint8), 0)) == []


# ---------------------------------------------------------------------------------------------------- predict.py
def _tiny_scene(tmp_path):
    """a tiny SNUNet checkpoint, georeferenced rasters and a raw DEM, as tests/test_gpu_depth.py and tests/test_gpu_sieve.py build theirs"""
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
    return [sys.executable, os.path.join(ROOT, "predict.py"), "--task", "cd", "--method", "snunet", "--checkpoint", str(tmp_path / "best.pt"),
            "--post", str(tmp_path / "post_vv.tif"), str(tmp_path / "post_vh.tif"), "--pre1", str(tmp_path / "pre.tif"),
            "--window", "32", "--stride", "16", "--batch_size", "5", "--precision", "fp32"]


def test_predict_script_with_component_attributes(tmp_path):
    from kurosiwo_amd import geotiff
    cmd = _tiny_scene(tmp_path)
    p = lambda name: str(tmp_path / name)
    run = subprocess.run(cmd + ["--out", p("flood.tif"), "--mmu", "6", "--polygons", p("flood.geojson"), "--depth_out", p("d.tif"), "--depth_dem",
                                p("dem.tif"), "--score", "softmax", "--score_out", p("s.tif"), "--components", p("c.csv"), "--report", p("r.json")],
                         cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    classes, meta = geotiff.read(p("flood.tif"))
    depth, _ = geotiff.read(p("d.tif"))
    score, _ = geotiff.read(p("s.tif"), squeeze=False)
    assert depth.dtype == score.dtype == np.float32 and depth.shape == classes.shape == score.shape[1:] == (80, 72) and score.shape[0] == 3
    scale, origin, area = meta["pixel_scale"], meta["origin"], 100.0
    labels = sieve_ref.label(classes, 4).astype(np.int32)
    chosen = polygon_ref.selected(classes, (1, 2)).astype(np.uint8)
    deep = zonal_ref.zonal_stats(labels, np.ascontiguousarray(depth), chosen, 16)
    conf = zonal_ref.zonal_stats(labels, np.ascontiguousarray(score), chosen, 30)
    N = deep.zone.size
    own = classes.ravel()[deep.zone].astype(int)
    assert N >= 3 and np.array_equal(deep.zone, conf.zone) and set(own.tolist()) <= {1, 2}
    want = []
    for r in range(N):
        n, k = int(deep.count[r]), int(deep.valid[0, r])
        metres = int(deep.vsum[0, r]) / float(2 ** 16)
        ck = int(conf.valid[own[r], r])
        want.append({"label": int(deep.zone[r]), "class": int(own[r]), "pixels": n, "x0": int(deep.bbox[r, 0]), "y0": int(deep.bbox[r, 1]),
                     "x1": int(deep.bbox[r, 2]), "y1": int(deep.bbox[r, 3]),
                     "centroid_x": origin[0] + (int(deep.sum_x[r]) + n / 2.0) / n * scale[0],
                     "centroid_y": origin[1] - (int(deep.sum_y[r]) + n / 2.0) / n * scale[1],
                     "depth_pixels": k, "depth_max": float(deep.vmax[0, r]) if k else None, "depth_mean": metres / k if k else None,
                     "volume": metres * area, "confidence": int(conf.vsum[own[r], r]) / float(2 ** 30) / ck if ck else None})
    print(f"predict.py components: {N}, pixels {[w['pixels'] for w in want][:8]}, depth_pixels {[w['depth_pixels'] for w in want][:8]}, "
          f"confidence {[w['confidence'] for w in want][:4]}")
    assert any(w["depth_pixels"] for w in want) and all(w["confidence"] is not None and 0.0 < w["confidence"] <= 1.0 for w in want)
    # the CSV: the fixed header, then one row per component in ascending label
    with open(p("c.csv"), newline="") as f:
        rows = list(csv.reader(f))
    header = ["label", "class", "pixels", "x0", "y0", "x1", "y1", "centroid_x", "centroid_y", "depth_pixels", "depth_max", "depth_mean", "volume",
              "confidence"]
    assert rows[0] == header and len(rows) == N + 1
    floats = {"centroid_x", "centroid_y", "depth_max", "depth_mean", "volume", "confidence"}
    for row, w in zip(rows[1:], want):
        got = {k: None if v == "" else float(v) if k in floats else int(v) for k, v in zip(header, row)}
        assert got == w
    # the GeoJSON: geometry and the old properties as before, the new ones from the tables
    with open(p("flood.geojson")) as f:
        written = json.load(f)
    rings = polygon_ref.rings(classes, (1, 2))
    plain = polygon_ref.geojson(rings, classes, pixel_scale=scale, origin=origin)
    assert len(written["features"]) == len(plain["features"]) == N
    for f, old, w in zip(written["features"], plain["features"], want):
        assert f["geometry"] == old["geometry"] and {k: f["properties"][k] for k in old["properties"]} == old["properties"]
        assert list(f["properties"]) == ["class", "pixels", "area", "centroid_x", "centroid_y", "depth_pixels", "depth_max", "depth_mean", "volume",
                                         "confidence"]
        assert f["properties"] == {**old["properties"], **{k: w[k] for k in list(f["properties"])[3:]}} and f["properties"]["pixels"] == w["pixels"]
        assert f["bbox"] == [origin[0] + w["x0"] * scale[0], origin[1] - (w["y1"] + 1) * scale[1], origin[0] + (w["x1"] + 1) * scale[0],
                             origin[1] - w["y0"] * scale[1]]
    report = json.load(open(p("r.json")))
    top = int(np.argmax(deep.count))
    assert report["components"] == {"count": N, "largest": {"label": int(deep.zone[top]), "pixels": int(deep.count[top])}}
    assert list(report)[-2:] == ["depth", "components"]
    # without the new flags: the bytes polygons_geojson gives without attributes, and a report without "components"
    again = subprocess.run(cmd + ["--out", p("flood2.tif"), "--mmu", "6", "--polygons", p("plain.geojson"), "--report", p("r2.json")],
                           cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert again.returncode == 0, again.stdout + again.stderr
    c = _dev(classes)
    assert open(p("plain.geojson")).read() == json.dumps(polygons_geojson(polygonize(c), classes, pixel_scale=scale, origin=origin))
    assert json.load(open(p("plain.geojson"))) == plain and open(p("flood2.tif"), "rb").read() == open(p("flood.tif"), "rb").read()
    assert "components" in json.load(open(p("r2.json"))) and "depth" not in json.load(open(p("r2.json")))
