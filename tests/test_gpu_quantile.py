"""Percentiles per zone on the device (csrc/quantile.hip, kurosiwo_amd/scene.py: zonal_quantiles, zonal_sorted, component_quantiles;
predict.py --percentiles) against tests/quantile_ref.py, equal bit for bit: zone maps whose element counts cross several sort tiles
and end inside one, and whose row counts need one, two, three and four row digits; value rasters with NaN, infinities, both zeros,
heavy ties and +-3e38; `where`; a band without a finite value; two runs give equal bits; the sorted segments themselves; the
components of a class map against component_stats and polygonize; predict.py end to end."""
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
import quantile_ref
import sieve_ref
from kurosiwo_amd import _lib
from kurosiwo_amd.scene import (QUANTILE_TILE, ZonalQuantiles, component_quantiles, component_stats, label_components, polygonize,
                                quantile_values, select_classes, zonal_quantiles, zonal_sorted, zonal_stats)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 130), (130, 1), (67, 133), (150, 300))
MAPS = ("one", "own", "labels30", "stripes63", "stripes64", "stripes65", "bands", "gaps")
PERCENTS = (0, 0.01, 25, 50, 97.5, 99.99, 100)
F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


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
        z = xx // int(kind[7:])
    elif kind == "bands":
        z = yy // 3 * 5 % HW
    elif kind == "gaps":
        ids = np.concatenate((rng.integers(0, HW, size=7), [0, HW - 1, -1, -7, HW, HW + 3, 2 ** 31 - 1, -2 ** 31]))
        z = ids[rng.integers(0, ids.size, size=shape)]
        z = np.where(rng.random(shape) < 0.5, z, np.roll(z, 1, axis=1))
    return np.ascontiguousarray(z.astype(np.int32))


@functools.lru_cache(maxsize=None)
def _values(shape):
    """three bands: random fp32 over many magnitudes; values drawn from 5 levels (heavy ties, both zeros among them); band 1 all NaN;
    NaN, +-inf and +-3e38 in the others"""
    H, W = shape
    rng = np.random.default_rng(H * 77 + W)
    v = (rng.normal(0.0, 3.0, size=(3, H, W)) * 10.0 ** rng.integers(-6, 6, size=(3, H, W))).astype(F)
    levels = np.asarray([-2.5, -0.0, 0.0, 1.0, 7.25], F)
    v[2] = levels[rng.integers(0, 5, size=(H, W))]                             # band 2: ties only
    v[0] = np.where(rng.random((H, W)) < 0.3, levels[rng.integers(0, 5, size=(H, W))], v[0])
    odd = rng.random((3, H, W))
    v[odd < 0.05] = np.nan
    v[(odd >= 0.05) & (odd < 0.07)] = np.inf
    v[(odd >= 0.07) & (odd < 0.09)] = -np.inf
    v[(odd >= 0.09) & (odd < 0.12)] = F(3e38)
    v[(odd >= 0.12) & (odd < 0.15)] = F(-3e38)
    v[1] = np.nan
    return np.ascontiguousarray(v.astype(F))


@functools.lru_cache(maxsize=None)
def _where(shape):
    rng = np.random.default_rng(shape[0] + shape[1])
    blocks = np.kron((rng.random((-(-shape[0] // 8), -(-shape[1] // 64))) < 0.5).astype(np.uint8), np.ones((8, 64), np.uint8))[:shape[0], :shape[1]]
    return np.ascontiguousarray(np.where(rng.random(shape) < 0.8, blocks, 1 - blocks).astype(np.uint8) * 201)


def _check(zones, values, where, what, percents=PERCENTS):
    """zonal_quantiles on the device against the reference, every field as bits; valid against zonal_stats; the inputs unchanged; two
    runs equal -> the reference"""
    want = quantile_ref.zonal_quantiles(zones, values, percents, where)
    z, v, w = _dev(zones), _dev(values), None if where is None else _dev(where)
    got = zonal_quantiles(z, v, percents, w)
    assert isinstance(got, ZonalQuantiles) and all(t.is_cuda for t in got[:-1]) and got.percentiles == want.percentiles
    bad = quantile_ref.same(got, want)
    print(f"{what}: {want.zone.size} zones ({_lib.load().ksmi_scene_quantile_passes(want.zone.size)} passes), finite values "
          f"{want.valid.sum(axis=1).tolist()}; fields that differ: {bad}")
    assert bad == []
    stats = zonal_stats(z, v, w)
    assert torch.equal(got.valid, stats.valid) and torch.equal(got.zone, stats.zone)
    assert torch.equal(z.cpu(), torch.from_numpy(zones))
    assert torch.equal(v.cpu().view(torch.int32), torch.from_numpy(values).view(torch.int32))
    assert w is None or torch.equal(w.cpu(), torch.from_numpy(where))
    assert quantile_ref.same(zonal_quantiles(z, v, percents, w), got) == []
    return want


@pytest.mark.parametrize("kind", MAPS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_field_equals_the_reference(shape, kind):
    zones = _zones(shape, kind)
    for B, masked in ((1, False), (1, True), (3, False), (3, True)):
        want = _check(zones, _values(shape)[:B], _where(shape) if masked else None, f"{shape} {kind} B={B} where={masked}")
        if B == 3:
            assert not want.valid[1].any() and np.isnan(want.lower[1]).all() and np.isnan(want.higher[1]).all()
            assert want.lower[1].view(np.uint32).tolist() == [[0x7FC00000] * want.zone.size] * len(PERCENTS)
    lib = _lib.load()
    if shape[0] * shape[1] > 1:
        assert zones.size % QUANTILE_TILE                                      # every scene ends inside a sort tile
    if shape in ((67, 133), (150, 300)):
        assert zones.size in (8911, 45000) and zones.size > 2 * QUANTILE_TILE  # several sort tiles
    if kind == "one":
        assert lib.ksmi_scene_quantile_passes(1) == 4                          # no row digit
    if kind == "own" and shape == (150, 300):
        assert want.zone.size > 256 and lib.ksmi_scene_quantile_passes(want.zone.size) == 6        # two row digits


@pytest.mark.parametrize("kind", ("own", "labels30"))
def test_three_row_digits(kind):
    shape = (260, 260)
    want = _check(_zones(shape, kind), _values(shape)[:1], None, f"{shape} {kind}", (0.01, 50, 99.99))
    if kind == "own":
        assert want.zone.size > 65536 and _lib.load().ksmi_scene_quantile_passes(want.zone.size) == 7
    _check(_zones(shape, kind), _values(shape)[2:], _where(shape), f"{shape} {kind} ties where=True", (50,))


def test_four_row_digits_every_pixel_its_own_zone():
    """4100 x 4100, N = 16 810 000 > 2^24: the expectation is closed form, lower = higher = the pixel's value where it is finite"""
    H = W = 4100
    rng = np.random.default_rng(41)
    values = rng.standard_normal(H * W, dtype=F)
    values[::7] = np.nan
    values[3::1001] = np.inf
    values[5::1003] = -np.inf
    values[11::13] = -0.0
    v = torch.from_numpy(values).cuda().view(H, W)
    zones = torch.arange(H * W, dtype=torch.int32, device="cuda").view(H, W)
    assert H * W > 2 ** 24 and _lib.load().ksmi_scene_quantile_passes(H * W) == 8
    got = zonal_quantiles(zones, v, (50,))
    fin = torch.isfinite(v).view(-1)
    bits = v.view(-1).view(torch.int32)
    want = torch.where(fin, bits, torch.full_like(bits, 0x7FC00000))
    assert got.percentiles == (5000,) and got.lower.shape == got.higher.shape == (1, 1, H * W) and got.valid.shape == (1, H * W)
    assert torch.equal(got.zone, zones.view(-1)) and torch.equal(got.valid[0], fin.to(torch.int32))
    assert torch.equal(got.lower.view(torch.int32).view(-1), want) and torch.equal(got.higher.view(torch.int32).view(-1), want)
    assert torch.equal(v.view(-1).cpu().view(torch.int32), torch.from_numpy(values).view(torch.int32))


def test_a_two_dimensional_value_raster_is_one_band_and_the_order_of_the_percentiles_is_kept():
    zones, values = _zones((67, 133), "labels30"), _values((67, 133))
    a, b = zonal_quantiles(_dev(zones), _dev(values[0]), (90, 10)), zonal_quantiles(_dev(zones), _dev(values[:1]), (90, 10))
    assert a.lower.shape == (1, 2, a.zone.numel()) and quantile_ref.same(a, b) == [] and a.percentiles == (9000, 1000)
    assert quantile_ref.same(a, quantile_ref.zonal_quantiles(zones, values[0], (90, 10))) == []
    host = quantile_values(a)
    assert host.dtype == np.float64 and host.tobytes() == quantile_ref.values(a).tobytes()


def test_an_empty_scene_and_a_scene_of_skipped_pixels_give_empty_tables():
    cases = [(torch.empty(s, dtype=torch.int32, device="cuda"), None) for s in ((0, 5), (5, 0))]
    cases += [(torch.full((9, 70), -1, dtype=torch.int32, device="cuda"), None), (torch.full((9, 70), 9 * 70, dtype=torch.int32, device="cuda"), None),
              (torch.zeros((9, 70), dtype=torch.int32, device="cuda"), torch.zeros((9, 70), dtype=torch.uint8, device="cuda"))]
    for zones, where in cases:
        values = torch.ones((2,) + tuple(zones.shape), device="cuda")
        got = zonal_quantiles(zones, values, (50, 90, 100), where)
        assert got.zone.shape == (0,) and got.valid.shape == (2, 0) and got.lower.shape == got.higher.shape == (2, 3, 0)
        assert got.zone.dtype == got.valid.dtype == torch.int32 and got.lower.dtype == torch.float32
        zone, offsets, flat = zonal_sorted(zones, values[0], where)
        assert zone.shape == (0,) and offsets.tolist() == [0] and flat.shape == (zones.numel(),)


@pytest.mark.parametrize("kind", ("one", "labels30", "stripes65", "gaps"))
def test_the_sorted_segments(kind):
    shape = (150, 300)
    zones, values, where = _zones(shape, kind), _values(shape), _where(shape)
    for band, wh in ((0, None), (0, where), (1, where), (2, None)):
        want = quantile_ref.zonal_sorted(zones, values[band], wh)
        v = _dev(values[band])
        zone, offsets, flat = zonal_sorted(_dev(zones), v, None if wh is None else _dev(wh))
        assert zone.dtype == offsets.dtype == torch.int32 and flat.dtype == torch.float32 and flat.shape == (zones.size,)
        assert np.array_equal(zone.cpu().numpy(), want[0]) and np.array_equal(offsets.cpu().numpy(), want[1])
        assert flat.cpu().numpy()[:int(want[1][-1])].tobytes() == want[2].tobytes()
        assert torch.equal(v.cpu().view(torch.int32), torch.from_numpy(values[band]).view(torch.int32))
        if band == 1:
            assert int(want[1][-1]) == 0


def test_component_quantiles_lines_up_with_component_stats_and_the_rings():
    rng = np.random.default_rng(12)
    classes = (rng.random((67, 133)) < 0.55).astype(np.uint8) * rng.integers(1, 4, size=(67, 133)).astype(np.uint8)
    values = _values((67, 133))
    c, v = _dev(classes), _dev(values)
    got = component_quantiles(c, v, PERCENTS)
    stats = component_stats(c, values=v)
    labels = label_components(c, 4)
    chosen = polygon_ref.selected(classes, (1, 2)).astype(np.uint8)
    assert torch.equal(got.zone, stats.zone) and torch.equal(got.valid, stats.valid) and got.zone.numel() > 20
    rings = polygonize(c)
    assert torch.equal(rings.label[rings.ring_id == 4 * rings.label], got.zone)
    want = quantile_ref.zonal_quantiles(labels.cpu().numpy(), values, PERCENTS, chosen)
    assert quantile_ref.same(got, want) == []
    assert quantile_ref.same(component_quantiles(c, v, PERCENTS, labels=labels), want) == []
    assert quantile_ref.same(zonal_quantiles(labels, v, PERCENTS, select_classes(c, (1, 2))), want) == []
    some = (stats.valid > 0)
    assert torch.equal(got.lower[:, 0][some].view(torch.int32), stats.vmin[some].view(torch.int32))      # percentile 0 and 100: the extremes
    assert torch.equal(got.higher[:, -1][some].view(torch.int32), stats.vmax[some].view(torch.int32))
    other = component_quantiles(c, v[0], (50,), select=(3,))
    assert quantile_ref.same(other, quantile_ref.zonal_quantiles(labels.cpu().numpy(), values[0], (50,), (classes == 3).astype(np.uint8))) == []


# ---------------------------------------------------------------------------------------------------- predict.py
def _tiny_scene(tmp_path):
    """a tiny SNUNet checkpoint, georeferenced rasters and a raw DEM, as tests/test_gpu_zonal.py builds its own"""
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


def test_predict_script_with_percentiles(tmp_path):
    from kurosiwo_amd import geotiff
    cmd = _tiny_scene(tmp_path)
    p = lambda name: str(tmp_path / name)
    outputs = lambda tag: ["--out", p(f"flood{tag}.tif"), "--mmu", "6", "--polygons", p(f"flood{tag}.geojson"), "--depth_out", p(f"d{tag}.tif"),
                           "--depth_dem", p("dem.tif"), "--components", p(f"c{tag}.csv"), "--report", p(f"r{tag}.json")]
    run = subprocess.run(cmd + outputs("") + ["--percentiles", "50", "90"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    classes, _ = geotiff.read(p("flood.tif"))
    depth, _ = geotiff.read(p("d.tif"))
    labels = sieve_ref.label(classes, 4).astype(np.int32)
    chosen = polygon_ref.selected(classes, (1, 2)).astype(np.uint8)
    ref = quantile_ref.zonal_quantiles(labels, np.ascontiguousarray(depth), (50, 90), chosen)
    lin = quantile_ref.values(ref)[0]
    N = ref.zone.size
    want = [{"depth_p50": None if ref.valid[0, r] == 0 else float(lin[0, r]), "depth_p90": None if ref.valid[0, r] == 0 else float(lin[1, r])}
            for r in range(N)]
    print(f"predict.py --percentiles: {N} components, finite depths {ref.valid[0].tolist()[:8]}, p50 {[w['depth_p50'] for w in want][:4]}, "
          f"p90 {[w['depth_p90'] for w in want][:4]}")
    assert N >= 3 and any(w["depth_p50"] is not None for w in want)
    assert any(w["depth_p50"] is not None and w["depth_p90"] > w["depth_p50"] for w in want)       # not all of them flat
    header = ["label", "class", "pixels", "x0", "y0", "x1", "y1", "centroid_x", "centroid_y", "depth_pixels", "depth_max", "depth_mean", "volume",
              "depth_p50", "depth_p90"]
    with open(p("c.csv"), newline="") as f:
        rows = list(csv.reader(f))
    assert rows[0] == header and len(rows) == N + 1
    for row, w, label, k in zip(rows[1:], want, ref.zone.tolist(), ref.valid[0].tolist()):
        assert int(row[0]) == label and int(row[9]) == k
        assert {name: None if cell == "" else float(cell) for name, cell in zip(header[13:], row[13:])} == w
    with open(p("flood.geojson")) as f:
        written = json.load(f)
    assert len(written["features"]) == N
    for f, w in zip(written["features"], want):
        assert list(f["properties"]) == ["class", "pixels", "area", "centroid_x", "centroid_y", "depth_pixels", "depth_max", "depth_mean", "volume",
                                         "depth_p50", "depth_p90"]
        assert {k: f["properties"][k] for k in w} == w
    report = json.load(open(p("r.json")))
    water = np.isin(classes, (1, 2)).astype(np.uint8)
    whole = quantile_ref.zonal_quantiles(np.zeros(classes.shape, np.int32), np.ascontiguousarray(depth), (50, 90), water)
    assert whole.valid.tolist() == [[report["depth"]["with_depth"]]] and report["depth"]["with_depth"] > 0
    assert list(report["depth"]) == ["water_pixels", "with_depth", "max", "mean", "volume", "percentiles"]
    assert report["depth"]["percentiles"] == {"p50": float(quantile_ref.values(whole)[0, 0, 0]), "p90": float(quantile_ref.values(whole)[0, 1, 0])}
    assert report["depth"]["percentiles"]["p50"] <= report["depth"]["percentiles"]["p90"] <= report["depth"]["max"]
    # without the flag: the same files less the new columns, byte for byte
    again = subprocess.run(cmd + outputs("2"), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert again.returncode == 0, again.stdout + again.stderr
    assert open(p("flood2.tif"), "rb").read() == open(p("flood.tif"), "rb").read() and open(p("d2.tif"), "rb").read() == open(p("d.tif"), "rb").read()
    assert open(p("c2.csv")).read() == "".join(",".join(row[:13]) + "\n" for row in rows)
    for f in written["features"]:
        del f["properties"]["depth_p50"], f["properties"]["depth_p90"]
    assert open(p("flood2.geojson")).read() == json.dumps(written)
    del report["depth"]["percentiles"]
    assert open(p("r2.json")).read() == json.dumps(report, indent=1)
