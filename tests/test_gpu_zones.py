"""Zones from a vector layer on the device (csrc/zones.hip, kurosiwo_amd/scene.py: rasterize_zones; predict.py --zones) against
tests/zones_ref.py, equal bit for bit: random polygons that reach outside the scene, a third of them with vertices on pixel centres
and corners; horizontal and vertical edges through pixel centres; zero-area rings and repeated vertices; a polygon around the scene
and one outside it; overlapping features in both orders of the edge table; holes and multipolygons; crossing counts that end inside
a sort tile; one, two and three feature digits; spans of every length a wave treats differently; no edge and no crossing; the
inputs unchanged and two runs equal; the round trip through polygonize; zonal_stats on the result; argument errors; predict.py end
to end."""
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
import zones_ref
from kurosiwo_amd import _lib
from kurosiwo_amd.scene import MAX_ZONE_COORD, QUANTILE_TILE, label_components, polygonize, rasterize_zones, zonal_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((1, 1), (1, 130), (130, 1), (67, 133), (150, 300))
KINDS = ("random", "centres", "degenerate", "around", "holes")
C = 128                                                                        # the centre of pixel k is at 256 k + C


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _random_rings(rng, n, Hs, Ws, lo=3, hi=9, reach=20, size=None):
    """n polygons of lo .. hi - 1 vertices in 1/256 pixel that reach `reach` pixels outside the scene (or of at most `size` pixels
    around a random place); every third has its vertices snapped to half pixels: pixel centres and corners"""
    rings = []
    for i in range(n):
        k = int(rng.integers(lo, hi))
        if size is None:
            x = rng.integers(-reach * 256, (Ws + reach) * 256 + 1, size=k)
            y = rng.integers(-reach * 256, (Hs + reach) * 256 + 1, size=k)
        else:
            x = rng.integers(0, Ws * 256 + 1) + rng.integers(-size * 128, size * 128 + 1, size=k)
            y = rng.integers(0, Hs * 256 + 1) + rng.integers(-size * 128, size * 128 + 1, size=k)
        if i % 3 == 0:
            x, y = (x // 128) * 128, (y // 128) * 128
        rings.append([list(zip(x.tolist(), y.tolist()))])
    return rings


def _rect(x0, y0, x1, y1):
    return [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(edges int32 [E, 4], feature int32 [E], F) of one scene and kind, vertices in 1/256 pixel"""
    Hs, Ws = shape
    rng = np.random.default_rng(Hs * 1000 + Ws)
    if kind == "random":
        rings = _random_rings(rng, 12, Hs, Ws)
    elif kind == "centres":                                                    # horizontal and vertical edges through pixel centres
        rings = []
        for _ in range(8):
            x = np.sort(rng.integers(-2, Ws + 2, size=2)) * 256 + C
            y = np.sort(rng.integers(-2, Hs + 2, size=2)) * 256 + C
            rings.append([_rect(int(x[0]), int(y[0]), int(x[1]), int(y[1]))])
        x, y = (Ws // 2) * 256 + C, (Hs // 2) * 256 + C                        # an L and a staircase with every vertex on a centre
        rings.append([[(C, C), (x, C), (x, y), (x + 512, y), (x + 512, y + 256), (C, y + 256)]])
        rings.append([[(C, C), (C + 256, C), (C + 256, C + 256), (C + 512, C + 256), (C + 512, C + 512), (C, C + 512)]])
    elif kind == "degenerate":                                                 # zero-area rings, repeated vertices, a point
        a, b, c = (C, C), (Ws * 256 - C, Hs * 128), (Ws * 100, Hs * 256 + 700)
        rings = [[[a, b, a]], [[a, b, c, b]], [[a, a, b, b, c, c, c]], [[b, b, b]], [[a, c]], [_rect(300, 40, 300, Hs * 256 + 9)],
                 [[(0, 0), (Ws * 256, 0), (Ws * 256, Hs * 256), (0, Hs * 256), (0, 0), (Ws * 256, 0)]]]
    elif kind == "around":                                                     # one wholly outside, one around the whole scene
        far = MAX_ZONE_COORD
        rings = [[_rect(-5000, -5000, -300, Hs * 256 + 5000)], [_rect(Ws * 256 + 1, 0, Ws * 256 + 900, Hs * 256)],
                 [_rect(-far, -far, far, far)], [_rect(-256, -256, Ws * 256 + 256, Hs * 256 + 256)]]
    elif kind == "holes":                                                      # holes, a part in a hole, parts apart: a multipolygon
        W, H = Ws * 256, Hs * 256
        rings = [[_rect(W // 10, H // 10, W - W // 10, H - H // 10), _rect(W // 5, H // 5, W - W // 5, H - H // 5)[::-1],
                  _rect(W // 3, H // 3, W - W // 3, H - H // 3), [(W // 2 - 90, H // 2 - 70), (W // 2 + 111, H // 2), (W // 2, H // 2 + 95)]],
                 [_rect(-700, -700, W // 2, H // 2), _rect(W // 2 + 300, H // 2 + 300, W + 4000, H + 4000)]] + _random_rings(rng, 3, Hs, Ws)
    edges, feature = zones_ref.ring_edges(rings, scale=1)
    return edges, feature, len(rings)


def _check(edges, feature, shape, F, what):
    """rasterize_zones on the device against the reference, as bits; count=None gives the same; the inputs unchanged; two runs equal
    -> (the reference, the number of crossings)"""
    Hs, Ws = shape
    want = zones_ref.rasterize(edges, feature, Hs, Ws)
    X = zones_ref.crossings(edges, feature, Hs, Ws).size
    e, f = _dev(edges), _dev(feature)
    got = rasterize_zones(e, f, Hs, Ws, count=F)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == shape and got.is_contiguous()
    differ = int((got.cpu().numpy() != want).sum())
    print(f"{what}: {edges.shape[0]} edges, {F} features, {X} crossings, {int((want >= 0).sum())} of {want.size} pixels in a zone; "
          f"pixels that differ: {differ}")
    assert differ == 0
    assert torch.equal(e.cpu(), torch.from_numpy(edges)) and torch.equal(f.cpu(), torch.from_numpy(feature))
    assert torch.equal(rasterize_zones(e, f, Hs, Ws, count=F), got)
    if edges.shape[0]:
        assert torch.equal(rasterize_zones(e, f, Hs, Ws), got)                 # the count read from the table
    return want, X


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_zones_equal_the_reference(shape, kind):
    edges, feature, F = _case(shape, kind)
    want, X = _check(edges, feature, shape, F, f"{shape} {kind}")
    if kind == "around":
        assert (want == 2).all()                                               # the two outside own nothing, the first around wins
    if kind in ("random", "holes") and shape[0] * shape[1] > 1:
        assert (want >= 0).any() and X > 0
    if kind == "holes" and shape == (150, 300):
        assert set(np.unique(want).tolist()) >= {-1, 0, 1}
        # the part inside the hole, the ring; in the hole the next feature shows: its first part, its second
        assert want[75, 150] == 0 and want[20, 150] == 0 and want[60, 70] == 1 and want[110, 230] == 1


def test_the_lowest_feature_wins_in_both_orders_of_the_edge_table():
    shape = (67, 133)
    rng = np.random.default_rng(5)
    rings = _random_rings(rng, 9, *shape, reach=5)
    edges, feature = zones_ref.ring_edges(rings, scale=1)
    want, _ = _check(edges, feature, shape, 9, "overlapping")
    back, _ = _check(np.ascontiguousarray(edges[::-1]), np.ascontiguousarray(feature[::-1]), shape, 9, "overlapping, the table reversed")
    mixed = rng.permutation(edges.shape[0])
    _check(np.ascontiguousarray(edges[mixed]), np.ascontiguousarray(feature[mixed]), shape, 9, "overlapping, the table shuffled")
    assert np.array_equal(want, back)
    alone = [zones_ref.rasterize(edges[feature == i], np.zeros(int((feature == i).sum()), np.int32), *shape) >= 0 for i in range(9)]
    assert (np.sum(alone, axis=0) > 1).sum() > 500                             # they do overlap
    first = np.where(np.any(alone, axis=0), np.argmax(alone, axis=0), -1)
    assert np.array_equal(want, first)


def test_more_crossings_than_a_sort_tile_ending_inside_one():
    shape = (150, 300)
    edges, feature = zones_ref.ring_edges(_random_rings(np.random.default_rng(40), 40, *shape), scale=1)
    _, X = _check(edges, feature, shape, 40, "40 polygons")
    assert X > QUANTILE_TILE and X % QUANTILE_TILE


def test_two_feature_digits():
    shape = (150, 300)
    rings = _random_rings(np.random.default_rng(300), 300, *shape, size=40)
    rings[7], rings[256], rings[299] = [], [], [_rect(C, C, 40 * 256, 30 * 256)]       # features without a ring keep their index
    edges, feature = zones_ref.ring_edges(rings, scale=1)
    want, X = _check(edges, feature, shape, 300, "F = 300")
    assert _lib.load().ksmi_scene_quantile_passes(300) == 6 and (want > 256).any() and want.max() == 299 and X > 300


def test_three_feature_digits_unit_squares():
    """F = 70 000 unit squares on 300 x 300, each around one pixel centre of a shuffled list, every 11th feature without a ring; X is
    about twice F here, and a table of 1000 squares with count = 70 000 has fewer composites than rows: the padded sort"""
    shape, F = (300, 300), 70000
    rng = np.random.default_rng(70)
    place = rng.permutation(300 * 300)[:F]
    x0 = (place % 300) * 256 + rng.integers(-127, 128, size=F)
    y0 = (place // 300) * 256 + rng.integers(-127, 128, size=F)
    keep = np.arange(F) % 11 != 3
    quad = np.stack((x0, y0, x0 + 256, y0, x0 + 256, y0 + 256, x0, y0 + 256), axis=1).reshape(F, 4, 2)[keep]
    edges = np.concatenate((quad, np.roll(quad, -1, axis=1)), axis=2).reshape(-1, 4).astype(np.int32)
    feature = np.repeat(np.arange(F)[keep], 4).astype(np.int32)
    want, X = _check(edges, feature, shape, F, "F = 70000")
    assert _lib.load().ksmi_scene_quantile_passes(F) == 7 and want.max() > 65536 and X > F
    assert np.array_equal(np.bincount(want[want >= 0], minlength=F), keep.astype(np.int64))    # one pixel each
    few = np.flatnonzero(keep)[-1000:]
    some = np.isin(feature, few)
    want, X = _check(np.ascontiguousarray(edges[some]), np.ascontiguousarray(feature[some]), shape, F, "F = 70000, 1000 squares")
    assert X == 2000 and (want >= 0).sum() == 1000


@pytest.mark.parametrize("shape", ((67, 133), (150, 300)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_spans_of_every_length_a_wave_treats_differently(shape):
    Hs, Ws = shape
    lengths = (0, 1, 63, 64, 65, 127, 128, 129, Ws)
    rings = []
    for row, n in enumerate(lengths):                                          # row 2 * row + 1, columns 3 .. 3 + n - 1
        y = (2 * row + 1) * 256
        rings.append([_rect(3 * 256 + C, y, (3 + n) * 256 + C, y + 256)] if n < Ws else [_rect(-2560, y, Ws * 256 + 2560, y + 256)])
    edges, feature = zones_ref.ring_edges(rings, scale=1)
    f, y, c0, c1 = zones_ref.spans(zones_ref.crossings(edges, feature, Hs, Ws))
    assert (c1 - c0).tolist() == list(lengths) and y.tolist() == [2 * r + 1 for r in range(len(lengths))]
    want, _ = _check(edges, feature, shape, len(lengths), f"{shape} span lengths")
    assert np.bincount(want[want >= 0], minlength=len(lengths)).tolist() == list(lengths)


def test_no_edge_and_no_crossing_give_a_raster_of_minus_one():
    none = (np.empty((0, 4), np.int32), np.empty(0, np.int32))
    flat = zones_ref.ring_edges([[[(0, 300), (5000, 300), (900, 300)]], [_rect(-900, -900, -300, -300)]], scale=1)      # horizontal; outside
    for shape in ((9, 70), (1, 1)):
        for (edges, feature), F in ((none, 0), (none, 5), (flat, 2)):
            want, X = _check(edges, feature, shape, F, f"{shape} nothing to draw")
            assert X == 0 and (want == -1).all()
    for shape in ((0, 5), (5, 0)):
        got = rasterize_zones(_dev(flat[0]), _dev(flat[1]), *shape)
        assert tuple(got.shape) == shape and got.dtype == torch.int32


@functools.lru_cache(maxsize=None)
def _class_map(shape):
    return np.ascontiguousarray(sieve_ref.speckle_scene(shape[0] + shape[1], *shape))


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_rings_of_polygonize_rasterise_back_to_the_components(shape):
    classes = _class_map(shape)
    c = _dev(classes)
    rings = polygonize(c)
    label, start, verts = (t.cpu().numpy() for t in (rings.label, rings.start, rings.verts))
    edges, feature, labels = zones_ref.edges_of_rings(label, start, verts)
    got = rasterize_zones(_dev(edges), _dev(feature), *shape, count=int(labels.size))
    lab = label_components(c, 4)
    chosen = torch.from_numpy(polygon_ref.selected(classes, (1, 2))).cuda()
    rank = torch.searchsorted(torch.from_numpy(labels).cuda(), lab.to(torch.int64))
    want = torch.where(chosen, rank, torch.full_like(rank, -1)).to(torch.int32)
    print(f"{shape}: {labels.size} components, {edges.shape[0]} edges")
    assert labels.size >= 1 and torch.equal(got, want)
    assert np.array_equal(got.cpu().numpy(), zones_ref.rasterize(edges, feature, *shape))


def test_zonal_stats_counts_the_pixels_of_every_feature():
    shape = (150, 300)
    edges, feature, F = _case(shape, "random")
    want = zones_ref.rasterize(edges, feature, *shape)
    stats = zonal_stats(rasterize_zones(_dev(edges), _dev(feature), *shape, count=F))
    counts = np.bincount(want[want >= 0], minlength=F)
    assert stats.zone.cpu().numpy().tolist() == np.flatnonzero(counts).tolist()
    assert stats.count.cpu().numpy().tolist() == counts[counts > 0].tolist() and counts.sum() > 1000


def test_what_is_no_vector_layer_is_refused():
    edges, feature, F = _case((67, 133), "random")
    e, f = _dev(edges), _dev(feature)
    # a triangle whose first edge crosses the five scanlines 0 .. 4: without it the number of crossings is odd
    open_ring = zones_ref.ring_edges([[[(C, C), (20 * 256, 5 * 256), (10 * 256, 30 * 256 + 7)]]], scale=1)[0][1:]
    assert zones_ref.crossings(open_ring, np.zeros(2, np.int32), 67, 133).size % 2 == 1
    for bad in (lambda: rasterize_zones(e, f, 67, 32768), lambda: rasterize_zones(e, f, -1, 5), lambda: rasterize_zones(e, f[:-1], 67, 133),
                lambda: rasterize_zones(e.to(torch.int64), f, 67, 133), lambda: rasterize_zones(e, f, 67, 133, count=-1),
                lambda: rasterize_zones(e, f, 67, 133, count=F - 1),                              # a feature outside 0 .. F - 2
                lambda: rasterize_zones(_dev(open_ring), _dev(np.zeros(2, np.int32)), 67, 133),           # a ring left open
                lambda: rasterize_zones(_dev(np.array([[0, 0, MAX_ZONE_COORD + 1, 9], [MAX_ZONE_COORD + 1, 9, 0, 0]], np.int32)),
                                        _dev(np.zeros(2, np.int32)), 67, 133),
                lambda: rasterize_zones(e, _dev(np.where(np.arange(feature.size) == 3, -1, feature).astype(np.int32)), 67, 133, count=F)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError):
        rasterize_zones(torch.from_numpy(edges), torch.from_numpy(feature), 67, 133)


def test_argument_errors_return_e_arg_and_launch_nothing():
    lib = _lib.load()
    E_ARG = -1                                                                 # KSMI_E_ARG of include/ksmi.h
    edges, feature, F = _case((67, 133), "random")
    e, f = _dev(edges), _dev(feature)
    E = edges.shape[0]
    counts = torch.full((E,), 77, dtype=torch.int32, device="cuda")
    info = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    keys = torch.full((64,), 77, dtype=torch.int64, device="cuda")
    zones = torch.full((67, 133), 77, dtype=torch.int32, device="cuda")
    p = lambda t: t.data_ptr()
    rows = [(None, p(f), E, F, 67, 133, p(counts), p(info)), (p(e), None, E, F, 67, 133, p(counts), p(info)),
            (p(e), p(f), E, F, 67, 133, None, p(info)), (p(e), p(f), E, F, 67, 133, p(counts), None), (p(e), p(f), 0, F, 67, 133, p(counts), None),
            (p(e), p(f), -1, F, 67, 133, p(counts), p(info)), (p(e), p(f), 2 ** 31, F, 67, 133, p(counts), p(info)),
            (p(e), p(f), E, -1, 67, 133, p(counts), p(info)), (p(e), p(f), E, 2 ** 31, 67, 133, p(counts), p(info)),
            (p(e), p(f), E, F, 32768, 133, p(counts), p(info)), (p(e), p(f), E, F, 67, -1, p(counts), p(info)),
            (p(e) + 4, p(f), E - 1, F, 67, 133, p(counts), p(info))]
    for args in rows:
        assert lib.ksmi_scene_zone_rows(*args, None) == E_ARG, args
    cross = [(None, p(f), p(counts), E, 10, 67, 133, p(keys), 64), (p(e), None, p(counts), E, 10, 67, 133, p(keys), 64),
             (p(e), p(f), None, E, 10, 67, 133, p(keys), 64), (p(e), p(f), p(counts), E, 10, 67, 133, None, 64),
             (p(e), p(f), p(counts), E, -1, 67, 133, p(keys), 64), (p(e), p(f), p(counts), E, 65, 67, 133, p(keys), 64),
             (p(e), p(f), p(counts), 0, 10, 67, 133, p(keys), 64), (p(e), p(f), p(counts), E, 10, 67, 133, p(keys), 2 ** 31),
             (p(e), p(f), p(counts), -1, 10, 67, 133, p(keys), 64), (p(e), p(f), p(counts), E, 10, 67, 40000, p(keys), 64),
             (p(e) + 8, p(f), p(counts), E - 1, 10, 67, 133, p(keys), 64)]
    for args in cross:
        assert lib.ksmi_scene_zone_crossings(*args, None) == E_ARG, args
    fill = [(None, 10, F, 67, 133, p(zones)), (p(keys), 10, F, 67, 133, None), (p(keys), 11, F, 67, 133, p(zones)),
            (p(keys), -2, F, 67, 133, p(zones)), (p(keys), 2 ** 31, F, 67, 133, p(zones)), (p(keys), 10, -1, 67, 133, p(zones)),
            (p(keys), 10, F, 32768, 133, p(zones)), (p(keys), 10, F, 67, -3, p(zones))]
    for args in fill:
        assert lib.ksmi_scene_zone_fill(*args, None) == E_ARG, args
    assert b"scene_zone_fill" in lib.ksmi_last_error()
    torch.cuda.synchronize()
    for t in (counts, info, keys, zones):
        assert (t == 77).all()                                                 # nothing was launched
    assert lib.ksmi_scene_zone_crossings(None, None, None, 0, 0, 67, 133, None, 0, None) == 0          # the no-ops
    assert lib.ksmi_scene_zone_fill(None, 0, 0, 0, 133, None, None) == 0
    assert lib.ksmi_scene_zone_rows(None, None, 0, 0, 67, 133, None, p(info), None) == 0 and info.tolist() == [0, 0]
    assert lib.ksmi_scene_zone_fill(None, 0, F, 67, 133, p(zones), None) == 0 and (zones == -1).all()
    # sorted pairs that are no span of the scene address nothing
    junk = _dev(np.array([(1 << 32) | (5 << 16) | 7, (1 << 32) | (6 << 16) | 9, (1 << 32) | (70 << 16) | 1, (1 << 32) | (70 << 16) | 9,
                          (2 << 32) | (5 << 16) | 100, (2 << 32) | (5 << 16) | 140, (900 << 32) | (5 << 16) | 1, (900 << 32) | (5 << 16) | 9,
                          (3 << 32) | (8 << 16) | 20, (3 << 32) | (8 << 16) | 10, (4 << 32) | (9 << 16) | 2, (4 << 32) | (9 << 16) | 4], np.int64))
    assert lib.ksmi_scene_zone_fill(p(junk), 12, 10, 67, 133, p(zones), None) == 0
    want = np.full((67, 133), -1, np.int32)
    want[9, 2:4] = 4
    assert np.array_equal(zones.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------- predict.py
def _tiny_scene(tmp_path):
    """a tiny SNUNet checkpoint, georeferenced rasters and a raw DEM, as tests/test_gpu_quantile.py builds its own"""
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
    return geo, [sys.executable, os.path.join(ROOT, "predict.py"), "--task", "cd", "--method", "snunet", "--checkpoint", str(tmp_path / "best.pt"),
                 "--post", str(tmp_path / "post_vv.tif"), str(tmp_path / "post_vh.tif"), "--pre1", str(tmp_path / "pre.tif"),
                 "--window", "32", "--stride", "16", "--batch_size", "5", "--precision", "fp32"]


def test_predict_script_with_zones(tmp_path):
    from kurosiwo_amd import geotiff
    geo, cmd = _tiny_scene(tmp_path)
    Hs, Ws = 80, 72
    (sx, sy), (ox, oy) = geo["pixel_scale"], geo["origin"]
    box = lambda x0, y0, x1, y1: [[ox + x * sx, oy - y * sy] for x, y in ((x0, y0), (x1, y0), (x1, y1), (x0, y1), (x0, y0))]      # pixels -> map, closed
    # two rectangles that split the scene along the line through the centres of column 30, one feature over both (first in the file:
    # it wins its pixels), one outside the scene and a Point
    rings = [("over", "Polygon", [box(20, 10, 50, 40.5)]), ("west", "Polygon", [box(-5, -5, 30.5, 85)]),
             ("east", "MultiPolygon", [[box(30.5, -5, 80, 85)]]), ("away", "Polygon", [box(100, 100, 140, 130)]), ("pin", "Point", [ox + 5.0, oy - 5.0])]
    layer = {"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"name": n}, "geometry": {"type": t, "coordinates": c}}
                                                       for n, t, c in rings]}
    p = lambda name: str(tmp_path / name)
    with open(p("districts.geojson"), "w") as f:
        json.dump(layer, f)
    outputs = lambda tag: ["--out", p(f"flood{tag}.tif"), "--mmu", "6", "--polygons", p(f"flood{tag}.geojson"), "--depth_out", p(f"d{tag}.tif"),
                           "--depth_dem", p("dem.tif"), "--components", p(f"c{tag}.csv"), "--report", p(f"r{tag}.json"), "--percentiles", "50", "90"]
    run = subprocess.run(cmd + outputs("") + ["--zones", p("districts.geojson"), "--zone_key", "name", "--zones_out", p("z.csv"), "--zones_raster",
                                              p("z.tif")], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    classes, _ = geotiff.read(p("flood.tif"))
    depth, _ = geotiff.read(p("d.tif"))
    features = [[box(20, 10, 50, 40.5)], [box(-5, -5, 30.5, 85)], [box(30.5, -5, 80, 85)], [box(100, 100, 140, 130)], []]
    edges, feature, F = zones_ref.zone_edges(features, Hs, Ws, **geo)
    zones = zones_ref.rasterize(edges, feature, Hs, Ws)
    assert F == 5 and (zones[:, :30] != 2).all() and (zones[:, 30:] != 1).all() and (zones[10:40, 20:50] == 0).all() and (zones >= 0).all()
    raster, meta = geotiff.read(p("z.tif"))
    assert raster.dtype == np.int32 and np.array_equal(raster, zones) and meta["nodata"] == -1
    want, report = zones_ref.zones_table(zones, ["over", "west", "east", "away", "pin"], classes, (1, 2), sx * sy, depth, (1, 2), (50, 90))
    with open(p("z.csv"), newline="") as f:
        rows = list(csv.reader(f))
    print("predict.py --zones:", *rows[:4], sep="\n  ")
    assert rows[0] == ["zone", "id", "pixels", "valid", "class_0", "class_1", "class_2", "class_3", "flooded", "flooded_area", "flooded_fraction",
                       "depth_pixels", "depth_max", "depth_mean", "volume", "depth_p50", "depth_p90"]
    assert rows == want and len(rows) == 6
    assert [int(r[2]) for r in rows[1:]] == [900, 30 * 80 - 300, 42 * 80 - 600, 0, 0] and rows[4][9:] == ["0.0", "", "0", "", "", "0.0", "", ""]
    assert sum(int(r[8]) for r in rows[1:]) == int(np.isin(classes, (1, 2)).sum()) > 0 and any(r[15] != "" for r in rows[1:4])
    written = json.load(open(p("r.json")))
    assert written["zones"] == report == {"features": 5, "with_pixels": 3, "pixels": Hs * Ws} and list(written)[-1] == "zones"
    # without --zones: every other file has the bytes it had
    again = subprocess.run(cmd + outputs("2"), cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert again.returncode == 0, again.stdout + again.stderr
    for a, b in (("flood.tif", "flood2.tif"), ("d.tif", "d2.tif"), ("c.csv", "c2.csv"), ("flood.geojson", "flood2.geojson")):
        assert open(p(a), "rb").read() == open(p(b), "rb").read(), a
    del written["zones"]
    assert open(p("r2.json")).read() == json.dumps(written, indent=1)
