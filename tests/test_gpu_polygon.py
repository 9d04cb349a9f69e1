"""Polygon output on the device (csrc/polygon.hip, kurosiwo_amd/scene.py: scan_i32, boundary_edges, trace_rings, polygonize,
polygons_geojson; predict.py --polygons) against the sequential walk of tests/polygon_ref.py: the scan on the sizes around its tile
and its recursion depths, then edge ids, successors, ring minima, ranks and the ring table, all equal bit for bit, on maps placed on
the edges of the scan tile and the label tile, on the structured maps that stress the walk (one ring around everything, a checkerboard
of saddles, a saddle within one label, an island in a hole, serpentines whose one ring is 2^k - 2, 2^k and 2^k + 2 edges long) and on
speckled scenes; single cycles of 2^k - 1, 2^k and 2^k + 1 edges through trace_rings; two runs give equal bits; invariants 2 and 3
from the device's own output; predict.py --mmu --polygons end to end."""
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
from kurosiwo_amd.scene import (LABEL_TILE, SCAN_TILE, Rings, boundary_edges, component_sizes, label_components, polygonize, polygons_geojson,
                                scan_i32, trace_rings)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = SCAN_TILE
SELECTS = ((1,), (1, 2), (0, 1, 2, 3))
# the three scenes of tests/test_gpu_sieve.py (seeds and shapes copied), and one whose pixels and edges both exceed a scan tile
SPECKLE = {"speckle65x129": (5, 65, 129), "speckle96x96": (2, 96, 96), "speckle130x67": (3, 130, 67), "speckle257x513": (7, 257, 513)}
SERPENTINE_K = 9                                   # rings of 2^9 - 2, 2^9 and 2^9 + 2 edges


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------- the scan
@functools.lru_cache(maxsize=None)
def _scan_input(n, kind):
    x = np.full(n, 4, np.int32) if kind == "all4" else np.random.default_rng(n).integers(0, 5, size=n, dtype=np.int32)
    c = np.cumsum(x, dtype=np.int64)
    return x, (c - x).astype(np.int32), int(c[-1])


@pytest.mark.parametrize("kind", ("random", "all4"))
@pytest.mark.parametrize("n", (1, T - 1, T, T + 1, 2 * T + 1, T * T - 1, T * T, T * T + 1))
def test_scan(n, kind):
    """T * T + 1 is the smallest n that needs three levels; every prefix stays below 2^31 (4 * (T * T + 1) < 2^25)"""
    assert T <= 4096 and T * T + 1 <= 16_800_000
    x, want, want_total = _scan_input(n, kind)
    d = _dev(x)
    out, total = scan_i32(d)
    assert out.dtype == torch.int32 and total.dtype == torch.int64 and total.numel() == 1 and out.data_ptr() != d.data_ptr()
    assert torch.equal(d.cpu(), torch.from_numpy(x))                             # the input is left alone
    bad = int((out.cpu().numpy() != want).sum())
    print(f"scan n = {n} ({kind}): {bad} prefixes differ; total {int(total.item())} (numpy {want_total})")
    assert bad == 0 and int(total.item()) == want_total
    again, total2 = scan_i32(d)                                                  # two runs, equal bits
    assert torch.equal(again, out) and torch.equal(total2, total)
    same, total3 = scan_i32(d, out=d)                                            # in place
    assert same.data_ptr() == d.data_ptr() and torch.equal(d, out) and int(total3.item()) == want_total


def test_scan_of_nothing():
    out, total = scan_i32(torch.empty(0, dtype=torch.int32, device="cuda"))
    assert out.numel() == 0 and int(total.item()) == 0


# ---------------------------------------------------------------------------------------------------- the maps
def _snake(W):
    """the pixels of a one-pixel path in walking order: every second row end to end, joined alternately right and left"""
    y = 0
    while True:
        xs = range(W) if (y // 2) % 2 == 0 else range(W - 1, -1, -1)
        for x in xs:
            yield y, x
        yield y + 1, (W - 1 if (y // 2) % 2 == 0 else 0)
        y += 2


def _serpentine(pixels, W):
    """a path of `pixels` pixels: a tree-like shape, so its one ring has 4 * pixels - 2 * (pixels - 1) = 2 * pixels + 2 edges"""
    pts = [p for p, _ in zip(_snake(W), range(pixels))]
    m = np.zeros((max(y for y, _ in pts) + 2, W), np.uint8)
    for y, x in pts:
        m[y, x] = 1
    return m


@functools.lru_cache(maxsize=None)
def _scene(name):
    """the map of a case, built once"""
    th, tw = LABEL_TILE
    if name in SPECKLE:
        return sieve_ref.speckle_scene(*SPECKLE[name])
    if name == "1x1":
        return np.ones((1, 1), np.uint8)
    if name == "row":                                               # 1 x W and H x 1 across a scan tile
        return np.random.default_rng(11).integers(0, 3, size=(1, T + 37), dtype=np.uint8)
    if name == "column":
        return np.random.default_rng(12).integers(0, 3, size=(T + 37, 1), dtype=np.uint8)
    if name.startswith("corner"):                                   # one selected pixel in one corner of the map
        m = np.zeros((5, 7), np.uint8)
        m[{"0": 0, "1": 0, "2": 4, "3": 4}[name[-1]], {"0": 0, "1": 6, "2": 0, "3": 6}[name[-1]]] = 1
        return m
    if name == "one_class":
        return np.full((2 * th + 1, 2 * tw + 2), 1, np.uint8)
    if name == "checkerboard":
        yy, xx = np.mgrid[0:2 * th + 1, 0:2 * tw + 1]
        return ((yy + xx) & 1).astype(np.uint8)
    if name == "cut_ring":
        m = np.ones((3, 3), np.uint8)
        m[1, 1] = m[0, 0] = 0
        return m
    if name == "nested":                                            # squares inside squares: an island sits in a hole
        yy, xx = np.mgrid[0:11, 0:13]
        depth = np.minimum(np.minimum(yy, 10 - yy), np.minimum(xx, 12 - xx))
        return (1 - (depth & 1)).astype(np.uint8)
    if name == "donut":                                             # across the borders of the label tile, both ways
        m = np.zeros((2 * th + 8, 2 * tw + 22), np.uint8)
        m[3:2 * th + 5, 5:2 * tw + 17] = 2
        m[th - 6:th + 14, 20:2 * tw + 2] = 0
        return m
    if name.startswith("serpentine"):
        edges = (1 << SERPENTINE_K) + int(name[len("serpentine"):])
        return _serpentine((edges - 2) // 2, LABEL_TILE[1] + 6)
    raise KeyError(name)


MAPS = ("1x1", "row", "column", "corner0", "corner1", "corner2", "corner3", "one_class", "checkerboard", "cut_ring", "nested", "donut",
        "serpentine-2", "serpentine+0", "serpentine+2") + tuple(sorted(SPECKLE))


@functools.lru_cache(maxsize=None)
def _want(name, select):
    m = _scene(name)
    tr = polygon_ref.trace(m, select)
    return tr, polygon_ref.rings(m, select, tr)


def _run(m, select):
    """everything the device computes for a map, as numpy: eid, succ, ring_min, rank and the ring table"""
    d = _dev(m)
    lab = label_components(d, 4)
    eid, succ = boundary_edges(d, lab, select)
    ring_min, rank = trace_rings(succ)
    r = polygonize(d, select)
    r2 = polygonize(d, select, labels=lab)
    assert isinstance(r, Rings) and all(torch.equal(a, b) for a, b in zip(r, r2))
    assert [t.dtype for t in r] == [torch.int32, torch.int32, torch.int32, torch.int64, torch.int32] and all(t.is_cuda for t in r)
    assert r.verts.dim() == 2 and r.verts.shape[1] == 2 and r.start.numel() == r.label.numel() + 1 == r.ring_id.numel() + 1 == r.area2.numel() + 1
    assert torch.equal(d.cpu(), torch.from_numpy(m))                # the input is left alone
    return [t.cpu().numpy() for t in (eid, succ, ring_min, rank) + tuple(r)]


NAMES = ("eid", "succ", "ring_min", "rank", "label", "ring_id", "start", "area2", "verts")


def _check(name, select):
    m = _scene(name)
    tr, want = _want(name, select)
    first, second = _run(m, select), _run(m, select)
    bad = {}
    for key, got, ref in zip(NAMES, first, tuple(tr) + tuple(want)):
        assert got.dtype == ref.dtype, key
        bad[key] = -1 if got.shape != ref.shape else int((got != ref).sum())
    lengths = np.bincount(tr.ring_min, minlength=1)
    print(f"{name} {m.shape} select {select}: E {len(tr.eid)}, R {len(want.label)}, V {len(want.verts)}, longest ring "
          f"{int(lengths.max())} edges; cells that differ: {bad}")
    assert not any(bad.values())
    for a, b in zip(first, second):                                 # two runs, equal bits
        assert np.array_equal(a, b)
    return Rings(*first[4:]), tr


@pytest.mark.parametrize("select", SELECTS, ids=lambda s: "select" + "".join(map(str, s)))
@pytest.mark.parametrize("name", MAPS)
def test_edges_rings_and_polygons(name, select):
    m = _scene(name)
    H, W = m.shape
    r, tr = _check(name, select)
    if name == "row" or name == "column":
        assert H * W > T and (H == 1 or W == 1)
    if name.startswith("corner"):
        assert (m == 1).sum() == 1 and (0 in select or (r.area2.tolist() == [2] and r.ring_id.tolist() == [4 * int(np.flatnonzero(m)[0])]))
    if name == "one_class":                                         # one ring around everything
        assert len(tr.eid) == 2 * (H + W) and r.ring_id.tolist() == [0] and r.area2.tolist() == [2 * H * W]
        assert r.verts.tolist() == [[W, 0], [W, H], [0, H], [0, 0]]
    if name == "checkerboard":                                      # saddles between different labels everywhere: nobody crosses over
        n = int(polygon_ref.selected(m, select).sum())
        assert len(r.label) == n and (np.bincount(tr.ring_min)[tr.ring_min] == 4).all() and (r.area2 == 2).all()
    if name == "cut_ring":                                          # a saddle within one label: both rings cross over at (1, 1)
        assert r.ring_id.tolist()[:2] == ([4, 6] if 0 not in select else [0, 4])
        if 0 not in select:
            assert r.area2.tolist() == [16, -2] and [1, 1] in r.verts[:6].tolist() and [1, 1] in r.verts[6:].tolist()
    if name == "nested" and 0 in select:
        assert (r.area2 < 0).sum() == 5 and len(r.label) == 6 + 5   # six squares, the five outer ones with a hole
    if name == "donut" and 2 in select:
        th, tw = LABEL_TILE
        assert H > 2 * th and W > 2 * tw and (r.area2 < 0).sum() == (2 if 0 in select else 1)
    if name.startswith("serpentine"):                               # rank and minimum over one long cycle, around a power of two
        want = (1 << SERPENTINE_K) + int(name[len("serpentine"):])
        assert len(tr.eid) == want or 0 in select
        if 0 not in select:
            assert np.array_equal(np.sort(tr.rank), np.arange(want)) and not tr.ring_min.any()
    if name == "speckle257x513":
        assert H * W > T and len(tr.eid) > T and len(r.label) > T // 4


def test_serpentine_lengths():
    """a closed walk on the grid has an even number of edges, so the rings of a map come in 2^k - 2, 2^k and 2^k + 2; the odd
    neighbours of the power of two are met by test_single_cycles below"""
    k = SERPENTINE_K
    assert k >= 8
    got = [len(_want(f"serpentine{d:+d}", (1,))[0].eid) for d in (-2, 0, 2)]
    print("serpentine ring lengths:", got)
    assert got == [(1 << k) - 2, 1 << k, (1 << k) + 2]
    for d in (-2, 0, 2):
        assert len(_want(f"serpentine{d:+d}", (1,))[1].label) == 1


@pytest.mark.parametrize("n", (1, 2, 3, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097))
def test_single_cycles(n):
    """one cycle through all n edges in a shuffled order, and the same cycle next to a second one: what pointer doubling can get wrong
    sits at n = 2^k and 2^k +- 1 (the round count, the last doubling step, the cut at the smallest edge)"""
    rng = np.random.default_rng(n)
    for extra in (0, 5):
        order = rng.permutation(n + extra)
        cycles = [order[:n]] + ([order[n:]] if extra else [])
        succ, ring_min, rank = (np.empty(n + extra, np.int32) for _ in range(3))
        for c in cycles:
            c = np.roll(c, -int(np.argmin(c)))                      # from its smallest edge
            succ[c] = np.roll(c, -1)
            ring_min[c] = c[0]
            rank[c] = np.arange(len(c))
        got_min, got_rank = trace_rings(_dev(succ))
        assert np.array_equal(got_min.cpu().numpy(), ring_min) and np.array_equal(got_rank.cpu().numpy(), rank), (n, extra)


def test_empty_selections():
    d = _dev(_scene("speckle96x96"))
    none3 = _dev(np.where(_scene("speckle96x96") == 3, 0, _scene("speckle96x96")).astype(np.uint8))
    for r in (polygonize(d, ()), polygonize(none3, (3,)), polygonize(none3, (62,)), polygonize(torch.empty((0, 5), dtype=torch.uint8, device="cuda"))):
        assert isinstance(r, Rings) and all(t.is_cuda for t in r)
        assert r.label.numel() == r.ring_id.numel() == r.area2.numel() == 0 and r.verts.shape == (0, 2) and r.start.tolist() == [0]
        assert [t.dtype for t in r] == [torch.int32, torch.int32, torch.int32, torch.int64, torch.int32]
        assert polygons_geojson(r, d) == {"type": "FeatureCollection", "features": []}
    eid, succ = boundary_edges(d, label_components(d, 4), ())
    assert eid.numel() == succ.numel() == 0 and all(t.numel() == 0 for t in trace_rings(succ))


@pytest.mark.parametrize("name", ("speckle257x513", "nested", "donut", "cut_ring", "checkerboard"))
def test_invariants_from_the_device_output_alone(name):
    """2: every selected component has one ring of positive area2, with id 4 * label, the smallest id of its rings, and every other
    ring has a negative one; 3: a component's area2 sum to twice its pixel count -- against component_sizes, without the oracle"""
    d = _dev(_scene(name))
    select = (0, 1, 2)
    lab = label_components(d, 4)
    size = component_sizes(lab).flatten().long()
    r = polygonize(d, select, labels=lab)
    label, ring_id = r.label.long(), r.ring_id.long()
    assert bool((ring_id[1:] > ring_id[:-1]).all()) and bool((r.area2 != 0).all())
    exterior = r.area2 > 0
    roots = torch.nonzero((lab.flatten() == torch.arange(lab.numel(), device="cuda")) & (d.flatten() <= 2)).flatten()
    assert torch.equal(label[exterior], roots)                     # one each, in ascending order
    assert torch.equal(ring_id[exterior], 4 * roots)
    first = torch.full((lab.numel(),), 2 ** 40, dtype=torch.int64, device="cuda").scatter_reduce(0, label, ring_id, "amin")
    assert torch.equal(first[roots], 4 * roots)                    # the exterior has the smallest id of its component
    twice = torch.zeros(lab.numel(), dtype=torch.int64, device="cuda").index_add_(0, label, r.area2)
    assert torch.equal(twice, 2 * size * (d.flatten() <= 2))
    assert int(r.start[-1]) == r.verts.shape[0] and bool((r.start[1:] - r.start[:-1] >= 4).all())


def test_wrappers_refuse_bad_shapes_and_dtypes():
    m, lab, v = (torch.zeros(s, dtype=t, device="cuda") for s, t in (((4, 4), torch.uint8), ((4, 4), torch.int32), ((8,), torch.int32)))
    for bad in (lambda: polygonize(m.int()), lambda: polygonize(m[:, ::2]), lambda: polygonize(m[0]), lambda: polygonize(m, labels=lab.long()),
                lambda: polygonize(m, labels=lab[:2]), lambda: boundary_edges(m, None), lambda: boundary_edges(m, lab.float()),
                lambda: trace_rings(v.long()), lambda: trace_rings(v.view(2, 4)), lambda: scan_i32(v.long()), lambda: scan_i32(v[::2]),
                lambda: scan_i32(v, out=v[:4]), lambda: polygonize(m, (63,))):
        with pytest.raises(ValueError):
            bad()


# ---------------------------------------------------------------------------------------------------- predict.py
def _tiny_scene(tmp_path):
    """a tiny SNUNet checkpoint and georeferenced rasters, as the end-to-end test of tests/test_gpu_sieve.py builds them"""
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
    model = SNUNet_ECAM(2, 3, base_channel=bc, precision="fp32")
    model.load_state_dict(seeded_fill_(R.new_state_dict(2, 3, bc)))
    torch.save({"epoch": 0, "model_state_dict": model.state_dict()}, str(tmp_path / "best.pt"))
    return [sys.executable, os.path.join(ROOT, "predict.py"), "--task", "cd", "--method", "snunet", "--checkpoint", str(tmp_path / "best.pt"),
            "--post", str(tmp_path / "post_vv.tif"), str(tmp_path / "post_vh.tif"), "--pre1", str(tmp_path / "pre.tif"),
            "--window", "32", "--stride", "16", "--batch_size", "5", "--precision", "fp32"]


def test_predict_script_with_mmu_and_polygons(tmp_path):
    from kurosiwo_amd import geotiff
    cmd = _tiny_scene(tmp_path) + ["--out", str(tmp_path / "flood.tif"), "--mmu", "6", "--polygons", str(tmp_path / "flood.geojson")]
    run = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    got, meta = geotiff.read(str(tmp_path / "flood.tif"))
    assert meta["pixel_scale"] == (10.0, 10.0) and meta["origin"] == (500000.0, 4100000.0)
    rings = polygon_ref.rings(got, (1, 2))
    want = polygon_ref.geojson(rings, got, pixel_scale=meta["pixel_scale"], origin=meta["origin"])
    with open(str(tmp_path / "flood.geojson")) as f:
        written = json.load(f)
    print(f"predict.py --mmu 6 --polygons: {len(want['features'])} features, {len(rings.label)} rings, {len(rings.verts)} vertices; "
          f"classes {np.bincount(got.ravel(), minlength=4).tolist()}")
    assert len(want["features"]) >= 3 and written == want and "crs" not in written
    assert f"{len(want['features'])} features, {len(rings.label)} rings" in run.stdout
    assert sum(f["properties"]["pixels"] for f in written["features"]) == int(((got == 1) | (got == 2)).sum())
    refused = subprocess.run(cmd + ["--slope"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "--slope is not supported" in refused.stderr
