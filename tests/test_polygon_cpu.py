"""Polygon output, host half (kurosiwo_amd/scene.py: polygonize, polygons_geojson; csrc/polygon.hip): the sequential walk of
tests/polygon_ref.py on hand cases with their rings written out, the three invariants of the ring table (no vertex twice in a ring;
one exterior ring per component, id 4 * label, every other ring a hole; the area2 of a component sums to twice its pixels) on speckled,
random and checkerboard maps, a cross-check against scipy.ndimage, the GeoJSON writer on oracle rings, and that the library exports
and binds the new entry points and refuses bad arguments before any launch.  No GPU."""
import numpy as np
import pytest

import polygon_ref
import sieve_ref

ENTRY_POINTS = ("ksmi_scan_i32", "ksmi_scene_edge_count", "ksmi_scene_edge_emit", "ksmi_scene_ring_trace", "ksmi_scene_ring_heads",
                "ksmi_scene_ring_table", "ksmi_scene_ring_order", "ksmi_scene_ring_verts")


def _rings(m, select=(1, 2)):
    m = np.asarray(m, dtype=np.uint8)
    tr = polygon_ref.trace(m, select)
    return tr, polygon_ref.rings(m, select, tr)


def _ring(r, i):
    return [tuple(v) for v in r.verts[r.start[i]:r.start[i + 1]].tolist()]


# ---------------------------------------------------------------------------------------------------- hand cases
def test_single_pixel():
    tr, r = _rings([[1]])
    assert tr.eid.tolist() == [0, 1, 2, 3] and tr.succ.tolist() == [1, 2, 3, 0]
    assert tr.ring_min.tolist() == [0, 0, 0, 0] and tr.rank.tolist() == [0, 1, 2, 3]
    assert r.label.tolist() == [0] and r.ring_id.tolist() == [0] and r.start.tolist() == [0, 4] and r.area2.tolist() == [2]
    assert _ring(r, 0) == [(1, 0), (1, 1), (0, 1), (0, 0)]
    assert r.area2.dtype == np.int64 and r.verts.dtype == np.int32 and r.verts.shape == (4, 2)


def test_two_by_two_block():
    tr, r = _rings([[2, 2], [2, 2]])
    assert tr.eid.tolist() == [0, 3, 4, 5, 10, 11, 13, 14]
    # top of 0 -> top of 1 -> right of 1 -> right of 3 -> bottom of 3 -> bottom of 2 -> left of 2 -> left of 0
    order = [0, 4, 5, 13, 14, 10, 11, 3]
    index = {e: k for k, e in enumerate(tr.eid.tolist())}
    for a, b in zip(order, order[1:] + order[:1]):
        assert tr.succ[index[a]] == index[b]
    assert [int(tr.rank[index[e]]) for e in order] == list(range(8)) and not tr.ring_min.any()
    assert r.ring_id.tolist() == [0] and r.area2.tolist() == [8] and _ring(r, 0) == [(2, 0), (2, 2), (0, 2), (0, 0)]


def test_l_shape():
    tr, r = _rings([[1, 0], [1, 1]], (1,))
    assert tr.eid.tolist() == [0, 1, 3, 10, 11, 12, 13, 14]
    assert r.label.tolist() == [0] and r.ring_id.tolist() == [0] and r.area2.tolist() == [6]
    assert _ring(r, 0) == [(1, 0), (1, 1), (2, 1), (2, 2), (0, 2), (0, 0)]
    both = polygon_ref.rings(np.asarray([[1, 0], [1, 1]], np.uint8), (0, 1))       # the other class as well: its pixel is a ring of its own
    assert both.ring_id.tolist() == [0, 4] and both.label.tolist() == [0, 1] and both.area2.tolist() == [6, 2]


def test_two_diagonal_pixels_are_two_rings():
    tr, r = _rings([[1, 0], [0, 1]], (1,))
    assert r.label.tolist() == [0, 3] and r.ring_id.tolist() == [0, 12] and r.area2.tolist() == [2, 2] and r.start.tolist() == [0, 4, 8]
    assert _ring(r, 0) == [(1, 0), (1, 1), (0, 1), (0, 0)] and _ring(r, 1) == [(2, 1), (2, 2), (1, 2), (1, 1)]
    assert tr.ring_min.tolist() == [0] * 4 + [4] * 4


def test_ring_with_one_corner_cut():
    """3 x 3 of class 1 without its centre and without pixel (0, 0): the exterior and the hole both pass through vertex (1, 1), where
    two diagonal pixels of the one component meet and the walk crosses over"""
    m = np.ones((3, 3), np.uint8)
    m[1, 1] = m[0, 0] = 0
    tr, r = _rings(m, (1,))
    assert r.ring_id.tolist() == [4, 6] and r.label.tolist() == [1, 1] and r.area2.tolist() == [16, -2]
    assert _ring(r, 0) == [(3, 0), (3, 3), (0, 3), (0, 1), (1, 1), (1, 0)]
    assert _ring(r, 1) == [(1, 1), (1, 2), (2, 2), (2, 1)]
    assert len(tr.eid) == 12 + 4 and (1, 1) in _ring(r, 0) and (1, 1) in _ring(r, 1)


def test_nothing_selected():
    tr, r = _rings([[0, 3], [3, 0]], (1, 2))
    assert all(len(a) == 0 for a in tr) and r.start.tolist() == [0] and r.verts.shape == (0, 2) and len(r.label) == 0
    assert polygon_ref.geojson(r, [[0, 3], [3, 0]]) == {"type": "FeatureCollection", "features": []}
    assert len(polygon_ref.trace(np.full((2, 2), 63, np.uint8), (63, 64)).eid) == 0          # class values above 62 are never selected


# ---------------------------------------------------------------------------------------------------- invariants
def _invariants(m, select):
    m = np.asarray(m, dtype=np.uint8)
    tr, r = _rings(m, select)
    lab = sieve_ref.label(m, 4).ravel()
    size = sieve_ref.sizes(lab.reshape(m.shape)).ravel()
    R = len(r.label)
    for i in range(R):                                                           # 1: no vertex twice in a ring
        ring = _ring(r, i)
        assert len(ring) >= 4 and len(set(ring)) == len(ring)
    assert np.all(np.diff(r.ring_id) > 0)
    want = sorted(int(l) for l in np.unique(lab) if polygon_ref.selected(m, select).ravel()[l])
    exterior = r.area2 > 0
    assert sorted(r.label[exterior].tolist()) == want                            # 2: one exterior ring per selected component ...
    assert np.array_equal(r.ring_id[exterior], 4 * r.label[exterior])            # ... its id 4 * label ...
    assert np.all(r.area2[~exterior] < 0)                                        # ... and every other ring a hole
    for l in want:
        mine = r.label == l
        assert r.ring_id[mine].min() == 4 * l
        assert int(r.area2[mine].sum()) == 2 * int(size[l])                      # 3
    assert int(np.bincount(tr.ring_min)[np.unique(tr.ring_min)].sum()) == len(tr.eid)
    return tr, r


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_invariants_on_speckled_scenes(seed):
    m = sieve_ref.speckle_scene(seed, 48, 80)
    for select in ((1, 2), (0, 1, 2, 3)):
        _, r = _invariants(m, select)
        assert (r.area2 < 0).any() and len(r.label) > 50


def test_invariants_on_random_small_maps_and_a_checkerboard():
    rng = np.random.default_rng(12)
    for _ in range(150):
        h, w = rng.integers(1, 8, size=2)
        _invariants(rng.integers(0, 3, size=(h, w), dtype=np.uint8), (1, 2) if rng.random() < 0.5 else (0, 1))
    yy, xx = np.mgrid[0:9, 0:12]
    tr, r = _invariants(((yy + xx) & 1).astype(np.uint8), (0, 1))
    assert len(r.label) == 9 * 12 and (r.area2 == 2).all() and (np.diff(r.start) == 4).all()


def test_against_scipy_ndimage():
    """exterior rings per class = scipy's edge-connected components; holes per component = the EDGE-connected components of its
    complement, padded by one pixel, minus one.  Edge-connected, not corner-connected: where the complement pinches through a corner
    between two diagonal pixels of the one component, the walk crosses over (invariant 1: no vertex twice in a ring) and so closes a
    ring on either side of the pinch.  The 3 x 3 ring with one corner cut shows it: its centre touches the cut corner, and with it the
    outside, only through vertex (1, 1), and is a hole all the same (test_ring_with_one_corner_cut)."""
    from scipy import ndimage
    cut = np.ones((3, 3), np.uint8)
    cut[1, 1] = cut[0, 0] = 0
    outside = np.pad(cut == 0, 1, constant_values=True)
    assert ndimage.label(outside)[1] - 1 == 1 and ndimage.label(outside, np.ones((3, 3), int))[1] - 1 == 0
    m = sieve_ref.speckle_scene(1, 48, 80)
    select = (0, 1, 2)
    r = polygon_ref.rings(m, select)
    lab = sieve_ref.label(m, 4)
    for c in select:
        n = ndimage.label(m == c)[1]                                             # the default structure: edges
        assert int(((r.area2 > 0) & (m.ravel()[r.label] == c)).sum()) == n
    holes_seen = 0
    for l in np.unique(lab):
        if m.ravel()[l] not in select:
            continue
        outside = np.pad(lab != l, 1, constant_values=True)                      # the complement, joined around the map
        holes = ndimage.label(outside)[1] - 1
        assert int(((r.label == l) & (r.area2 < 0)).sum()) == holes
        holes_seen += holes
    assert holes_seen >= 10


# ---------------------------------------------------------------------------------------------------- GeoJSON
def _shoelace(ring):
    return sum(x0 * y1 - x1 * y0 for (x0, y0), (x1, y1) in zip(ring, ring[1:]))


def test_polygons_geojson_on_oracle_rings():
    from kurosiwo_amd.scene import polygons_geojson
    m = sieve_ref.speckle_scene(2, 48, 80)
    r = polygon_ref.rings(m, (1, 2))
    size = sieve_ref.sizes(sieve_ref.label(m, 4)).ravel()
    scale, origin = (10.0, 20.0), (500000.0, 4100000.0)
    for kw in (dict(), dict(pixel_scale=scale, origin=origin), dict(pixel_scale=scale)):
        g = polygons_geojson(r, m, **kw)
        assert g == polygon_ref.geojson(r, m, **kw) and set(g) == {"type", "features"} and g["type"] == "FeatureCollection"
        labels = sorted(set(r.label.tolist()))
        assert len(g["features"]) == len(labels)
        sx, sy = kw.get("pixel_scale", (1.0, 1.0))
        ox, oy = kw.get("origin", (0.0, 0.0))
        for f, l in zip(g["features"], labels):                                  # features in ascending label
            mine = np.flatnonzero(r.label == l)                                  # ascending ring id: the exterior first
            assert f["type"] == "Feature" and f["geometry"]["type"] == "Polygon" and set(f["properties"]) == {"class", "pixels", "area"}
            assert f["properties"]["class"] == int(m.ravel()[l]) and f["properties"]["pixels"] == int(size[l])
            assert f["properties"]["area"] == (int(size[l]) * sx * sy if "pixel_scale" in kw else None)
            coords = f["geometry"]["coordinates"]
            assert len(coords) == len(mine) and r.ring_id[mine[0]] == 4 * l
            for j, (ring, i) in enumerate(zip(coords, mine)):
                want = [[ox + x * sx, oy - y * sy] for x, y in r.verts[r.start[i]:r.start[i + 1]].tolist()]
                assert ring[0] == want[0] and ring[1:-1] == want[:0:-1] and ring[-1] == ring[0]      # closed; against the walk
                assert all(type(v) is float for xy in ring for v in xy)
                a = _shoelace([(x - ox, y - oy) for x, y in ring])                # y points up: a positive sum is counter-clockwise
                assert (a > 0) == (j == 0) and a == int(r.area2[i]) * sx * sy
    one = polygons_geojson(polygon_ref.rings(np.asarray([[1]], np.uint8)), np.asarray([[1]], np.uint8), (2.0, 3.0), (10.0, 50.0))
    assert one["features"][0]["geometry"]["coordinates"] == [[[12.0, 50.0], [10.0, 50.0], [10.0, 47.0], [12.0, 47.0], [12.0, 50.0]]]
    assert one["features"][0]["properties"] == {"class": 1, "pixels": 1, "area": 6.0}


# ---------------------------------------------------------------------------------------------------- the library
def test_library_exports_the_polygon_entry_points():
    from kurosiwo_amd import _lib, scene
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and args[-1] is _lib.C.c_void_p               # a launch-list entry: int status, the stream last
    assert hasattr(lib, "ksmi_scan_i32_scratch") and _lib.SIGNATURES["ksmi_scan_i32_scratch"][0] is _lib.C.c_int64
    assert lib.ksmi_abi_version() == 8
    T = scene.SCAN_TILE
    assert T <= 4096
    want = lambda n: 0 if n <= T else -(-n // T) + want(-(-n // T))
    for n in (0, 1, T, T + 1, T * T, T * T + 1, 2 ** 31 - 1):
        assert lib.ksmi_scan_i32_scratch(n) == want(n)
    assert lib.ksmi_scan_i32_scratch(-1) == -1 and lib.ksmi_scan_i32_scratch(2 ** 31) == -1


def test_polygon_argument_errors_need_no_device():
    """the checks run before any launch: with made-up non-null addresses a refused call returns before touching them"""
    from kurosiwo_amd import _lib, scene
    lib = _lib.load()
    P, T = 4096, scene.SCAN_TILE
    err = lambda name: name.encode() in lib.ksmi_last_error()
    assert lib.ksmi_scan_i32(None, P, 8, P, None, 0, None) < 0 and err("scan_i32")
    assert lib.ksmi_scan_i32(P, None, 8, P, None, 0, None) < 0
    assert lib.ksmi_scan_i32(P, P, 8, None, None, 0, None) < 0
    assert lib.ksmi_scan_i32(P, P, -1, P, None, 0, None) < 0                                               # n < 0
    assert lib.ksmi_scan_i32(P, P, 2 ** 31, P, P, 2 ** 31, None) < 0
    assert lib.ksmi_scan_i32(P, P, T + 1, P, P, 1, None) < 0 and err("scan_i32")                           # scratch too small
    assert lib.ksmi_scan_i32(P, P, T + 1, P, None, 2, None) < 0
    assert lib.ksmi_scan_i32(P, P, 0, P, None, 0, None) == 0
    big = (23171, 23171)                                                                                   # 23171^2 > 2^29 - 1
    assert big[0] * big[1] > 2 ** 29 - 1 and 23170 * 23170 <= 2 ** 29 - 1
    assert lib.ksmi_scene_edge_count(P, P, 6, *big, P, None) < 0 and err("scene_edge_count")
    assert lib.ksmi_scene_edge_count(None, P, 6, 4, 4, P, None) < 0
    assert lib.ksmi_scene_edge_count(P, None, 6, 4, 4, P, None) < 0
    assert lib.ksmi_scene_edge_count(P, P, 6, 4, 4, None, None) < 0
    assert lib.ksmi_scene_edge_count(P, P, 6, 0, 4, P, None) < 0
    assert lib.ksmi_scene_edge_count(P, P, -1, 4, 4, P, None) < 0                                          # bit 63
    assert lib.ksmi_scene_edge_emit(P, P, 6, *big, P, 4, P, P, None) < 0 and err("scene_edge_emit")
    assert lib.ksmi_scene_edge_emit(P, P, 6, 4, 4, P, -1, P, P, None) < 0                                  # E < 0
    assert lib.ksmi_scene_edge_emit(P, P, 6, 4, 4, P, 65, P, P, None) < 0                                  # more than 4 per pixel
    assert lib.ksmi_scene_edge_emit(P, P, 6, 4, 4, P, 8, None, P, None) < 0
    assert lib.ksmi_scene_edge_emit(P, P, 6, 4, 4, None, 8, P, P, None) < 0
    assert lib.ksmi_scene_edge_emit(P, P, 6, 4, 4, P, 0, P, P, None) == 0
    assert lib.ksmi_scene_ring_trace(P, -1, 3, P, P, P, 64, None) < 0 and err("scene_ring_trace")
    assert lib.ksmi_scene_ring_trace(P, 16, 3, P, P, P, 63, None) < 0                                         # scratch too small
    assert lib.ksmi_scene_ring_trace(None, 16, 3, P, P, P, 64, None) < 0
    assert lib.ksmi_scene_ring_trace(P, 16, 3, P, None, P, 64, None) < 0
    assert lib.ksmi_scene_ring_trace(P, 16, 0, P, P, P, 64, None) < 0 and lib.ksmi_scene_ring_trace(P, 16, 4, P, P, P, 64, None) < 0       # phases
    assert lib.ksmi_scene_ring_trace(P, 16, 3, P, P, None, 64, None) < 0
    assert lib.ksmi_scene_ring_trace(P, 0, 3, P, P, None, 0, None) == 0
    assert lib.ksmi_scene_ring_heads(P, -1, P, None) < 0 and err("scene_ring_heads")
    assert lib.ksmi_scene_ring_heads(None, 4, P, None) < 0
    assert lib.ksmi_scene_ring_heads(P, 0, P, None) == 0
    assert lib.ksmi_scene_ring_table(P, P, P, P, P, P, 16, -1, 1, P, P, P, None) < 0 and err("scene_ring_table")
    assert lib.ksmi_scene_ring_table(P, P, P, P, P, P, 16, 8, 9, P, P, P, None) < 0                        # more rings than edges
    assert lib.ksmi_scene_ring_table(P, P, P, P, P, P, 2 ** 29, 8, 2, P, P, P, None) < 0
    assert lib.ksmi_scene_ring_table(P, P, P, P, P, None, 16, 8, 2, P, P, P, None) < 0
    assert lib.ksmi_scene_ring_table(P, P, P, P, P, P, 16, 0, 0, P, P, P, None) == 0
    assert lib.ksmi_scene_ring_order(P, P, P, P, P, P, -1, 0, P, P, P, None) < 0 and err("scene_ring_order")
    assert lib.ksmi_scene_ring_order(P, P, P, P, P, None, 8, 2, P, P, P, None) < 0
    assert lib.ksmi_scene_ring_order(P, P, P, P, P, P, 8, 2, P, P, None, None) < 0
    assert lib.ksmi_scene_ring_order(P, P, P, P, P, P, 0, 0, P, P, P, None) == 0
    assert lib.ksmi_scene_ring_verts(P, P, P, -1, 0, 0, 4, P, P, P, None) < 0 and err("scene_ring_verts")
    assert lib.ksmi_scene_ring_verts(P, P, P, 8, 2, 9, 4, P, P, P, None) < 0                               # more vertices than edges
    assert lib.ksmi_scene_ring_verts(P, P, P, 8, 2, 8, 0, P, P, P, None) < 0                               # Ws < 1
    assert lib.ksmi_scene_ring_verts(P, P, P, 8, 2, 8, 4, P, None, P, None) < 0
    assert lib.ksmi_scene_ring_verts(P, P, P, 8, 2, 8, 4, P, P, None, None) < 0
    assert lib.ksmi_scene_ring_verts(P, P, P, 0, 0, 0, 4, P, P, P, None) == 0


def test_polygon_wrappers_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from kurosiwo_amd import _lib
    from kurosiwo_amd.scene import Rings, boundary_edges, polygonize, scan_i32, trace_rings
    assert Rings._fields == ("label", "ring_id", "start", "area2", "verts")
    m, lab, v = torch.zeros((4, 4), dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.int32), torch.zeros(8, dtype=torch.int32)
    for call in (lambda: polygonize(m), lambda: polygonize(m, labels=lab), lambda: boundary_edges(m, lab), lambda: trace_rings(v),
                 lambda: scan_i32(v)):
        with pytest.raises(_lib.KsmiError):
            call()
    for select in ((63,), (-1,), (1.5,)):                                        # before the tensors are looked at
        with pytest.raises(ValueError):
            polygonize(m, select)
        with pytest.raises(ValueError):
            boundary_edges(m, lab, select)
