"""Polygon output of a class map restated in plain Python and numpy (kurosiwo_amd/scene.py: boundary_edges, trace_rings, polygonize,
polygons_geojson; csrc/polygon.hip): a sequential boundary walk on the 4-connectivity labels of tests/sieve_ref.py.  Integers
throughout, so the tests ask for equal bits.

Image coordinates: x to the right, y down; a vertex is a pixel corner (vx, vy).  Side s of pixel (x, y) is walked clockwise on screen,
the pixel on the right of the heading: 0 top (x, y) -> (x+1, y), 1 right (x+1, y) -> (x+1, y+1), 2 bottom (x+1, y+1) -> (x, y+1), 3 left
(x, y+1) -> (x, y).  The heading of side s is HEADING[s]; its edge id is 4 * (y * W + x) + s."""
from collections import namedtuple

import numpy as np

import sieve_ref

HEADING = ((1, 0), (0, 1), (-1, 0), (0, -1))                      # of side 0 .. 3: east, south, west, north
START = ((0, 0), (1, 0), (1, 1), (0, 1))                          # the corner of the pixel a side starts at
ACROSS = ((0, -1), (1, 0), (0, 1), (-1, 0))                       # the pixel on the other side of a side
# the pixel on the right of an edge that LEAVES vertex (vx, vy) with heading h is (vx, vy) + RIGHT_OF[h]: the edge is its side h
RIGHT_OF = ((0, 0), (-1, 0), (-1, -1), (0, -1))

Rings = namedtuple("Rings", "label ring_id start area2 verts")
Trace = namedtuple("Trace", "eid succ ring_min rank")


def selected(classes, select):
    classes = np.asarray(classes)
    ok = np.zeros(classes.shape, bool)
    for c in select:
        if 0 <= int(c) <= 62:
            ok |= classes == int(c)
    return ok


def trace(classes, select=(1, 2)):
    """Trace(eid, succ, ring_min, rank), int32 [E] each, indexed by compact index (the rank of an edge among all boundary edges in
    ascending edge id): the edge id, the compact index of the successor, of the smallest edge of the ring, and the number of successor
    steps from that smallest edge"""
    classes = np.asarray(classes, dtype=np.uint8)
    H, W = classes.shape
    lab = sieve_ref.label(classes, 4).tolist() if H * W else []
    sel = selected(classes, select).tolist()

    def label_at(x, y):
        return lab[y][x] if 0 <= x < W and 0 <= y < H else -1

    def is_edge(x, y, s):
        """side s of pixel (x, y) is a boundary edge"""
        if not (0 <= x < W and 0 <= y < H) or not sel[y][x]:
            return False
        return label_at(x + ACROSS[s][0], y + ACROSS[s][1]) != lab[y][x]

    eid = [4 * (y * W + x) + s for y in range(H) for x in range(W) for s in range(4) if is_edge(x, y, s)]
    index = {e: k for k, e in enumerate(eid)}
    succ = []
    for e in eid:
        p, s = divmod(e, 4)
        y, x = divmod(p, W)
        m = lab[y][x]
        vx, vy = x + START[(s + 1) % 4][0], y + START[(s + 1) % 4][1]           # the end vertex: where the next side of the pixel starts
        for h in ((s + 3) % 4, s, (s + 1) % 4):                                    # left of the heading, the heading, right of it
            qx, qy = vx + RIGHT_OF[h][0], vy + RIGHT_OF[h][1]
            if label_at(qx, qy) == m and is_edge(qx, qy, h):
                succ.append(index[4 * (qy * W + qx) + h])
                break
        else:
            raise AssertionError(f"edge {e} has no successor")
    E = len(eid)
    assert sorted(succ) == list(range(E)), "the successor map is a permutation"
    ring_min, rank = [-1] * E, [-1] * E
    for k in range(E):                                                             # ascending: the first edge met of a ring is its smallest
        if ring_min[k] >= 0:
            continue
        j, n = k, 0
        while ring_min[j] < 0:
            ring_min[j], rank[j] = k, n
            j, n = succ[j], n + 1
        assert j == k
    as32 = lambda v: np.asarray(v, dtype=np.int32).reshape(-1)
    return Trace(as32(eid), as32(succ), as32(ring_min), as32(rank))


def edge_vertices(e, W):
    """(x0, y0, x1, y1): the start and end vertex of edge id e"""
    p, s = divmod(int(e), 4)
    y, x = divmod(p, W)
    return x + START[s][0], y + START[s][1], x + START[(s + 1) % 4][0], y + START[(s + 1) % 4][1]


def rings(classes, select=(1, 2), tr=None):
    """Rings(label int32 [R], ring_id int32 [R], start int32 [R + 1], area2 int64 [R], verts int32 [V, 2]) in ascending ring id"""
    classes = np.asarray(classes, dtype=np.uint8)
    H, W = classes.shape
    tr = trace(classes, select) if tr is None else tr
    lab = sieve_ref.label(classes, 4).ravel() if H * W else np.zeros(0, np.int32)
    eid, succ = tr.eid.tolist(), tr.succ.tolist()
    label, ring_id, start, area2, verts = [], [], [0], [], []
    for k in range(len(eid)):
        if tr.ring_min[k] != k:
            continue
        ring_id.append(eid[k])
        label.append(int(lab[eid[k] // 4]))
        a, j = 0, k
        while True:
            x0, y0, x1, y1 = edge_vertices(eid[j], W)
            a += x0 * y1 - x1 * y0
            if eid[succ[j]] % 4 != eid[j] % 4:                                     # the walk turns at the end of this edge
                verts.append((x1, y1))
            j = succ[j]
            if j == k:
                break
        area2.append(a)
        start.append(len(verts))
    return Rings(np.asarray(label, np.int32), np.asarray(ring_id, np.int32), np.asarray(start, np.int32), np.asarray(area2, np.int64),
                 np.asarray(verts, np.int32).reshape(-1, 2))


def geojson(r, classes, pixel_scale=None, origin=None):
    """the FeatureCollection of kurosiwo_amd.scene.polygons_geojson from a ring table: one Polygon per component in ascending label,
    the exterior first, then the holes in ascending ring id; [ox + x * sx, oy - y * sy].  The walk is clockwise on screen and a
    north-up map keeps that sense, so each ring is written against the walk: exteriors counter-clockwise, holes clockwise"""
    flat = np.asarray(classes).ravel()
    sx, sy = (1.0, 1.0) if pixel_scale is None else (float(pixel_scale[0]), float(pixel_scale[1]))
    ox, oy = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    by_label = {}
    for i in range(len(r.label)):                                                  # ascending ring id within a label
        by_label.setdefault(int(r.label[i]), []).append(i)
    features = []
    for l in sorted(by_label):
        coords, twice = [], 0
        for i in by_label[l]:
            ring = [[ox + float(x) * sx, oy - float(y) * sy] for x, y in r.verts[r.start[i]:r.start[i + 1]].tolist()]
            coords.append([ring[0]] + ring[:0:-1] + [ring[0]])                    # from the first vertex, against the walk
            twice += int(r.area2[i])
        pixels = twice // 2
        features.append({"type": "Feature", "properties": {"class": int(flat[l]), "pixels": pixels,
                                                           "area": None if pixel_scale is None else pixels * sx * sy},
                         "geometry": {"type": "Polygon", "coordinates": coords}})
    return {"type": "FeatureCollection", "features": features}
