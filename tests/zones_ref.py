"""The definition of zones from a vector layer (kurosiwo_amd.scene.rasterize_zones, csrc/zones.hip) in numpy and Python integers: the
scanline crossings of the edges, their sort, the pairing into spans and the smallest feature per pixel; a vectorised form (np.repeat,
np.minimum.at) and a direct loop over features and scanlines that it is checked against.  Also the scalar restatement of
kurosiwo_amd.scene.zone_edges (map coordinates -> edges in 1/256 pixel, Sutherland-Hodgman clipping) and the numpy form of the
--zones_out table of predict.py, built on tests/zonal_ref.py and tests/quantile_ref.py.  Integers throughout: numpy's // is the
floor division the rule asks for."""
import numpy as np

import quantile_ref
import zonal_ref

MAX_SIDE = 32767
MAX_COORD = 3 * 32767 * 256


def _oriented(edges):
    """(x0, y0, x1, y1) int64 with y0 <= y1"""
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    up = e[:, 1] <= e[:, 3]
    return (np.where(up, e[:, 0], e[:, 2]), np.where(up, e[:, 1], e[:, 3]), np.where(up, e[:, 2], e[:, 0]), np.where(up, e[:, 3], e[:, 1]))


def rows(edges, Hs):
    """(ylo, yhi) per edge: it crosses the scanlines ylo .. yhi - 1: y0 <= 256 y + 128 < y1, kept to 0 <= y < Hs"""
    _, y0, _, y1 = _oriented(edges)
    lo, hi = -((128 - y0) // 256), -((128 - y1) // 256)                     # ceil((y - 128) / 256)
    lo = np.maximum(lo, 0)
    return lo, np.maximum(np.minimum(hi, Hs), lo)


def crossings(edges, feature, Hs, Ws):
    """the composites f << 32 | y << 16 | c of all crossings, uint64 [X], in edge order and ascending scanline within an edge"""
    edges, feature = np.asarray(edges), np.asarray(feature, np.int64)
    assert edges.ndim == 2 and edges.shape[1] == 4 and feature.shape == (edges.shape[0],)
    assert 0 <= Hs <= MAX_SIDE and 0 <= Ws <= MAX_SIDE
    assert edges.size == 0 or (np.abs(edges.astype(np.int64)).max() <= MAX_COORD and feature.min() >= 0)
    x0, y0, x1, y1 = _oriented(edges)
    lo, hi = rows(edges, Hs)
    n = hi - lo
    e = np.repeat(np.arange(edges.shape[0]), n)
    first = np.cumsum(n) - n
    y = lo[e] + (np.arange(int(n.sum())) - first[e])
    dy, dx, cy = (y1 - y0)[e], (x1 - x0)[e], 256 * y + 128
    num, den = x0[e] * dy + (cy - y0[e]) * dx - 128 * dy, 256 * dy
    c = np.clip(-((-num) // den), 0, Ws)                                    # the ceiling, exactly
    return (feature[e].astype(np.uint64) << np.uint64(32)) | (y.astype(np.uint64) << np.uint64(16)) | c.astype(np.uint64)


def spans(composites):
    """the sorted composites paired -> (f, y, c0, c1) int64 arrays, one entry per pair; asserts the global pairing: every (f, y) group
    has an even size, so no pair straddles two groups"""
    s = np.sort(np.asarray(composites, np.uint64))
    assert s.size % 2 == 0, "an odd number of crossings: a ring is not closed"
    a, b = s[0::2], s[1::2]
    assert np.array_equal(a >> np.uint64(16), b >> np.uint64(16)), "a pair of crossings straddles two (feature, scanline) groups"
    return ((a >> np.uint64(32)).astype(np.int64), ((a >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64),
            (a & np.uint64(0xFFFF)).astype(np.int64), (b & np.uint64(0xFFFF)).astype(np.int64))


def rasterize(edges, feature, Hs, Ws):
    """the vectorised form -> zones int32 [Hs, Ws]"""
    f, y, c0, c1 = spans(crossings(edges, feature, Hs, Ws))
    n = c1 - c0
    k = np.repeat(np.arange(f.size), n)
    first = np.cumsum(n) - n
    pixel = y[k] * Ws + c0[k] + (np.arange(int(n.sum())) - first[k])
    flat = np.full(Hs * Ws, 2 ** 32 - 1, np.int64)
    np.minimum.at(flat, pixel, f[k])
    return np.where(flat == 2 ** 32 - 1, -1, flat).astype(np.int32).reshape(Hs, Ws)


def rasterize_loop(edges, feature, Hs, Ws):
    """the definition: feature by feature from the last to the first, scanline by scanline, in Python integers"""
    zones = np.full((Hs, Ws), -1, np.int32)
    table = [tuple(int(v) for v in e) for e in np.asarray(edges).reshape(-1, 4)]
    owner = [int(v) for v in np.asarray(feature)]
    for f in sorted(set(owner), reverse=True):                              # the smallest feature is written last
        mine = [e for e, o in zip(table, owner) if o == f]
        for y in range(Hs):
            cy, cols = 256 * y + 128, []
            for x0, y0, x1, y1 in mine:
                if y0 == y1:
                    continue
                if y0 > y1:
                    x0, y0, x1, y1 = x1, y1, x0, y0
                if y0 <= cy < y1:
                    dy, dx = y1 - y0, x1 - x0
                    num, den = x0 * dy + (cy - y0) * dx - 128 * dy, 256 * dy
                    cols.append(min(max(-((-num) // den), 0), Ws))
            cols.sort()
            assert len(cols) % 2 == 0
            for c0, c1 in zip(cols[0::2], cols[1::2]):
                zones[y, c0:c1] = f
    return zones


# ---------------------------------------------------------------------------------------------------- zone_edges
def _clip(ring, axis, bound, keep_above):
    """one Sutherland-Hodgman pass over a list of (x, y) float pairs"""
    out = []
    inside = lambda p: p[axis] >= bound if keep_above else p[axis] <= bound
    for i, a in enumerate(ring):
        b = ring[(i + 1) % len(ring)]
        if inside(a):
            out.append(a)
        if inside(a) != inside(b):
            lo, hi = (a, b) if a <= b else (b, a)                           # from the lexicographically smaller end
            t = (bound - lo[axis]) / (hi[axis] - lo[axis])
            hit = [lo[0] + t * (hi[0] - lo[0]), lo[1] + t * (hi[1] - lo[1])]
            hit[axis] = bound
            out.append(tuple(hit))
    return out


def zone_edges(features, Hs, Ws, pixel_scale=None, origin=None):
    """(edges int32 [E, 4], feature int32 [E], count): kurosiwo_amd.scene.zone_edges ring by ring and vertex by vertex"""
    sx, sy = (1.0, 1.0) if pixel_scale is None else (float(pixel_scale[0]), float(pixel_scale[1]))
    ox, oy = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    edges, owner = [], []
    for f, rings in enumerate(features):
        for ring in rings:
            p = [((float(v[0]) - ox) / sx, (oy - float(v[1])) / sy) for v in ring]
            if len(p) > 1 and p[0] == p[-1]:
                p = p[:-1]
            if any(x < -Ws or x > 2 * Ws or y < -Hs or y > 2 * Hs for x, y in p):
                for axis, bound, keep_above in ((0, -float(Ws), True), (0, 2.0 * Ws, False), (1, -float(Hs), True), (1, 2.0 * Hs, False)):
                    p = _clip(p, axis, bound, keep_above) if p else p
            q = [(int(np.rint(256.0 * x)), int(np.rint(256.0 * y))) for x, y in p]
            if len(q) < 3:
                continue
            for i, a in enumerate(q):
                edges.append(a + q[(i + 1) % len(q)])
                owner.append(f)
    return np.asarray(edges, np.int32).reshape(-1, 4), np.asarray(owner, np.int32), len(features)


def ring_edges(rings_of_features, scale=256):
    """integer rings (lists of (x, y) vertices, one list of rings per feature) times `scale` -> (edges int32 [E, 4], feature int32 [E])"""
    edges, owner = [], []
    for f, rings in enumerate(rings_of_features):
        for ring in rings:
            q = [(int(x) * scale, int(y) * scale) for x, y in ring]
            for i, a in enumerate(q):
                edges.append(a + q[(i + 1) % len(q)])
                owner.append(f)
    return np.asarray(edges, np.int32).reshape(-1, 4), np.asarray(owner, np.int32)


# ---------------------------------------------------------------------------------------------------- predict.py --zones_out
def cell(v):
    """a cell of the table as predict.py writes it: a null is empty, repr of a float reads back to the same float64"""
    return "" if v is None else repr(v) if isinstance(v, float) else str(v)


def zones_table(zones, ids, classes, zone_classes=(1, 2), area=None, depth=None, depth_classes=(1, 2), percents=None):
    """the rows of --zones_out, header first, every cell a string -> (rows, report): zones int32 [Hs, Ws] with F = len(ids) features,
    classes the uint8 map as written, depth the float32 depth raster as written (or None), percents in percent (or None)"""
    zones, classes = np.asarray(zones, np.int32), np.asarray(classes)
    F = len(ids)
    z = zones.ravel().astype(np.int64)
    inside = (z >= 0) & (z < F)
    count = lambda keep: np.bincount(z[inside & keep.ravel()], minlength=F).astype(np.int64)
    pixels, valid = count(np.ones(classes.shape, bool)), count(classes != 3)
    per_class = [count(classes == k) for k in range(4)]
    flooded = count(np.isin(classes, zone_classes))
    header = ["zone", "id", "pixels", "valid"] + [f"class_{k}" for k in range(4)] + ["flooded", "flooded_area", "flooded_fraction"]
    cols = [list(range(F)), list(ids), pixels.tolist(), valid.tolist()] + [c.tolist() for c in per_class] + [flooded.tolist()]
    cols.append([None if area is None else n * area for n in flooded.tolist()])
    cols.append([n / v if v else None for n, v in zip(flooded.tolist(), valid.tolist())])
    if depth is not None:
        depth = np.ascontiguousarray(depth, np.float32)
        water = np.isin(classes, depth_classes).astype(np.uint8)
        st = zonal_ref.zonal_stats(zones, depth, water, 16)
        keep = st.zone < F                                                  # zone ids are below F by construction
        assert keep.all()
        n, top, metres = np.zeros(F, np.int64), np.zeros(F, np.float64), np.zeros(F, np.float64)
        n[st.zone], top[st.zone], metres[st.zone] = st.valid[0], st.vmax[0].astype(np.float64), st.vsum[0] / float(2 ** 16)
        header += ["depth_pixels", "depth_max", "depth_mean", "volume"]
        cols.append(n.tolist())
        cols.append([float(v) if k else None for v, k in zip(top.tolist(), n.tolist())])
        cols.append([m / k if k else None for m, k in zip(metres.tolist(), n.tolist())])
        cols.append([None if area is None else m * area for m in metres.tolist()])
        if percents:
            zq = quantile_ref.zonal_quantiles(zones, depth, percents, water)
            lin = quantile_ref.values(zq)[0]
            for j, c in enumerate(zq.percentiles):
                whole, part = divmod(int(c), 100)
                header.append(f"depth_p{whole}" + (("_" + f"{part:02d}".rstrip("0")) if part else ""))
                column = [None] * F
                for r, zone in enumerate(zq.zone.tolist()):
                    column[zone] = float(lin[j, r]) if zq.valid[0, r] else None
                cols.append(column)
    rows = [header] + [[cell(c[f]) for c in cols] for f in range(F)]
    report = {"features": F, "with_pixels": int((pixels > 0).sum()), "pixels": int(pixels.sum())}
    return rows, report


def edges_of_rings(label, start, verts, scale=256):
    """a ring table (the label, start and verts of polygon_ref.rings or kurosiwo_amd.scene.polygonize, as arrays) -> (edges int32
    [E, 4], feature int32 [E], labels): one feature per component, numbered by the rank of its label; vertices times `scale`"""
    label, start, verts = np.asarray(label, np.int64), np.asarray(start, np.int64), np.asarray(verts, np.int64).reshape(-1, 2)
    labels, rank = np.unique(label, return_inverse=True)
    n = np.diff(start)
    ring = np.repeat(np.arange(label.size), n)
    k = np.arange(verts.shape[0])
    nxt = np.where(k + 1 == start[1:][ring], start[:-1][ring], k + 1) if verts.shape[0] else k
    edges = np.concatenate((verts, verts[nxt]), axis=1) * scale
    return edges.astype(np.int32).reshape(-1, 4), rank.reshape(-1)[ring].astype(np.int32), labels
