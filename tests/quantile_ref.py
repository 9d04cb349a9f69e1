"""The definition of percentiles per zone (kurosiwo_amd.scene.zonal_quantiles, zonal_sorted, csrc/quantile.hip) in numpy: a direct
loop per zone and a vectorised form (np.lexsort on (key, row)) that it is checked against.  Integers and bit copies throughout: the
position c * (n - 1) of a percentile of c basis points is taken in exact integer arithmetic, and `lower` / `higher` are elements of
the input.  The float64 combinations of `values` restate kurosiwo_amd.scene.quantile_values."""
from collections import namedtuple

import numpy as np

from zonal_ref import _inputs, key, unkey

ZonalQuantiles = namedtuple("ZonalQuantiles", "zone valid lower higher percentiles")
NAN = np.uint32(0x7FC00000)
METHODS = ("linear", "lower", "higher", "midpoint", "nearest")


def basis_points(percents):
    """percents -> basis points c = round(100 * p), for percents that are whole numbers of basis points"""
    out = tuple(int(round(100 * float(p))) for p in percents)
    assert all(0 <= c <= 10000 and abs(float(p) - c / 100) <= 1e-9 for p, c in zip(percents, out))
    return out


def position(c, n):
    """(k, g): the index of `lower` among n sorted values and the fraction towards `higher`, in basis points"""
    pos = int(c) * (int(n) - 1)
    return pos // 10000, pos % 10000


def _rows(z, keep):
    zone, inv = np.unique(z[keep], return_inverse=True)
    return zone.astype(np.int32), inv.reshape(-1)


def zonal_sorted_loop(zones, values, where=None):
    """(zone int32 [N], offsets int32 [N + 1], sorted float32 [total]) of one band [Hs, Ws]: zone by zone, a Python sort of the keys"""
    z, keep, vals, Hs, Ws = _inputs(zones, values, where)
    assert vals.shape[0] == 1
    ids = sorted(set(int(v) for v in z[keep]))
    offsets, parts = [0], []
    for zid in ids:
        v = vals[0][keep & (z == zid)]
        v = v[np.isfinite(v)]
        ks = sorted(int(k) for k in key(v))
        parts.append(unkey(np.asarray(ks, np.uint32)))
        offsets.append(offsets[-1] + len(ks))
    flat = np.concatenate(parts) if parts else np.empty(0, np.float32)
    return np.asarray(ids, np.int32).reshape(len(ids)), np.asarray(offsets, np.int32), flat.astype(np.float32)


def zonal_sorted(zones, values, where=None):
    """the vectorised form: one np.lexsort on (key, row) over the pixels that take part"""
    z, keep, vals, Hs, Ws = _inputs(zones, values, where)
    assert vals.shape[0] == 1
    zone, inv = _rows(z, keep)
    v = vals[0][keep]
    fin = np.isfinite(v)
    k, r = key(v[fin]), inv[fin]
    order = np.lexsort((k, r))                                                # the last key is the primary one
    offsets = np.zeros(zone.size + 1, np.int64)
    np.add.at(offsets, r + 1, 1)
    return zone, np.cumsum(offsets).astype(np.int32), unkey(k[order])


def _select(offsets, flat, pcts):
    N = offsets.size - 1
    bits = flat.view(np.uint32)
    lower, higher = np.full((len(pcts), N), NAN, np.uint32), np.full((len(pcts), N), NAN, np.uint32)
    n = np.diff(offsets.astype(np.int64))
    some = n > 0
    for j, c in enumerate(pcts):
        pos = int(c) * (n[some] - 1)
        k, g = pos // 10000, pos % 10000
        lower[j, some] = bits[offsets[:-1][some] + k]
        higher[j, some] = bits[offsets[:-1][some] + k + (g > 0)]
    return n.astype(np.int32), lower.view(np.float32), higher.view(np.float32)


def zonal_quantiles(zones, values, percents=(50,), where=None):
    """the vectorised form; percents as the Python interface takes them"""
    pcts = basis_points(percents)
    values = np.asarray(values)
    if values.ndim == 2:
        values = values[None]
    zone, cols = None, []
    for b in range(values.shape[0]):
        zone, offsets, flat = zonal_sorted(zones, values[b], where)
        cols.append(_select(offsets, flat, pcts))
    N, P = zone.size, len(pcts)
    return ZonalQuantiles(zone, np.stack([c[0] for c in cols]).reshape(len(cols), N), np.stack([c[1] for c in cols]).reshape(len(cols), P, N),
                          np.stack([c[2] for c in cols]).reshape(len(cols), P, N), pcts)


def zonal_quantiles_loop(zones, values, percents=(50,), where=None):
    """the definition: per band, zone and percentile, by position() on the zone's sorted values"""
    pcts = basis_points(percents)
    values = np.asarray(values)
    if values.ndim == 2:
        values = values[None]
    B, P = values.shape[0], len(pcts)
    zone, _, _ = zonal_sorted_loop(zones, values[0], where)
    N = zone.size
    out = ZonalQuantiles(zone, np.zeros((B, N), np.int32), np.full((B, P, N), NAN, np.uint32).view(np.float32),
                         np.full((B, P, N), NAN, np.uint32).view(np.float32), pcts)
    for b in range(B):
        _, offsets, flat = zonal_sorted_loop(zones, values[b], where)
        for r in range(N):
            s = flat[offsets[r]:offsets[r + 1]]
            out.valid[b, r] = s.size
            for j, c in enumerate(pcts):
                if s.size:
                    k, g = position(c, s.size)
                    out.lower[b, j, r], out.higher[b, j, r] = s[k], s[k + (g > 0)]
    return out


def same(a, b):
    """the names of the fields in which two ZonalQuantiles differ in dtype, shape or bits"""
    bad = []
    for name in ZonalQuantiles._fields[:-1]:
        u, v = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in (getattr(a, name), getattr(b, name)))
        if u.dtype != v.dtype or u.shape != v.shape or u.tobytes() != v.tobytes():
            bad.append(name)
    if tuple(int(c) for c in a.percentiles) != tuple(int(c) for c in b.percentiles):
        bad.append("percentiles")
    return bad


def values(zq, method="linear"):
    """float64 [B, P, N]: lower and higher combined as kurosiwo_amd.scene.quantile_values combines them, element by element"""
    assert method in METHODS
    host = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    lower, higher, valid = host(zq.lower), host(zq.higher), host(zq.valid)
    out = np.full(lower.shape, np.nan, np.float64)
    for b in range(lower.shape[0]):
        for j, c in enumerate(zq.percentiles):
            for r in range(lower.shape[2]):
                if valid[b, r] == 0:
                    continue
                lo, hi, g = float(lower[b, j, r]), float(higher[b, j, r]), position(c, valid[b, r])[1]
                out[b, j, r] = {"linear": lo + (hi - lo) * (g / 10000), "lower": lo, "higher": hi, "midpoint": (lo + hi) / 2,
                                "nearest": lo if 2 * g <= 10000 else hi}[method]
    return out
