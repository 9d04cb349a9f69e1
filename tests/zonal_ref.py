"""The definition of zonal statistics (kurosiwo_amd.scene.zonal_stats, csrc/zonal.hip) in numpy: a vectorised form (np.unique,
integer np.add.at, key-ordered min / max) and a direct per-zone loop that it is checked against.  Integers throughout but for the
one fp32 product of the fixed-point rule, which is exact.  No float sum anywhere: np.bincount with weights goes through float64."""
from collections import namedtuple

import numpy as np

Zonal = namedtuple("Zonal", "zone count bbox sum_x sum_y valid vmin vmax vsum frac_bits")
MAX_BANDS = 8


def key(v):
    """uint32 keys of float32 values: k = bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000); unsigned order, -0.0 < +0.0"""
    bits = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return bits ^ np.where(bits >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def quantise(v, frac_bits):
    """q(v) = rint(clamp(v, -2^(32 - frac_bits), 2^(32 - frac_bits)) * 2^frac_bits) as int64: the product in fp32 (exact: a power of
    two after the clamp), rint to even.  For finite v."""
    if not 0 <= int(frac_bits) <= 30:
        raise ValueError("frac_bits in 0 .. 30")
    limit = np.float32(2.0 ** (32 - int(frac_bits)))
    scaled = np.clip(np.asarray(v, np.float32), -limit, limit).astype(np.float32) * np.float32(2.0 ** int(frac_bits))
    assert scaled.dtype == np.float32
    return np.rint(scaled).astype(np.int64)


def _inputs(zones, values, where):
    zones = np.asarray(zones)
    assert zones.dtype == np.int32 and zones.ndim == 2
    Hs, Ws = zones.shape
    if values is None:
        values = np.empty((0, Hs, Ws), np.float32)
    values = np.asarray(values)
    if values.ndim == 2:
        values = values[None]
    assert values.dtype == np.float32 and values.shape[1:] == (Hs, Ws) and values.shape[0] <= MAX_BANDS
    z = zones.ravel().astype(np.int64)
    keep = (z >= 0) & (z < Hs * Ws)
    if where is not None:
        where = np.asarray(where)
        assert where.dtype == np.uint8 and where.shape == (Hs, Ws)
        keep &= where.ravel() != 0
    return z, keep, values.reshape(values.shape[0], Hs * Ws), Hs, Ws


def zonal_stats(zones, values=None, where=None, frac_bits=16):
    """the vectorised form"""
    z, keep, vals, Hs, Ws = _inputs(zones, values, where)
    B = vals.shape[0]
    p = np.flatnonzero(keep)
    zone, inv = np.unique(z[p], return_inverse=True)
    inv = inv.reshape(-1)
    N = zone.size
    y, x = np.divmod(p, Ws) if Ws else (p, p)
    count = np.zeros(N, np.int64)
    np.add.at(count, inv, 1)
    bbox = np.empty((N, 4), np.int64)
    bbox[:, :2], bbox[:, 2:] = 2 ** 31 - 1, -1
    np.minimum.at(bbox[:, 0], inv, x)
    np.minimum.at(bbox[:, 1], inv, y)
    np.maximum.at(bbox[:, 2], inv, x)
    np.maximum.at(bbox[:, 3], inv, y)
    sum_x, sum_y = np.zeros(N, np.int64), np.zeros(N, np.int64)
    np.add.at(sum_x, inv, x)
    np.add.at(sum_y, inv, y)
    valid = np.zeros((B, N), np.int64)
    kmin = np.full((B, N), key(np.float32(np.inf)), np.uint32)
    kmax = np.full((B, N), key(np.float32(-np.inf)), np.uint32)
    vsum = np.zeros((B, N), np.int64)
    for b in range(B):
        v = vals[b][p]
        fin = np.isfinite(v)
        np.add.at(valid[b], inv[fin], 1)
        np.minimum.at(kmin[b], inv[fin], key(v[fin]))
        np.maximum.at(kmax[b], inv[fin], key(v[fin]))
        np.add.at(vsum[b], inv[fin], quantise(v[fin], frac_bits))
    return Zonal(zone.astype(np.int32), count.astype(np.int32), bbox.astype(np.int32), sum_x, sum_y, valid.astype(np.int32), unkey(kmin),
                 unkey(kmax), vsum, int(frac_bits))


def zonal_stats_loop(zones, values=None, where=None, frac_bits=16):
    """the definition, zone by zone and pixel by pixel"""
    z, keep, vals, Hs, Ws = _inputs(zones, values, where)
    B = vals.shape[0]
    ids = sorted(set(int(v) for v in z[keep]))
    N = len(ids)
    out = Zonal(np.asarray(ids, np.int32).reshape(N), np.zeros(N, np.int32), np.zeros((N, 4), np.int32), np.zeros(N, np.int64), np.zeros(N, np.int64),
                np.zeros((B, N), np.int32), np.full((B, N), np.inf, np.float32), np.full((B, N), -np.inf, np.float32), np.zeros((B, N), np.int64),
                int(frac_bits))
    for r, zid in enumerate(ids):
        pix = [int(q) for q in np.flatnonzero(keep & (z == zid))]
        xs, ys = [q % Ws for q in pix], [q // Ws for q in pix]
        out.count[r] = len(pix)
        out.bbox[r] = (min(xs), min(ys), max(xs), max(ys))
        out.sum_x[r], out.sum_y[r] = sum(xs), sum(ys)
        for b in range(B):
            fin = [vals[b][q] for q in pix if np.isfinite(vals[b][q])]
            out.valid[b, r] = len(fin)
            if fin:
                ks = [int(k) for k in key(np.asarray(fin, np.float32))]
                out.vmin[b, r], out.vmax[b, r] = fin[ks.index(min(ks))], fin[ks.index(max(ks))]
                out.vsum[b, r] = sum(int(quantise(v, frac_bits)) for v in fin)
    return out


def same(a, b):
    """the names of the fields in which two Zonal differ in dtype, shape or bits"""
    bad = []
    for name in Zonal._fields[:-1]:
        u, v = (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t) for t in (getattr(a, name), getattr(b, name)))
        if u.dtype != v.dtype or u.shape != v.shape or u.tobytes() != v.tobytes():
            bad.append(name)
    if int(a.frac_bits) != int(b.frac_bits):
        bad.append("frac_bits")
    return bad


def mean(z, band=0):
    """float64 [N]: vsum / 2^frac_bits / valid, NaN where valid == 0"""
    valid = np.asarray(z.valid[band] if not hasattr(z.valid, "cpu") else z.valid[band].cpu().numpy(), np.float64)
    total = np.asarray(z.vsum[band] if not hasattr(z.vsum, "cpu") else z.vsum[band].cpu().numpy(), np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(valid > 0, total / float(2 ** int(z.frac_bits)) / valid, np.nan)
