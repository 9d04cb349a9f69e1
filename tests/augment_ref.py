"""TEST INFRASTRUCTURE: float64 oracle of the augmentation views (kurosiwo_amd/augment.py, csrc/augment.hip), written pixel formula
by pixel formula from the statement of the feature, with Python integers for every index:

  output column dx of a crop of width w:  q = dx*w, sx = q // 224, r = q % 224, fx = max(0, r + w - 224) / w;  sx >= w-1 -> sx = w-1,
  fx = 0;  rows alike;  value = horizontal two-tap blend on both source rows, then the vertical blend;  every tap is clamped to
  [0, clamp] with NaN -> clamp first (clamp < 0 / None: taps as they are);  flips act on the resized tile;  (v - mean) / std last.
  Masks: sx = min(dx*w // 224, w-1).

The taps are fp32 numbers; the oracle blends them in float64 with the exact rational coefficient, so what separates it from the
fp32 implementations is their own rounding: fx (one rounding), 1 - fx, two products and a sum per pass, two passes, subtract, divide
-- a handful of fp32 roundings on values no larger than max|ref|, hence the bound TOL_ULPS * 2^-24 * max|ref|."""
import numpy as np

TILE = 224
TOL_ULPS = 8


def tolerance(ref):
    return TOL_ULPS * 2.0 ** -24 * float(np.max(np.abs(ref)))


def area_taps(n, size=TILE):
    """[(first tap, second tap, weight of the second tap as float64)] for every output position"""
    out = []
    for d in range(size):
        q = d * n
        s, r = q // size, q % size
        f = max(0, r + n - size) / n
        if s >= n - 1:
            s, f = n - 1, 0.0
        out.append((s, min(s + 1, n - 1), f))
    return out


def nearest_taps(n, size=TILE):
    return [min(d * n // size, n - 1) for d in range(size)]


def prep64(x, clamp):
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    if clamp is None or clamp < 0:
        return x
    c = float(np.float32(clamp))
    return np.where(np.isnan(x), c, np.clip(x, 0.0, c))


def blend(a, b, f):
    return a if f == 0.0 else a * (1.0 - f) + b * f


def resize_ref(crop, size=TILE):
    """crop [C, h, w] float64 -> [C, size, size]"""
    C, h, w = crop.shape
    tx, ty = area_taps(w, size), area_taps(h, size)
    hor = np.empty((C, h, size))
    for d, (s, sb, f) in enumerate(tx):
        hor[:, :, d] = blend(crop[:, :, s], crop[:, :, sb], f)
    out = np.empty((C, size, size))
    for d, (s, sb, f) in enumerate(ty):
        out[:, d, :] = blend(hor[:, s, :], hor[:, sb, :], f)
    return out


def view_ref(raw, row, mean, std, clamp):
    """one sample: raw [C, 224, 224] fp32, row = (y0, x0, h, w, flip_h, flip_v) -> float64 [C, 224, 224]"""
    y0, x0, h, w, fh, fv = (int(v) for v in row)
    v = resize_ref(prep64(raw[:, y0:y0 + h, x0:x0 + w], clamp), raw.shape[-1])
    if fh:
        v = v[:, :, ::-1]
    if fv:
        v = v[:, ::-1, :]
    m = np.asarray(mean, dtype=np.float32).astype(np.float64).reshape(-1, 1, 1)
    s = np.asarray(std, dtype=np.float32).astype(np.float64).reshape(-1, 1, 1)
    return (v - m) / s


def views_ref(raw, rows, mean, std, clamp):
    return np.stack([view_ref(raw[b], rows[b], mean, std, clamp) for b in range(raw.shape[0])])


def mask_ref(mask, row):
    """mask [224, 224] of any dtype -> its nearest-neighbour view (bit-exact by construction)"""
    y0, x0, h, w, fh, fv = (int(v) for v in row)
    size = mask.shape[-1]
    ty, tx = nearest_taps(h, size), nearest_taps(w, size)
    out = np.empty_like(mask)
    for oy in range(size):
        sy = ty[size - 1 - oy if fv else oy]
        for ox in range(size):
            sx = tx[size - 1 - ox if fh else ox]
            out[oy, ox] = mask[y0 + sy, x0 + sx]
    return out


def raw_tiles(seed, B, C, clamp=0.15):
    """raw backscatter-like fp32 tiles with NaN no-data, negatives and values above the clamp"""
    rng = np.random.default_rng(seed)
    x = rng.gamma(2.0, clamp / 4, size=(B, C, TILE, TILE)).astype(np.float32)
    u = rng.random(x.shape)
    x[u < 0.02] = np.nan
    x[(u > 0.02) & (u < 0.03)] = -0.003
    x[(u > 0.03) & (u < 0.04)] = 0.9
    return x


def boxes(seed, B):
    """int32 [B, 6] rows: the special boxes first (identity, 1 x 1, full height x k, a corner box), both flip states, then random"""
    rng = np.random.default_rng(seed)
    rows = [(0, 0, 224, 224, 0, 0), (100, 37, 1, 1, 1, 0), (0, 50, 224, 77, 1, 0), (224 - 61, 224 - 90, 61, 90, 0, 1),
            (0, 0, 112, 112, 1, 1), (3, 0, 100, 224, 0, 0), (0, 0, 224, 224, 1, 1)]
    while len(rows) < B:
        h, w = int(rng.integers(1, 225)), int(rng.integers(1, 225))
        rows.append((int(rng.integers(0, 225 - h)), int(rng.integers(0, 225 - w)), h, w, int(rng.integers(2)), int(rng.integers(2))))
    return np.array(rows[:B], dtype=np.int32)
