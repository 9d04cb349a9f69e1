"""Flood depth restated in numpy (kurosiwo_amd/scene.py: nearest_feature, shore, flood_depth; csrc/depth.hip): the exact Euclidean
nearest-feature transform by its definition and in the separable form the device computes, the shore of the water, and FwDET's depth.
Integers throughout, with floats only in the final subtraction, so the tests ask for equal bits."""
import numpy as np

FAR = 2 ** 31 - 1                     # dist2 where there is no feature, or the pixel was skipped
_BIG = np.int64(2) ** 62


def _skip(dist2, nearest, where):
    if where is not None:
        off = np.asarray(where) == 0
        dist2[off], nearest[off] = FAR, -1
    return dist2, nearest


def nearest_feature_direct(mask, where=None):
    """(dist2 int32 [H, W], nearest int32 [H, W]) by the definition, O(pixels x features): dist2[p] = the minimum over the features q
    (mask != 0) of (yp - yq)^2 + (xp - xq)^2, nearest[p] = the smallest linear index y * W + x among the features that attain it;
    (FAR, -1) without a feature, and where `where` is given and zero"""
    mask = np.asarray(mask)
    H, W = mask.shape
    fy, fx = np.nonzero(mask)                                       # row-major: in ascending linear index
    dist2, nearest = np.full((H, W), FAR, np.int32), np.full((H, W), -1, np.int32)
    if len(fy):
        fy, fx = fy.astype(np.int64), fx.astype(np.int64)
        xs = np.arange(W, dtype=np.int64)
        for y in range(H):                                          # a row at a time: [W, features]
            d = (y - fy)[None, :] ** 2 + (xs[:, None] - fx[None, :]) ** 2
            k = d.argmin(axis=1)                                    # the first minimum: the smallest index
            dist2[y] = d[xs, k]
            nearest[y] = fy[k] * W + fx[k]
    return _skip(dist2, nearest, where)


def nearest_in_column(mask):
    """near_y int32 [H, W]: the row of the nearest feature in the pixel's column, the smaller row when the one above and the one
    below are equally far, -1 in a column without one.  All columns at once: a running maximum down, a running minimum up."""
    mask = np.asarray(mask) != 0
    H, W = mask.shape
    rows = np.broadcast_to(np.arange(H, dtype=np.int64)[:, None], (H, W))
    above = np.maximum.accumulate(np.where(mask, rows, -1), axis=0)
    below = np.minimum.accumulate(np.where(mask, rows, _BIG)[::-1], axis=0)[::-1]
    take_above = (above >= 0) & ((below == _BIG) | (rows - above <= below - rows))
    return np.where(take_above, above, np.where(below == _BIG, -1, below)).astype(np.int32)


def nearest_from_columns(near_y, where=None):
    """(dist2, nearest) from near_y: for pixel (y, x) the lexicographic minimum of ((x - i)^2 + (y - near_y[y, i])^2,
    near_y[y, i] * W + i) over the columns i with near_y[y, i] >= 0, by brute force over all columns"""
    near_y = np.asarray(near_y).astype(np.int64)
    H, W = near_y.shape
    dist2, nearest = np.full((H, W), FAR, np.int32), np.full((H, W), -1, np.int32)
    xs = np.arange(W, dtype=np.int64)
    for y in range(H):
        cols = np.flatnonzero(near_y[y] >= 0)
        if not len(cols):
            continue
        ny = near_y[y, cols]
        cost = (xs[:, None] - cols[None, :]) ** 2 + ((y - ny) ** 2)[None, :]
        index = ny * W + cols
        least = cost.min(axis=1)
        dist2[y] = least
        nearest[y] = np.where(cost == least[:, None], index[None, :], _BIG).min(axis=1)
    return _skip(dist2, nearest, where)


def nearest_feature(mask, where=None):
    """the separable form: nearest_in_column, then nearest_from_columns.  Exact: a feature of column i at minimum distance from
    (y, x) is a nearest feature of its column to row y, and of the two column ties the smaller row has the smaller index."""
    return nearest_from_columns(nearest_in_column(mask), where)


def in_set(classes, select):
    return np.isin(np.asarray(classes), np.asarray(list(select), dtype=np.int64))


def shore(classes, dem, water=(1, 2), invalid_class=3):
    """uint8 [H, W]: 1 where the pixel is water, its DEM is finite and some 4-edge neighbour inside the scene is valid (not
    invalid_class) and not water; a scene border or an invalid neighbour makes no shore"""
    classes = np.asarray(classes)
    wet = in_set(classes, water)
    dry = np.pad(~wet & (classes != invalid_class), 1, constant_values=False)      # outside the scene: nothing
    beside = dry[:-2, 1:-1] | dry[2:, 1:-1] | dry[1:-1, :-2] | dry[1:-1, 2:]
    return (wet & np.isfinite(np.asarray(dem)) & beside).astype(np.uint8)


def flood_depth(classes, dem, water=(1, 2), invalid_class=3):
    """(depth float32, wse float32, dist2 int32): depth, by the first rule that matches, NaN where the pixel is not valid, +0 where
    it is valid and not water, NaN where it is water and the scene has no shore or its DEM is not finite, else
    max(dem[nearest] - dem, +0) in one float32 subtraction; wse = dem[nearest] at a water pixel with a shore in the scene, else NaN;
    nearest = the transform of the shore over the water pixels"""
    classes, dem = np.asarray(classes), np.asarray(dem, dtype=np.float32)
    wet = in_set(classes, water)
    dist2, nearest = nearest_feature(shore(classes, dem, water, invalid_class), where=wet.astype(np.uint8))
    found = wet & (nearest >= 0)
    level = np.where(found, dem.ravel()[np.maximum(nearest, 0)], np.float32(np.nan)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        diff = (level - dem).astype(np.float32)
        deep = np.where(diff > 0, diff, np.float32(0.0)).astype(np.float32)
    depth = np.where(wet, np.where(found & np.isfinite(dem), deep, np.float32(np.nan)), np.float32(0.0)).astype(np.float32)
    depth[classes == invalid_class] = np.nan
    return depth, level, dist2


# hand-made ties, each decided for the smallest index
TIES = {
    # name: (features (y, x), the pixel, its nearest feature, dist2) on a 7 x 7 map
    "left_and_right": (((3, 1), (3, 5)), (3, 3), (3, 1), 4),
    "above_and_below": (((1, 3), (5, 3)), (3, 3), (1, 3), 4),
    "diamond": (((1, 3), (3, 1), (3, 5), (5, 3)), (3, 3), (1, 3), 4),
}


def tie_map(name, H=7, W=7, y0=0, x0=0):
    m = np.zeros((H, W), np.uint8)
    for y, x in TIES[name][0]:
        m[y0 + y, x0 + x] = 1
    return m
