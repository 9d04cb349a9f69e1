"""Whole-scene inference: a trained model over a raster larger than its 224 x 224 tiles (csrc/scene.hip).

The scene's rasters live on the device.  `predict_scene` walks a product grid of overlapping windows in batches: one
ksmi_scene_gather per input raster cuts and normalises the batch's windows (the arithmetic of ksmi_sar_preprocess), the model runs
under torch.no_grad(), and one ksmi_scene_accumulate adds weight * logits onto the scene in gather form (one thread per scene pixel,
the covering windows in ascending order, no atomics: the blend is bitwise reproducible and equals the numpy slice loop of
tests/scene_ref.py).  ksmi_scene_valid marks the pixels where some input is NaN or the nodata sentinel, ksmi_scene_finalize divides
by the summed weights and takes the first maximum.  With test-time views (`tta`: VIEW_SETS) every window goes through the model once
per flipped / transposed view: ksmi_scene_gather_view cuts the windows already turned, ksmi_scene_unview turns the logits back, and
one ksmi_scene_accumulate_views per batch sums the views inside the pixel's window walk (tests/scene_tta_ref.py).  `sieve` (csrc/sieve.hip) then applies a minimum mapping unit to the class map:
connected components by a tile-local union-find and border merges, their sizes, and a vote of the large neighbours for every small
component; integers throughout, equal to the flood fill of tests/sieve_ref.py.  `polygonize` (csrc/polygon.hip) turns the class map
into boundary rings: the boundary edges of the 4-connected components, each with its successor, the rings by pointer doubling, and the
vertex lists in ring order; `polygons_geojson` writes them as GeoJSON on the host.  `flood_depth` (csrc/depth.hip) turns the class map
and a DEM into water depth: the shore pixels, the exact Euclidean nearest-feature transform of the shore (`nearest_feature`: a column
pass and a row pass, integers throughout, equal to tests/depth_ref.py) and one subtraction.  `zonal_stats` (csrc/zonal.hip) reduces value
rasters per zone of a zone raster -- pixel count, bounding box, coordinate sums and per band the finite count, the extremes under a
total order and a fixed-point sum; integers and min / max only, equal to tests/zonal_ref.py -- and `component_stats` keys it by the
component labels, so that the depth and the scores meet the polygons: `polygons_geojson(..., attributes=)` joins the rows to the
features by label.  `zonal_quantiles` (csrc/quantile.hip) sorts a band's finite values per zone -- 64-bit composites of row and value
key through a stable radix sort, equal to tests/quantile_ref.py -- and selects percentiles on the sorted order; `zonal_sorted` hands
out the sorted segments themselves and `component_quantiles` keys the percentiles by the component labels.  `rasterize_zones`
(csrc/zones.hip) makes the zone raster of a vector layer -- the scanline crossings of the polygons' edges, sorted by the same radix
sort, paired into spans and written with an integer minimum, equal to tests/zones_ref.py -- from the edge table `zone_edges` or
`zones_from_geojson` build on the host.  Everything runs on the
current stream; nothing synchronises but the three counts (edges, rings, vertices) that `polygonize` reads to size its buffers, the
one count (zones) that `zonal_stats` and `zonal_quantiles` read to size their tables and the one count (crossings) that
`rasterize_zones` reads."""
import gc
import math
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .runtime import require_gpu, stream_ptr

MAX_CLASSES = 8                   # SCENE_MAX_K of csrc/scene.hip
LABEL_TILE = (16, 64)             # (LT_H, LT_W) of csrc/sieve.hip: the tile one workgroup labels in LDS
SCAN_TILE = 2048                  # SCAN_TILE of csrc/polygon.hip: the elements one workgroup scans
MAX_POLYGON_PIXELS = 2 ** 29 - 1  # edge ids 4 * p + s and the edge count fit int32
MAX_EDT_SIDE = 32767              # rows and columns of a scene to transform: 2 * 32766^2 < 2^31 - 1
EDT_FAR = 2 ** 31 - 1             # dist2 where there is no feature, or the pixel was skipped
EDT_COLUMN_TILE = 64              # COL_MIN_TILE of csrc/depth.hip: the rows of a y-tile of the column pass, up to 8192 rows
EDT_ROW_WINDOW = (256, 896)       # (ROW_TILE, ROW_HALO) of csrc/depth.hip: the pixels of a workgroup, the columns staged either side
Rings = namedtuple("Rings", "label ring_id start area2 verts")
MAX_ZONAL_BANDS = 8               # ZN_MAX_B of csrc/zonal.hip
ZONAL_BLOCK = (4096, 64)          # (ZN_PER_BLOCK, ZN_SLOTS) of csrc/zonal.hip: the pixels of a workgroup, the zones it combines in LDS
Zonal = namedtuple("Zonal", "zone count bbox sum_x sum_y valid vmin vmax vsum frac_bits")
MAX_PERCENTILES = 16              # QT_MAX_P of csrc/quantile.hip
QUANTILE_TILE = 4096              # QT_TILE of csrc/quantile.hip: the composites one workgroup counts and scatters in a radix pass
ZonalQuantiles = namedtuple("ZonalQuantiles", "zone valid lower higher percentiles")
QUANTILE_METHODS = ("linear", "lower", "higher", "midpoint", "nearest")
MAX_ZONE_SIDE = 32767             # ZR_MAX_SIDE of csrc/zones.hip: a scanline and a column each fit 15 bits of a crossing's composite
MAX_ZONE_COORD = 3 * 32767 * 256  # ZR_MAX_COORD of csrc/zones.hip: vertices in 1/256 pixel; every product of the rule stays under 2^53
ZoneEdges = namedtuple("ZoneEdges", "edges feature count")
SCORES = {None: None, "logits": 0, "softmax": 1}
# test-time view sets, in ascending code; a code's bit 2 transposes the window (first), bit 1 then flips y, bit 0 then flips x
VIEW_SETS = {"hflip": (0, 1), "flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def _views(tta):
    """predict_scene's tta -> None (no views: one pass) or the view codes in ascending order"""
    if tta is None or tta == "none":
        return None
    if isinstance(tta, str):
        if tta not in VIEW_SETS:
            raise ValueError(f'predict_scene: tta is None, "none", one of {sorted(VIEW_SETS)} or a tuple of view codes 0 .. 7, got {tta!r}')
        return VIEW_SETS[tta]
    codes = list(tta) if isinstance(tta, (tuple, list)) else None
    if not codes or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 7 for v in codes) \
            or len(set(int(v) for v in codes)) != len(codes):
        raise ValueError(f"predict_scene: tta as a tuple holds distinct view codes 0 .. 7, at least one, got {tta!r}")
    return tuple(sorted(int(v) for v in codes))


def _axis(L, win, s):
    if not 1 <= s <= win:
        raise ValueError(f"window_grid: 1 <= stride <= window, got stride {s} for window {win}")
    if L < 1:
        raise ValueError(f"window_grid: a scene of {L} pixels")
    if L < win:
        return [0]
    o = list(range(0, L - win + 1, s))
    if o[-1] + win != L:
        o.append(L - win)                # the last window ends flush with the border
    return o


def window_grid(Hs, Ws, h, w, sy, sx):
    """(ys, xs): int32 row and column origins of the product grid of h x w windows at strides (sy, sx) over an Hs x Ws scene; per
    axis range(0, L - win + 1, stride) plus L - win when the last window would not end at the border, [0] when L < win."""
    return np.asarray(_axis(Hs, h, sy), np.int32), np.asarray(_axis(Ws, w, sx), np.int32)


def blend_weights(h, w, kind="hann"):
    """[h, w] float32: "uniform" = ones; "hann" = float32(a[y] * a[x]), a[i] = 0.5 - 0.5 cos(2 pi (i + 0.5) / L) in float64 (the
    half-sample shift keeps every weight strictly positive), the product taken in float64 and rounded once."""
    if h < 1 or w < 1:
        raise ValueError("blend_weights: h, w >= 1")
    if kind == "uniform":
        return np.ones((h, w), np.float32)
    if kind != "hann":
        raise ValueError(f'blend_weights: kind is "uniform" or "hann", got {kind!r}')
    a = lambda L: 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(L, dtype=np.float64) + 0.5) / L)
    return (a(h)[:, None] * a(w)[None, :]).astype(np.float32)


def _nodata(v):
    return float("nan") if v is None else float(v)


def _check_raster(r, name):
    require_gpu(r)
    if r.dtype != torch.float32 or r.dim() != 3 or not r.is_contiguous() or r.shape[0] < 1:
        raise ValueError(f"{name}: a contiguous float32 tensor [C, Hs, Ws]")


# ---------------------------------------------------------------------------------------------------- thin wrappers of the C-ABI
def scene_valid(raster, nodata=None, valid=None):
    """ksmi_scene_valid: valid uint8 [Hs, Ws] = (valid given: valid &) no channel of raster [C, Hs, Ws] is NaN or equal to nodata"""
    _check_raster(raster, "scene_valid")
    C, Hs, Ws = raster.shape
    first = valid is None
    if first:
        valid = torch.empty((Hs, Ws), dtype=torch.uint8, device=raster.device)
    elif valid.dtype != torch.uint8 or valid.shape != (Hs, Ws) or valid.device != raster.device or not valid.is_contiguous():
        raise ValueError("scene_valid: valid is a contiguous uint8 tensor [Hs, Ws] on the raster's device")
    _lib.check(_lib.load().ksmi_scene_valid(raster.data_ptr(), C, Hs * Ws, _nodata(nodata), valid.data_ptr(), 1 if first else 0, stream_ptr()),
               "scene_valid")
    return valid


def _check_grid(ys, xs, name):
    for o in (ys, xs):
        require_gpu(o)
        if o.dtype != torch.int32 or o.dim() != 1 or not o.is_contiguous() or o.numel() < 1:
            raise ValueError(f"{name}: ys and xs are contiguous int32 device vectors")


def _gather(name, raster, ys, xs, i0, n, h, w, norm, nodata, out, view=None):
    _check_raster(raster, name)
    _check_grid(ys, xs, name)
    C, Hs, Ws = raster.shape
    if out is None:
        out = torch.empty((max(n, 0), C, h, w), dtype=torch.float32, device=raster.device)
    elif out.dtype != torch.float32 or out.shape != (n, C, h, w) or out.device != raster.device or not out.is_contiguous():
        raise ValueError(f"{name}: out is a contiguous float32 tensor [n, C, h, w] on the raster's device")
    if norm is not None:
        for t in norm:
            if t.dtype != torch.float32 or t.numel() != C or t.device != raster.device or not t.is_contiguous():
                raise ValueError(f"{name}: mean, std and clamp are float32 device vectors of {C} entries")
    m, s, c = (None, None, None) if norm is None else (t.data_ptr() for t in norm)
    head = (raster.data_ptr(), C, Hs, Ws, ys.data_ptr(), ys.numel(), xs.data_ptr(), xs.numel(), i0, n, h, w, m, s, c, _nodata(nodata))
    if view is None:
        _lib.check(_lib.load().ksmi_scene_gather(*head, out.data_ptr(), stream_ptr()), name)
    else:
        _lib.check(_lib.load().ksmi_scene_gather_view(*head, int(view), out.data_ptr(), stream_ptr()), name)
    return out


def scene_gather(raster, ys, xs, i0, n, h, w, norm=None, nodata=None, out=None):
    """ksmi_scene_gather: windows i0 .. i0 + n - 1 of raster [C, Hs, Ws] as [n, C, h, w]; norm = (mean, std, clamp) float32 device
    vectors of C entries, or None for raw values (nodata -> NaN)"""
    return _gather("scene_gather", raster, ys, xs, i0, n, h, w, norm, nodata, out)


def _check_view(view, h, w, name):
    if isinstance(view, bool) or not isinstance(view, (int, np.integer)) or not 0 <= int(view) <= 7:
        raise ValueError(f"{name}: view is a code 0 .. 7 (1: flip x, 2: flip y, 4: transpose), got {view!r}")
    if int(view) & 4 and h != w:
        raise ValueError(f"{name}: a transposed view needs h == w, got {h} x {w}")


def scene_gather_view(raster, ys, xs, i0, n, h, w, view, norm=None, nodata=None, out=None):
    """ksmi_scene_gather_view: scene_gather with every [h, w] tile in view `view` (0 .. 7: bit 2 transposes first, bit 1 then flips y,
    bit 0 then flips x); view 0 gives the bits of scene_gather"""
    _check_view(view, h, w, "scene_gather_view")
    return _gather("scene_gather_view", raster, ys, xs, i0, n, h, w, norm, nodata, out, view)


def scene_unview(x, view, out=None):
    """ksmi_scene_unview: the inverse of view `view` on every [h, w] plane of the contiguous float32 device tensor x [..., h, w], out of
    place; a copy of bits.  out: a contiguous tensor of x's shape that shares no memory with it"""
    require_gpu(x)
    if x.dtype != torch.float32 or x.dim() < 2 or not x.is_contiguous() or x.shape[-1] < 1 or x.shape[-2] < 1:
        raise ValueError("scene_unview: x is a contiguous float32 tensor [..., h, w]")
    h, w = x.shape[-2:]
    _check_view(view, h, w, "scene_unview")
    if out is None:
        out = torch.empty_like(x)
    elif out.dtype != torch.float32 or out.shape != x.shape or out.device != x.device or not out.is_contiguous():
        raise ValueError("scene_unview: out is a contiguous float32 tensor of x's shape on its device")
    _lib.check(_lib.load().ksmi_scene_unview(x.data_ptr(), out.data_ptr(), x.numel() // (h * w), h, w, int(view), stream_ptr()), "scene_unview")
    return out


def scene_accumulate(logits, ys, xs, i0, weight, acc, wsum):
    """ksmi_scene_accumulate: acc [K, Hs, Ws] += weight [h, w] * logits [n, K, h, w] of windows i0 ..; wsum [Hs, Ws] += weight"""
    require_gpu(logits)
    _check_grid(ys, xs, "scene_accumulate")
    if logits.dtype != torch.float32 or logits.dim() != 4 or not logits.is_contiguous():
        raise ValueError("scene_accumulate: logits is a contiguous float32 tensor [n, K, h, w]")
    n, K, h, w = logits.shape
    if acc.dim() != 3 or acc.shape[0] != K or wsum.shape != acc.shape[1:] or weight.shape != (h, w) or any(
            t.dtype != torch.float32 or not t.is_contiguous() or t.device != logits.device for t in (weight, acc, wsum)):
        raise ValueError("scene_accumulate: float32 contiguous weight [h, w], acc [K, Hs, Ws] and wsum [Hs, Ws] on the logits' device")
    _lib.check(_lib.load().ksmi_scene_accumulate(logits.data_ptr(), ys.data_ptr(), ys.numel(), xs.data_ptr(), xs.numel(), i0, n, K, h, w,
                                                 weight.data_ptr(), acc.data_ptr(), wsum.data_ptr(), acc.shape[1], acc.shape[2], stream_ptr()),
               "scene_accumulate")


def scene_accumulate_views(logits, ys, xs, i0, weight, acc, wsum):
    """ksmi_scene_accumulate_views: scene_accumulate over logits [V, n, K, h, w], the V views of windows i0 .. in window orientation
    (after scene_unview): per scene pixel the covering windows in ascending order and for each the views in ascending order"""
    require_gpu(logits)
    _check_grid(ys, xs, "scene_accumulate_views")
    if logits.dtype != torch.float32 or logits.dim() != 5 or not logits.is_contiguous():
        raise ValueError("scene_accumulate_views: logits is a contiguous float32 tensor [V, n, K, h, w]")
    V, n, K, h, w = logits.shape
    if acc.dim() != 3 or acc.shape[0] != K or wsum.shape != acc.shape[1:] or weight.shape != (h, w) or any(
            t.dtype != torch.float32 or not t.is_contiguous() or t.device != logits.device for t in (weight, acc, wsum)):
        raise ValueError("scene_accumulate_views: float32 contiguous weight [h, w], acc [K, Hs, Ws] and wsum [Hs, Ws] on the logits' device")
    _lib.check(_lib.load().ksmi_scene_accumulate_views(logits.data_ptr(), V, ys.data_ptr(), ys.numel(), xs.data_ptr(), xs.numel(), i0, n, K, h, w,
                                                       weight.data_ptr(), acc.data_ptr(), wsum.data_ptr(), acc.shape[1], acc.shape[2],
                                                       stream_ptr()), "scene_accumulate_views")


def scene_finalize(acc, wsum, valid=None, score=None, invalid_class=3):
    """ksmi_scene_finalize -> (classes uint8 [Hs, Ws], scores float32 [K, Hs, Ws] or None); score: None, "logits" (the blended mean
    logits) or "softmax"; invalid pixels get `invalid_class` and NaN scores"""
    require_gpu(acc)
    if score not in SCORES:
        raise ValueError(f'scene_finalize: score is None, "logits" or "softmax", got {score!r}')
    if acc.dtype != torch.float32 or acc.dim() != 3 or not acc.is_contiguous() or wsum.dtype != torch.float32 or wsum.shape != acc.shape[1:] \
            or not wsum.is_contiguous() or wsum.device != acc.device:
        raise ValueError("scene_finalize: float32 contiguous acc [K, Hs, Ws] and wsum [Hs, Ws]")
    K, Hs, Ws = acc.shape
    if valid is not None and (valid.dtype != torch.uint8 or valid.shape != (Hs, Ws) or not valid.is_contiguous() or valid.device != acc.device):
        raise ValueError("scene_finalize: valid is a contiguous uint8 tensor [Hs, Ws]")
    cls = torch.empty((Hs, Ws), dtype=torch.uint8, device=acc.device)
    out = None if score is None else torch.empty_like(acc)
    _lib.check(_lib.load().ksmi_scene_finalize(acc.data_ptr(), wsum.data_ptr(), None if valid is None else valid.data_ptr(), K, Hs * Ws,
                                               int(invalid_class), cls.data_ptr(), None if out is None else out.data_ptr(), SCORES[score] or 0,
                                               stream_ptr()), "scene_finalize")
    return cls, out


# ---------------------------------------------------------------------------------------------------- minimum mapping unit
def _check_map(t, dtype, name, what):
    require_gpu(t)
    if t.dtype != dtype or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name}: {what} is a contiguous {str(dtype).replace('torch.', '')} device tensor [Hs, Ws]")


def label_components(classes, connectivity=4):
    """ksmi_scene_label: labels int32 [Hs, Ws], labels[p] = the smallest linear index y * Ws + x of p's component (pixels of one class
    value joined by edges, connectivity 4, or by edges and corners, 8); every class value is labelled"""
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity is 4 or 8, got {connectivity!r}")
    _check_map(classes, torch.uint8, "label_components", "classes")
    Hs, Ws = classes.shape
    labels = torch.empty((Hs, Ws), dtype=torch.int32, device=classes.device)
    if Hs * Ws:
        _lib.check(_lib.load().ksmi_scene_label(classes.data_ptr(), Hs, Ws, int(connectivity), labels.data_ptr(), stream_ptr()), "scene_label")
    return labels


def component_sizes(labels):
    """ksmi_scene_component_sizes: sizes int32 [Hs, Ws], at a root index (labels[p] == p) the pixels of that component, 0 elsewhere"""
    _check_map(labels, torch.int32, "component_sizes", "labels")
    sizes = torch.empty_like(labels)
    _lib.check(_lib.load().ksmi_scene_component_sizes(labels.data_ptr(), labels.numel(), sizes.data_ptr(), stream_ptr()), "scene_component_sizes")
    return sizes


def sieve(classes, mmu, connectivity=4, invalid_class=3, num_classes=4, passes=1):
    """Minimum mapping unit -> (classes uint8 [Hs, Ws], removed int32 device tensor [1]).

    One pass, judged on its input map alone: a component (label_components at `connectivity`) is small when it has fewer than `mmu`
    pixels and its class is not `invalid_class`.  Every pixel of a small component lets each of its 4 edge neighbours inside the scene
    vote for its class when that neighbour lies in another component that is neither small nor invalid; the component takes the class
    with the most votes (the lowest class on a tie) or, without a vote, keeps its own.  The invalid class (and any value >=
    num_classes) is never changed and never votes; mmu <= 1 is the identity.  passes = n repeats the pass on its own output; removed
    counts the components replaced over all passes.  The input is left alone.  Scratch: 8 + 4 * num_classes bytes per pixel."""
    if connectivity not in (4, 8):
        raise ValueError(f"sieve: connectivity is 4 or 8, got {connectivity!r}")
    if not 1 <= int(num_classes) <= MAX_CLASSES:
        raise ValueError(f"sieve: 1 <= num_classes <= {MAX_CLASSES}, got {num_classes!r}")
    if int(passes) < 1:
        raise ValueError(f"sieve: passes >= 1, got {passes!r}")
    if not 0 <= int(invalid_class) <= 255:
        raise ValueError(f"sieve: invalid_class in 0 .. 255, got {invalid_class!r}")
    _check_map(classes, torch.uint8, "sieve", "classes")
    mmu, K, Hs, Ws = int(mmu), int(num_classes), classes.shape[0], classes.shape[1]
    removed = torch.zeros(1, dtype=torch.int32, device=classes.device)
    if mmu <= 1 or Hs * Ws == 0:
        return classes.clone(), removed
    lib, st = _lib.load(), stream_ptr()
    votes = torch.empty((K, Hs, Ws), dtype=torch.int32, device=classes.device)       # only the cells at small roots are ever used
    for _ in range(int(passes)):
        labels = label_components(classes, connectivity)
        sizes = component_sizes(labels)
        out = torch.empty_like(classes)
        _lib.check(lib.ksmi_scene_sieve_vote(classes.data_ptr(), labels.data_ptr(), sizes.data_ptr(), mmu, int(invalid_class), K, Hs, Ws,
                                             votes.data_ptr(), st), "scene_sieve_vote")
        _lib.check(lib.ksmi_scene_sieve_apply(classes.data_ptr(), labels.data_ptr(), sizes.data_ptr(), votes.data_ptr(), mmu, int(invalid_class),
                                              K, Hs * Ws, out.data_ptr(), removed.data_ptr(), st), "scene_sieve_apply")
        classes = out
    return classes, removed


# ---------------------------------------------------------------------------------------------------- flood depth
def _check_edt_map(t, dtype, name, what, like=None):
    """the checks of _check_map that need no device, and the size limit of the transform; the caller ends with require_gpu"""
    if not torch.is_tensor(t) or t.dtype != dtype or t.dim() != 2 or not t.is_contiguous():
        raise ValueError(f"{name}: {what} is a contiguous {str(dtype).replace('torch.', '')} device tensor [Hs, Ws]")
    if t.shape[0] > MAX_EDT_SIDE or t.shape[1] > MAX_EDT_SIDE:
        raise ValueError(f"{name}: at most {MAX_EDT_SIDE} rows and {MAX_EDT_SIDE} columns (squared distances are int32), got {tuple(t.shape)}")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError(f"{name}: {what} has the shape and the device of the map")


def nearest_feature_columns(mask):
    """ksmi_scene_edt_cols: near_y int32 [Hs, Ws], the row of the nearest feature (mask != 0) in the pixel's column, the smaller row
    when the one above and the one below are equally far, -1 in a column without one"""
    _check_edt_map(mask, torch.uint8, "nearest_feature_columns", "mask")
    require_gpu(mask)
    Hs, Ws = mask.shape
    near_y = torch.empty((Hs, Ws), dtype=torch.int32, device=mask.device)
    if Hs * Ws:
        _lib.check(_lib.load().ksmi_scene_edt_cols(mask.data_ptr(), Hs, Ws, near_y.data_ptr(), stream_ptr()), "scene_edt_cols")
    return near_y


def nearest_feature_rows(near_y, where=None):
    """ksmi_scene_edt_rows -> (dist2 int32 [Hs, Ws], nearest int32 [Hs, Ws]) from the near_y of nearest_feature_columns: per pixel
    (y, x) the lexicographic minimum of ((x - i)^2 + (y - near_y[y, i])^2, near_y[y, i] * Ws + i) over the columns i with a feature"""
    _check_edt_map(near_y, torch.int32, "nearest_feature_rows", "near_y")
    if where is not None:
        _check_edt_map(where, torch.uint8, "nearest_feature_rows", "where", like=near_y)
    require_gpu(near_y)
    Hs, Ws = near_y.shape
    dist2, nearest = torch.empty_like(near_y), torch.empty_like(near_y)
    if Hs * Ws:
        _lib.check(_lib.load().ksmi_scene_edt_rows(near_y.data_ptr(), None if where is None else where.data_ptr(), Hs, Ws, dist2.data_ptr(),
                                                   nearest.data_ptr(), stream_ptr()), "scene_edt_rows")
    return dist2, nearest


def nearest_feature(mask, where=None):
    """The exact Euclidean nearest-feature transform -> (dist2 int32 [Hs, Ws], nearest int32 [Hs, Ws]).

    A non-zero mask[p] (uint8 [Hs, Ws]) marks a feature; pixels are p = y * Ws + x.  dist2[p] = the minimum over the features q of
    (yp - yq)^2 + (xp - xq)^2; nearest[p] = the smallest linear index among the features at that distance (p itself at a feature).
    Without a feature in the scene dist2 = 2^31 - 1 (EDT_FAR) and nearest = -1.  where (uint8 [Hs, Ws]): a pixel where it is zero is
    skipped and holds those two values; the others hold what they hold without it.  At most 32767 rows and 32767 columns, so every
    squared distance fits int32 below EDT_FAR.  Two launches (columns, then rows), integers throughout, nothing read on the host;
    an empty scene gives empty tensors without a launch.  Scratch: 4 B per pixel.  The row pass walks outward from the pixel until
    the squared column offset passes the best distance: its cost grows with the distance to the nearest feature."""
    _check_edt_map(mask, torch.uint8, "nearest_feature", "mask")
    if where is not None:
        _check_edt_map(where, torch.uint8, "nearest_feature", "where", like=mask)
    require_gpu(mask)
    return nearest_feature_rows(nearest_feature_columns(mask), where)


def _check_depth_maps(classes, dem, water, invalid_class, name):
    _check_edt_map(classes, torch.uint8, name, "classes")
    _check_edt_map(dem, torch.float32, name, "dem", like=classes)
    if not 0 <= int(invalid_class) <= 255:
        raise ValueError(f"{name}: invalid_class in 0 .. 255, got {invalid_class!r}")
    mask = _select_mask(water, name)
    require_gpu(classes)
    return mask


def select_classes(classes, select=(1, 2)):
    """ksmi_scene_select: uint8 [Hs, Ws], 1 where the pixel's class is in `select` (values 0 .. 62), else 0"""
    mask = _select_mask(select, "select_classes")
    _check_map(classes, torch.uint8, "select_classes", "classes")
    out = torch.empty_like(classes)
    _lib.check(_lib.load().ksmi_scene_select(classes.data_ptr(), mask, classes.numel(), out.data_ptr(), stream_ptr()), "scene_select")
    return out


def shore(classes, dem, water=(1, 2), invalid_class=3):
    """ksmi_scene_shore: uint8 [Hs, Ws], 1 at a water pixel (class in `water`) whose DEM is finite and which has a 4-edge neighbour
    inside the scene that is neither water nor `invalid_class`; the scene border and invalid neighbours make no shore"""
    mask = _check_depth_maps(classes, dem, water, invalid_class, "shore")
    Hs, Ws = classes.shape
    out = torch.empty_like(classes)
    if Hs * Ws:
        _lib.check(_lib.load().ksmi_scene_shore(classes.data_ptr(), dem.data_ptr(), mask, int(invalid_class), Hs, Ws, out.data_ptr(), stream_ptr()),
                   "scene_shore")
    return out


def flood_depth(classes, dem, water=(1, 2), invalid_class=3, return_wse=False, distance=False):
    """Flood depth from a class map and a DEM on its grid -> depth float32 [Hs, Ws] (then wse, then dist2, where asked for).

    The three steps of FwDET (Cohen et al. 2018): the DEM at the flood boundary; every flooded pixel takes the elevation of its
    nearest boundary pixel (Euclidean allocation: `nearest_feature` of `shore` over the water pixels, the smallest index on a tie);
    minus the DEM, clamped at zero.  water(p): the class is in `water` (values 0 .. 62); valid(p): it is not `invalid_class`;
    shore(p): water, a finite DEM, and a 4-edge neighbour inside the scene that is valid and not water -- a scene border or an invalid
    neighbour makes no shore, as the water's real edge is not seen there (FwDET v2).  depth[p], by the first rule that matches: NaN
    where p is not valid; +0.0 where p is valid and not water; NaN where p is water and the scene has no shore or dem[p] is not
    finite; else max(dem[nearest[p]] - dem[p], +0.0) in one float32 subtraction.  return_wse: also the water surface elevation,
    dem[nearest[p]] at a water pixel with a shore in the scene, NaN elsewhere.  distance: also dist2 int32 of the shore transform,
    2^31 - 1 off the water.  The allocation is global: a pixel may take its level from the shore of another water body, as Euclidean
    allocation does in the published method.  dem: float32 [Hs, Ws] in the unit the depth is wanted in, NaN where unknown.
    Scratch: 14 B per pixel (shore, water, near_y, dist2, nearest) next to the outputs."""
    mask = _check_depth_maps(classes, dem, water, invalid_class, "flood_depth")
    Hs, Ws = classes.shape
    edge, wet = shore(classes, dem, water, invalid_class), select_classes(classes, water)
    dist2, nearest = nearest_feature(edge, where=wet)
    depth = torch.empty_like(dem)
    wse = torch.empty_like(dem) if return_wse else None
    _lib.check(_lib.load().ksmi_scene_depth(classes.data_ptr(), dem.data_ptr(), nearest.data_ptr(), mask, int(invalid_class), Hs * Ws,
                                            depth.data_ptr(), None if wse is None else wse.data_ptr(), stream_ptr()), "scene_depth")
    out = (depth,) + ((wse,) if return_wse else ()) + ((dist2,) if distance else ())
    return out[0] if len(out) == 1 else out


# ---------------------------------------------------------------------------------------------------- polygon output
def _check_vec(t, name, what, dtype=torch.int32):
    require_gpu(t)
    if t.dtype != dtype or t.dim() != 1 or not t.is_contiguous():
        raise ValueError(f"{name}: {what} is a contiguous {str(dtype).replace('torch.', '')} device vector")


def _select_mask(select, name):
    mask = 0
    for c in select:
        if int(c) != c or not 0 <= int(c) <= 62:
            raise ValueError(f"{name}: select holds class values 0 .. 62, got {c!r}")
        mask |= 1 << int(c)
    return mask


def _scan(x, out, name):
    """exclusive scan of the int32 device vector x into out (x itself: in place) -> the total, an int64 device tensor [1]"""
    n = x.numel()
    total = torch.zeros(1, dtype=torch.int64, device=x.device)
    if n:
        lib = _lib.load()
        need = int(lib.ksmi_scan_i32_scratch(n))
        scratch = torch.empty(max(need, 1), dtype=torch.int32, device=x.device)
        _lib.check(lib.ksmi_scan_i32(x.data_ptr(), out.data_ptr(), n, total.data_ptr(), scratch.data_ptr(), need, stream_ptr()), name)
    return total


def scan_i32(x, out=None):
    """ksmi_scan_i32 -> (prefix int32 [n], total int64 device tensor [1]): prefix[i] = x[0] + ... + x[i - 1], total = the sum of all.
    Every prefix and the total must fit int32.  out: where the prefix goes (x itself: in place); by default a new tensor, and x is
    left alone.  Tiles of SCAN_TILE elements, three passes, as deep as n needs."""
    _check_vec(x, "scan_i32", "x")
    if x.numel() > 2 ** 31 - 1:
        raise ValueError("scan_i32: at most 2^31 - 1 elements")
    if out is None:
        out = torch.empty_like(x)
    else:
        _check_vec(out, "scan_i32", "out")
        if out.shape != x.shape or out.device != x.device:
            raise ValueError("scan_i32: out has the length and the device of x")
    return out, _scan(x, out, "scan_i32")


def _check_polygon_maps(classes, labels, name):
    _check_map(classes, torch.uint8, name, "classes")
    if labels is not None:
        _check_map(labels, torch.int32, name, "labels")
        if labels.shape != classes.shape or labels.device != classes.device:
            raise ValueError(f"{name}: labels has the shape and the device of classes")
    if classes.numel() > MAX_POLYGON_PIXELS:
        raise ValueError(f"{name}: at most 2^29 - 1 pixels (edge ids are int32), got {classes.numel()}")


def _boundary_edges(classes, labels, mask):
    """(eid, succ, E) -- two host-visible launches around one scan; E is the one value read back"""
    Hs, Ws = classes.shape
    dev = classes.device
    lib, st = _lib.load(), stream_ptr()
    empty = lambda: torch.empty(0, dtype=torch.int32, device=dev)
    if Hs * Ws == 0:
        return empty(), empty(), 0
    offsets = torch.empty(Hs * Ws, dtype=torch.int32, device=dev)
    _lib.check(lib.ksmi_scene_edge_count(classes.data_ptr(), labels.data_ptr(), mask, Hs, Ws, offsets.data_ptr(), st), "scene_edge_count")
    E = int(_scan(offsets, offsets, "scan_i32").item())             # the first of the three host reads
    if E == 0:
        return empty(), empty(), 0
    eid, succ = torch.empty(E, dtype=torch.int32, device=dev), torch.empty(E, dtype=torch.int32, device=dev)
    _lib.check(lib.ksmi_scene_edge_emit(classes.data_ptr(), labels.data_ptr(), mask, Hs, Ws, offsets.data_ptr(), E, eid.data_ptr(),
                                        succ.data_ptr(), st), "scene_edge_emit")
    return eid, succ, E


def boundary_edges(classes, labels, select=(1, 2)):
    """ksmi_scene_edge_count, ksmi_scan_i32, ksmi_scene_edge_emit -> (eid int32 [E], succ int32 [E]).

    Side s of pixel p = y * Ws + x (0 top, 1 right, 2 bottom, 3 left, walked clockwise on screen with the pixel on the right) is a
    boundary edge when p's class is in `select` (values 0 .. 62) and the pixel across it is outside the scene or has another label.
    eid[k] = 4 * p + s in ascending order; succ[k] = the index of the next edge of the ring: at the edge's end, turn left when the pixel
    ahead-left has p's label, else go straight when the pixel ahead-right has it, else turn right around p.  labels: the
    4-connectivity labels of label_components(classes, 4)."""
    mask = _select_mask(select, "boundary_edges")
    _check_polygon_maps(classes, labels, "boundary_edges")
    if labels is None:
        raise ValueError("boundary_edges: labels is the int32 map of label_components(classes, 4)")
    eid, succ, _ = _boundary_edges(classes, labels, mask)
    return eid, succ


def trace_rings(succ):
    """ksmi_scene_ring_trace -> (ring_min int32 [E], rank int32 [E]): for a permutation succ, the smallest index on k's cycle and the
    number of successor steps from it to k.  Pointer doubling, 2 * ceil(log2(E)) rounds whatever the rings look like; 16 B of scratch
    per edge."""
    _check_vec(succ, "trace_rings", "succ")
    E = succ.numel()
    if E > 2 ** 31 - 1:
        raise ValueError("trace_rings: at most 2^31 - 1 edges")
    ring_min, rank = torch.empty_like(succ), torch.empty_like(succ)
    if E:
        scratch = torch.empty(4 * E, dtype=torch.int32, device=succ.device)
        _lib.check(_lib.load().ksmi_scene_ring_trace(succ.data_ptr(), E, 3, ring_min.data_ptr(), rank.data_ptr(), scratch.data_ptr(), 4 * E,
                                                     stream_ptr()), "scene_ring_trace")
    return ring_min, rank


def polygonize(classes, select=(1, 2), labels=None):
    """The boundary rings of a class map -> Rings(label, ring_id, start, area2, verts), device tensors.

    One ring per boundary of every 4-connected component whose class is in `select` (values 0 .. 62), in ascending ring id:
      label   int32 [R]      the component: the smallest linear index y * Ws + x of its pixels (label_components(classes, 4))
      ring_id int32 [R]      the smallest edge id 4 * p + s of the ring; a component's exterior ring has id 4 * label, its smallest
      start   int32 [R + 1]  ring r has the vertices verts[start[r]:start[r + 1]]
      area2   int64 [R]      the sum of x0 * y1 - x1 * y0 over the ring's edges: positive for the exterior ring, negative for a hole;
                             over a component twice its pixel count
      verts   int32 [V, 2]   (x, y) pixel corners, x right and y down, clockwise on screen around the component (holes the other way),
                             collinear vertices dropped, the first vertex not repeated
    Nothing selected: empty tensors and start == [0].  labels, if given, must be the 4-connectivity labels of `classes`
    (label_components(classes, 4)): with 8-connectivity labels a ring would touch itself at corners.  At most 2^29 - 1 pixels.  Three
    integers are read on the host (edges, rings, vertices) to size the buffers; scratch: 8 B per pixel and 48 B per boundary edge."""
    mask = _select_mask(select, "polygonize")
    _check_polygon_maps(classes, labels, "polygonize")
    Hs, Ws = classes.shape
    dev = classes.device
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    if labels is None and Hs * Ws:
        labels = label_components(classes, 4)
    eid, succ, E = _boundary_edges(classes, labels, mask)
    if E == 0:
        return Rings(i32(0), i32(0), torch.zeros(1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int64, device=dev),
                     torch.empty((0, 2), dtype=torch.int32, device=dev))
    lib, st = _lib.load(), stream_ptr()
    ring_min, rank = trace_rings(succ)
    ring_index = i32(E)
    _lib.check(lib.ksmi_scene_ring_heads(ring_min.data_ptr(), E, ring_index.data_ptr(), st), "scene_ring_heads")
    R = int(_scan(ring_index, ring_index, "scan_i32").item())           # the second host read
    ring_id, label, offset = i32(R), i32(R), i32(R)
    _lib.check(lib.ksmi_scene_ring_table(eid.data_ptr(), succ.data_ptr(), ring_min.data_ptr(), rank.data_ptr(), ring_index.data_ptr(),
                                         labels.data_ptr(), Hs * Ws, E, R, ring_id.data_ptr(), label.data_ptr(), offset.data_ptr(), st),
               "scene_ring_table")
    _scan(offset, offset, "scan_i32")                                   # lengths -> offsets in ring order; the total is E
    ordered_eid, ordered_ring, vertex_offset = i32(E), i32(E), i32(E)
    _lib.check(lib.ksmi_scene_ring_order(eid.data_ptr(), succ.data_ptr(), ring_min.data_ptr(), rank.data_ptr(), ring_index.data_ptr(),
                                         offset.data_ptr(), E, R, ordered_eid.data_ptr(), ordered_ring.data_ptr(), vertex_offset.data_ptr(), st),
               "scene_ring_order")
    V = int(_scan(vertex_offset, vertex_offset, "scan_i32").item())     # the third
    verts = torch.empty((V, 2), dtype=torch.int32, device=dev)
    start = i32(R + 1)
    area2 = torch.empty(R, dtype=torch.int64, device=dev)
    _lib.check(lib.ksmi_scene_ring_verts(ordered_eid.data_ptr(), ordered_ring.data_ptr(), vertex_offset.data_ptr(), E, R, V, Ws,
                                         verts.data_ptr(), start.data_ptr(), area2.data_ptr(), st), "scene_ring_verts")
    return Rings(label, ring_id, start, area2, verts)


def zonal_geometry(zonal, pixel_scale=None, origin=None):
    """(bbox float64 [N, 4], centroid_x float64 [N], centroid_y float64 [N]) of the rows of a Zonal, on the host, in the arithmetic of
    the vertices of polygons_geojson (ox + x * sx, oy - y * sy; scale (1, 1) and origin (0, 0) without georeferencing): bbox = [west,
    south, east, north] from the pixel corners x0, y1 + 1, x1 + 1, y0 of the integer bbox; the centroid is the mean pixel centre,
    (sum_x + count / 2) / count and (sum_y + count / 2) / count in float64, through the same map."""
    count, box, sum_x, sum_y = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in (zonal.count, zonal.bbox, zonal.sum_x, zonal.sum_y))
    sx, sy = (1.0, 1.0) if pixel_scale is None else (float(pixel_scale[0]), float(pixel_scale[1]))
    ox, oy = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    n = count.astype(np.float64)
    bbox = np.empty((count.shape[0], 4), np.float64)
    bbox[:, 0] = ox + box[:, 0].astype(np.float64) * sx
    bbox[:, 1] = oy - (box[:, 3].astype(np.float64) + 1.0) * sy
    bbox[:, 2] = ox + (box[:, 2].astype(np.float64) + 1.0) * sx
    bbox[:, 3] = oy - box[:, 1].astype(np.float64) * sy
    return bbox, ox + (sum_x.astype(np.float64) + n / 2.0) / n * sx, oy - (sum_y.astype(np.float64) + n / 2.0) / n * sy


def polygons_geojson(rings, classes, pixel_scale=None, origin=None, attributes=None):
    """A GeoJSON FeatureCollection (a dict) of the rings of `polygonize`, built on the host.

    One Polygon feature per component in ascending label: its exterior ring first, then its holes in ascending ring id, each closed by
    repeating its first vertex.  Coordinates are [ox + x * sx, oy - y * sy] in float64 with pixel_scale = (sx, sy) and origin = (ox, oy)
    as geotiff.read returns them (the model position of the corner of pixel (0, 0)); without georeferencing the scale is (1, 1) and
    the origin (0, 0).  The ring table walks clockwise on screen and a north-up map keeps that sense, so every ring is written from its
    first vertex against the walk: exterior rings counter-clockwise and holes clockwise, as RFC 7946 asks.  Properties:
    "class" (the class value of the component), "pixels" (the component's pixel count: the sum of its rings' area2 over 2) and "area"
    (pixels * sx * sy; null without a pixel scale).  No "crs" member is written: the coordinates are in the raster's own coordinate
    reference system, not necessarily the WGS 84 of RFC 7946, and whoever reads the file must know it.  classes: the map the rings
    were traced on, a tensor or an array.

    attributes: None (the output above, byte for byte), a Zonal whose `zone` values are component labels (component_stats), or a pair
    (Zonal, {property name: one value per row}).  Rows are joined to features by label (both are in ascending label).  A feature
    with a row gets a GeoJSON "bbox" member [west, south, east, north] (zonal_geometry: the pixel corners of the integer bbox through
    the vertices' arithmetic), the properties "centroid_x" and "centroid_y" (the mean pixel centre, in map coordinates) and every
    named property from its row; a feature without a row gets null for all of these properties and no "bbox"."""
    extra, names, row_of = None, (), {}
    if attributes is not None:
        zonal, extra = attributes if isinstance(attributes, tuple) and not hasattr(attributes, "_fields") else (attributes, {})
        zone = (zonal.zone.cpu().numpy() if torch.is_tensor(zonal.zone) else np.asarray(zonal.zone)).tolist()
        names = tuple(extra)
        extra = [v.tolist() if hasattr(v, "tolist") else list(v) for v in extra.values()]
        if any(len(v) != len(zone) for v in extra):
            raise ValueError("polygons_geojson: every attribute has one value per row of the Zonal")
        boxes, cxs, cys = (a.tolist() for a in zonal_geometry(zonal, pixel_scale, origin))
        row_of = {z: r for r, z in enumerate(zone)}
    label, ring_id, start, area2, verts = (t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t) for t in rings)
    flat = (classes.cpu().numpy() if torch.is_tensor(classes) else np.asarray(classes)).ravel()
    sx, sy = (1.0, 1.0) if pixel_scale is None else (float(pixel_scale[0]), float(pixel_scale[1]))
    ox, oy = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    xy = np.empty((verts.shape[0], 2), np.float64)
    xy[:, 0] = ox + verts[:, 0].astype(np.float64) * sx
    xy[:, 1] = oy - verts[:, 1].astype(np.float64) * sy
    xy, first = xy.tolist(), start.tolist()                             # one conversion each: the loop below slices lists
    order = np.argsort(label, kind="stable")                            # rings are in ascending ring id: the exterior (4 * label) leads
    by_label, twice, owner = order.tolist(), area2[order].tolist(), label[order].tolist()
    features, i, n = [], 0, len(by_label)
    collecting = gc.isenabled()                                         # millions of small lists and no cycle among them: the cycle
    gc.disable()                                                        # collector would walk them again and again, 3 x the time
    try:
        while i < n:
            l, coords, total = owner[i], [], 0
            while i < n and owner[i] == l:
                ring = xy[first[by_label[i]]:first[by_label[i] + 1]]
                coords.append(ring[:1] + ring[:0:-1] + ring[:1])            # from the first vertex, against the walk
                total += twice[i]
                i += 1
            pixels = total // 2
            features.append({"type": "Feature",
                             "properties": {"class": int(flat[l]), "pixels": pixels, "area": None if pixel_scale is None else pixels * sx * sy},
                             "geometry": {"type": "Polygon", "coordinates": coords}})
            if extra is not None:
                r, props = row_of.get(l), features[-1]["properties"]
                props["centroid_x"], props["centroid_y"] = (None, None) if r is None else (cxs[r], cys[r])
                for name, column in zip(names, extra):
                    props[name] = None if r is None else column[r]
                if r is not None:
                    features[-1]["bbox"] = boxes[r]
    finally:
        if collecting:
            gc.enable()
    return {"type": "FeatureCollection", "features": features}


# ---------------------------------------------------------------------------------------------------- zonal statistics
def _check_zonal_values(values, like, frac_bits, name):
    """values and frac_bits against the map `like`, without a device -> values as [B, Hs, Ws] (or None)"""
    if isinstance(frac_bits, bool) or not isinstance(frac_bits, (int, np.integer)) or not 0 <= int(frac_bits) <= 30:
        raise ValueError(f"{name}: frac_bits is an int in 0 .. 30, got {frac_bits!r}")
    if values is None:
        return None
    if not torch.is_tensor(values) or values.dtype != torch.float32 or values.dim() not in (2, 3) or not values.is_contiguous() \
            or values.shape[-2:] != like.shape or values.device != like.device:
        raise ValueError(f"{name}: values is a contiguous float32 tensor [B, Hs, Ws] or [Hs, Ws] on the map's device")
    if values.dim() == 2:
        values = values.unsqueeze(0)
    if values.shape[0] > MAX_ZONAL_BANDS:
        raise ValueError(f"{name}: at most {MAX_ZONAL_BANDS} bands, got {values.shape[0]}")
    return values


def _check_zonal(zones, values, where, frac_bits, name):
    """the checks that need no device -> values as [B, Hs, Ws] (or None); the caller ends with require_gpu"""
    if not torch.is_tensor(zones) or zones.dtype != torch.int32 or zones.dim() != 2 or not zones.is_contiguous():
        raise ValueError(f"{name}: zones is a contiguous int32 device tensor [Hs, Ws]")
    if zones.numel() > 2 ** 31 - 1:
        raise ValueError(f"{name}: at most 2^31 - 1 pixels, got {zones.numel()}")
    values = _check_zonal_values(values, zones, frac_bits, name)
    if where is not None and (not torch.is_tensor(where) or where.dtype != torch.uint8 or where.shape != zones.shape or not where.is_contiguous()
                              or where.device != zones.device):
        raise ValueError(f"{name}: where is a contiguous uint8 tensor [Hs, Ws] on the zones' device")
    return values


def _zonal_rows(zones, where):
    """the presence flags of the zones, their exclusive scan (the row of every present zone) and N, the one value read on the host ->
    (present int32 [HW], row int32 [HW], N); (None, None, 0) for an empty scene"""
    HW = zones.numel()
    if not HW:
        return None, None, 0
    present = torch.empty(HW, dtype=torch.int32, device=zones.device)
    _lib.check(_lib.load().ksmi_scene_zonal_mark(zones.data_ptr(), None if where is None else where.data_ptr(), HW, present.data_ptr(),
                                                 stream_ptr()), "scene_zonal_mark")
    row = torch.empty(HW, dtype=torch.int32, device=zones.device)
    return present, row, int(_scan(present, row, "scan_i32").item())    # the one host read


def zonal_stats(zones, values=None, where=None, frac_bits=16):
    """Statistics of value rasters per zone of a zone raster -> Zonal, device tensors.

    zones int32 [Hs, Ws]: the zone of pixel p = y * Ws + x is zones[p]; a value outside 0 .. Hs * Ws - 1 is no zone and the pixel is
    skipped (the rule of component_sizes), so the labels of label_components are zones as they are.  values: float32 [B, Hs, Ws] or
    [Hs, Ws], 0 <= B <= 8, or None (geometry only).  where: uint8 [Hs, Ws] or None; a pixel where it is zero is skipped.  One row per
    zone with at least one pixel that is not skipped, in ascending zone id (N rows):
      zone         int32 [N]     the zone id
      count        int32 [N]     its pixels that are not skipped
      bbox         int32 [N, 4]  (x0, y0, x1, y1), inclusive pixel indices
      sum_x, sum_y int64 [N]     the sums of the pixel indices x and y: the mean pixel centre is (sum_x + count / 2) / count
      valid        int32 [B, N]  its pixels whose value in band b is finite
      vmin, vmax   float32 [B, N] the extremes over the finite values, in the order of the key bits ^ (bits >> 31 ? 0xFFFFFFFF :
                                 0x80000000) compared unsigned (-0.0 < +0.0); +inf and -inf where valid == 0
      vsum         int64 [B, N]  the sum over the finite values of q(v) = rint(clamp(v, -2^(32 - frac_bits), 2^(32 - frac_bits)) *
                                 2^frac_bits), rint to even: |q| <= 2^32, so the sum cannot overflow; the mean is vsum / 2^frac_bits /
                                 valid in float64 on the host
    and frac_bits itself.  Everything accumulated is an integer, or a minimum / maximum under a total order: the bits are those of
    tests/zonal_ref.py on every run.  Launches: the presence flags, their scan, the zone ids and the neutral tables, the accumulate
    pass (between two small passes that turn the extremes into keys and back).  One integer, N, is read on the host to size the
    tables.  Scratch: 8 B per pixel (the flags and their scan) and the scan's own 4 B per 2048 pixels; the tables are O(N).  The
    inputs are left unchanged.  No zone present, or an empty scene: empty tensors; B == 0: the band tables are [0, N]."""
    values = _check_zonal(zones, values, where, frac_bits, "zonal_stats")
    require_gpu(zones)
    dev, HW = zones.device, zones.numel()
    Hs, Ws = zones.shape
    B = 0 if values is None else values.shape[0]
    lib, st = _lib.load(), stream_ptr()
    present, row, N = _zonal_rows(zones, where)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = Zonal(i32(N), i32(N), i32(N, 4), i64(N), i64(N), i32(B, N), f32(B, N), f32(B, N), i64(B, N), int(frac_bits))
    if N:
        band = [t.data_ptr() if B else None for t in (out.valid, out.vmin, out.vmax, out.vsum)]
        _lib.check(lib.ksmi_scene_zonal_tables(present.data_ptr(), row.data_ptr(), HW, N, B, out.zone.data_ptr(), out.count.data_ptr(),
                                               out.bbox.data_ptr(), out.sum_x.data_ptr(), out.sum_y.data_ptr(), *band, st), "scene_zonal_tables")
        _lib.check(lib.ksmi_scene_zonal_accumulate(zones.data_ptr(), None if where is None else where.data_ptr(),
                                                   values.data_ptr() if B else None, B, Hs, Ws, int(frac_bits), row.data_ptr(), N,
                                                   out.count.data_ptr(), out.bbox.data_ptr(), out.sum_x.data_ptr(), out.sum_y.data_ptr(), *band, st),
                   "scene_zonal_accumulate")
    return out


def component_stats(classes, select=(1, 2), values=None, labels=None, frac_bits=16):
    """zonal_stats over the 4-connected components of the classes in `select` -> Zonal: zones = labels (label_components(classes, 4)
    unless given), where = select_classes(classes, select).  Its rows are the components `polygonize(classes, select)` emits, in the
    same order (ascending label; an exterior ring has ring_id == 4 * zone), and count is the feature's "pixels"."""
    _select_mask(select, "component_stats")
    if not torch.is_tensor(classes) or classes.dtype != torch.uint8 or classes.dim() != 2 or not classes.is_contiguous():
        raise ValueError("component_stats: classes is a contiguous uint8 device tensor [Hs, Ws]")
    if labels is not None and (not torch.is_tensor(labels) or labels.shape != classes.shape or labels.device != classes.device):
        raise ValueError("component_stats: labels has the shape and the device of classes")
    _check_zonal_values(values, classes, frac_bits, "component_stats")
    require_gpu(classes)
    if labels is None:
        labels = label_components(classes, 4)
    return zonal_stats(labels, values, select_classes(classes, select), frac_bits)


# ---------------------------------------------------------------------------------------------------- percentiles per zone
def basis_points(percentiles, name="zonal_quantiles"):
    """percents (one number or a sequence: 50, 97.5, 99.99) -> the tuple of basis points c = round(100 * p), in the order given.  A p
    that is no finite real number, that is further than 1e-9 from c / 100, or whose c is outside 0 .. 10000 is refused, and so are an
    empty sequence and more than MAX_PERCENTILES."""
    if isinstance(percentiles, (int, float, np.integer, np.floating)):
        percentiles = (percentiles,)
    try:
        given = tuple(percentiles)
    except TypeError:
        raise ValueError(f"{name}: percentiles is a sequence of percents, got {percentiles!r}") from None
    if not 1 <= len(given) <= MAX_PERCENTILES:
        raise ValueError(f"{name}: 1 .. {MAX_PERCENTILES} percentiles, got {len(given)}")
    out = []
    for p in given:
        if isinstance(p, (bool, np.bool_)) or not isinstance(p, (int, float, np.integer, np.floating)) or not math.isfinite(p):
            raise ValueError(f"{name}: a percentile is a percent 0 .. 100, got {p!r}")
        c = int(round(100 * float(p)))
        if abs(float(p) - c / 100) > 1e-9:
            raise ValueError(f"{name}: a percentile is a whole number of basis points (hundredths of a percent), got {p!r}")
        if not 0 <= c <= 10000:
            raise ValueError(f"{name}: a percentile is a percent 0 .. 100, got {p!r}")
        out.append(c)
    return tuple(out)


def percentile_name(c):
    """the name of the basis point c: "p" and the percent with trailing zeros stripped and "." written as "_": p50, p97_5, p0_01"""
    c = int(c)
    if not 0 <= c <= 10000:
        raise ValueError(f"percentile_name: a basis point 0 .. 10000, got {c}")
    whole, part = divmod(c, 100)
    return f"p{whole}" + (("_" + f"{part:02d}".rstrip("0")) if part else "")


def quantile_values(zq, method="linear"):
    """The percentiles of a ZonalQuantiles as float64 [B, P, N], combined on the host from its `lower` and `higher` in float64.  With
    g = c * (valid - 1) % 10000 (the position's fraction in basis points): "linear" lower + (higher - lower) * (g / 10000); "lower";
    "higher"; "midpoint" (lower + higher) / 2; "nearest" lower if 2 * g <= 10000 else higher.  NaN where valid == 0."""
    if method not in QUANTILE_METHODS:
        raise ValueError(f"quantile_values: method is one of {', '.join(QUANTILE_METHODS)}, got {method!r}")
    host = lambda t: t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    lower, higher, valid = host(zq.lower).astype(np.float64), host(zq.higher).astype(np.float64), host(zq.valid).astype(np.int64)
    c = np.asarray(zq.percentiles, np.int64).reshape(1, -1, 1)
    g = c * np.maximum(valid[:, None, :] - 1, 0) % 10000
    if method == "lower":
        return lower
    if method == "higher":
        return higher
    if method == "midpoint":
        return (lower + higher) / 2.0
    if method == "nearest":
        return np.where(2 * g <= 10000, lower, higher)
    return lower + (higher - lower) * (g / 10000.0)


def _sorted_composites(zones, band_ptr, where, row, N):
    """the composites of one band (a device address of HW float32), sorted -> int64 [HW] holding them as unsigned 64-bit integers"""
    HW, dev = zones.numel(), zones.device
    lib, st = _lib.load(), stream_ptr()
    keys, alt = torch.empty(HW, dtype=torch.int64, device=dev), torch.empty(HW, dtype=torch.int64, device=dev)
    need = int(lib.ksmi_scene_quantile_scratch(HW))
    scratch = torch.empty(need, dtype=torch.int32, device=dev)
    _lib.check(lib.ksmi_scene_quantile_keys(zones.data_ptr(), None if where is None else where.data_ptr(), band_ptr, row.data_ptr(), HW, N,
                                            keys.data_ptr(), st), "scene_quantile_keys")
    _lib.check(lib.ksmi_scene_quantile_sort(keys.data_ptr(), alt.data_ptr(), HW, N, scratch.data_ptr(), need, st), "scene_quantile_sort")
    return keys if int(lib.ksmi_scene_quantile_passes(N)) % 2 == 0 else alt          # an odd number of passes ends in the other buffer


def zonal_quantiles(zones, values, percentiles=(50,), where=None):
    """Percentiles of value rasters per zone of a zone raster -> ZonalQuantiles(zone, valid, lower, higher, percentiles).

    zones, where, the skip rule and the rows are those of zonal_stats.  values: float32 [B, Hs, Ws] or [Hs, Ws], 1 <= B <= 8.
    percentiles: 1 .. 16 percents such as 50, 97.5 or 99.99, whole numbers of basis points (basis_points).  For band b and row r, s is
    the ascending sequence of the finite values of the row's pixels, ordered by the key bits ^ (bits >> 31 ? 0xFFFFFFFF : 0x80000000)
    compared unsigned (-0.0 < +0.0), and n its length:
      zone        int32 [N]         the zone id
      valid       int32 [B, N]      n: zonal_stats(...).valid
      lower       float32 [B, P, N] s[k]            with pos = c * (n - 1) in integers, k = pos // 10000, g = pos % 10000: what
      higher      float32 [B, P, N] s[k + (g > 0)]  np.percentile(method="lower") and "higher" give, the position taken exactly;
                                                    NaN where n == 0.  Bit copies of input values.
      percentiles tuple [P]         the basis points c, in the order given
    quantile_values combines lower and higher on the host ("linear" by default).  Equal keys are equal bits, so the sorted sequence is
    unique: the bits are those of tests/quantile_ref.py on every run.  Launches: the presence flags and their scan (as zonal_stats),
    the zone ids, and per band the composites (row << 32 | key; all ones where a pixel takes no part), a stable radix sort of 8-bit
    digits over all Hs * Ws composites (4 value passes and one per started byte of N - 1: 4 .. 8 passes of three launches) and the
    selection (two binary searches per row, shared by its percentiles).  One integer, N, is read on the host, as in zonal_stats, and nothing
    else.  Scratch: 8 B per pixel (the flags and their scan), 16 B per pixel (two buffers of composites) and 1 KiB of counters per
    4096 pixels: 24.25 B per pixel, 487 MB for a scene of 4480 x 4480.  Bands go one at a time, so scratch does not grow with B.  The
    inputs are left unchanged.  No zone present, or an empty scene: empty tensors."""
    name = "zonal_quantiles"
    values = _check_zonal(zones, values, where, 16, name)
    if values is None or values.shape[0] < 1:
        raise ValueError(f"{name}: values is a contiguous float32 tensor [B, Hs, Ws] or [Hs, Ws] on the map's device, 1 <= B <= {MAX_ZONAL_BANDS}")
    pcts = basis_points(percentiles, name)
    require_gpu(zones)
    dev, HW, B, P = zones.device, zones.numel(), values.shape[0], len(pcts)
    lib, st = _lib.load(), stream_ptr()
    present, row, N = _zonal_rows(zones, where)
    out = ZonalQuantiles(torch.empty(N, dtype=torch.int32, device=dev), torch.empty((B, N), dtype=torch.int32, device=dev),
                         torch.empty((B, P, N), dtype=torch.float32, device=dev), torch.empty((B, P, N), dtype=torch.float32, device=dev), pcts)
    if N:
        _lib.check(lib.ksmi_scene_quantile_zones(present.data_ptr(), row.data_ptr(), HW, N, out.zone.data_ptr(), st), "scene_quantile_zones")
        del present
        host_pcts = (_lib.C.c_int32 * P)(*pcts)
        for b in range(B):
            ordered = _sorted_composites(zones, values[b].data_ptr(), where, row, N)
            _lib.check(lib.ksmi_scene_quantile_select(ordered.data_ptr(), HW, N, host_pcts, P, out.valid[b].data_ptr(), out.lower[b].data_ptr(),
                                                      out.higher[b].data_ptr(), st), "scene_quantile_select")
            del ordered
    return out


def zonal_sorted(zones, values2d, where=None):
    """The sorted values of one band per zone -> (zone int32 [N], offsets int32 [N + 1], sorted float32 [Hs * Ws]), device tensors: the
    primitive under zonal_quantiles.  values2d: float32 [Hs, Ws].  sorted[offsets[r]:offsets[r + 1]] holds the finite values of the
    pixels of row r in ascending key order (zonal_quantiles), offsets[0] == 0 and offsets[N] is the number of pixels that take part;
    what lies past offsets[N] is unspecified.  The launches, the one host read (N) and the scratch are those of zonal_quantiles for
    one band.  No zone present, or an empty scene: zone is empty, offsets == [0] and sorted has Hs * Ws unspecified elements."""
    name = "zonal_sorted"
    if torch.is_tensor(values2d) and values2d.dim() != 2:
        raise ValueError(f"{name}: values2d is a contiguous float32 tensor [Hs, Ws] on the map's device")
    values = _check_zonal(zones, values2d, where, 16, name)
    if values is None:
        raise ValueError(f"{name}: values2d is a contiguous float32 tensor [Hs, Ws] on the map's device")
    require_gpu(zones)
    dev, HW = zones.device, zones.numel()
    lib, st = _lib.load(), stream_ptr()
    present, row, N = _zonal_rows(zones, where)
    zone = torch.empty(N, dtype=torch.int32, device=dev)
    offsets = torch.zeros(N + 1, dtype=torch.int32, device=dev)
    ordered = torch.empty(HW, dtype=torch.float32, device=dev)
    if N:
        _lib.check(lib.ksmi_scene_quantile_zones(present.data_ptr(), row.data_ptr(), HW, N, zone.data_ptr(), st), "scene_quantile_zones")
        del present
        composites = _sorted_composites(zones, values.data_ptr(), where, row, N)
        _lib.check(lib.ksmi_scene_quantile_segments(composites.data_ptr(), HW, N, offsets.data_ptr(), ordered.data_ptr(), st),
                   "scene_quantile_segments")
    return zone, offsets, ordered


def component_quantiles(classes, values, percentiles=(50,), select=(1, 2), labels=None):
    """zonal_quantiles over the 4-connected components of the classes in `select` -> ZonalQuantiles: zones = labels
    (label_components(classes, 4) unless given), where = select_classes(classes, select), as component_stats keys zonal_stats.  Its
    rows are those of component_stats(classes, select) and the features of polygonize(classes, select), in the same order."""
    name = "component_quantiles"
    _select_mask(select, name)
    if not torch.is_tensor(classes) or classes.dtype != torch.uint8 or classes.dim() != 2 or not classes.is_contiguous():
        raise ValueError(f"{name}: classes is a contiguous uint8 device tensor [Hs, Ws]")
    if labels is not None and (not torch.is_tensor(labels) or labels.shape != classes.shape or labels.device != classes.device):
        raise ValueError(f"{name}: labels has the shape and the device of classes")
    checked = _check_zonal_values(values, classes, 16, name)
    if checked is None or checked.shape[0] < 1:
        raise ValueError(f"{name}: values is a contiguous float32 tensor [B, Hs, Ws] or [Hs, Ws] on the map's device, 1 <= B <= {MAX_ZONAL_BANDS}")
    basis_points(percentiles, name)
    require_gpu(classes)
    if labels is None:
        labels = label_components(classes, 4)
    return zonal_quantiles(labels, values, percentiles, select_classes(classes, select))


# ---------------------------------------------------------------------------------------------------- zones from a vector layer
def rasterize_zones(edges, feature, Hs, Ws, count=None):
    """The zone raster of a vector layer -> int32 [Hs, Ws] on the device of `edges`: zones[y][x] = the smallest feature whose polygons
    cover the centre of pixel (x, y), -1 where none does; what zonal_stats and zonal_quantiles take as `zones`.

    edges int32 [E, 4] = (x0, y0, x1, y1) and feature int32 [E], device tensors (ZoneEdges of zone_edges, uploaded): the edges of
    feature f form closed rings; vertices are in units of 1/256 pixel, x right and y down, the centre of pixel (x, y) at (256 x + 128,
    256 y + 128), every |coordinate| <= MAX_ZONE_COORD.  Hs, Ws <= 32767.  count: the number of features F (every feature[e] is in
    0 .. F - 1); None reads max(feature) + 1 on the host, a second read.  The rule, in integers throughout: a horizontal edge crosses
    no scanline; any other, oriented so that y0 < y1, crosses the scanlines y with y0 <= 256 y + 128 < y1 (half open), kept to 0 <= y <
    Hs, at the column c = clamp(ceil((x0 * dy + (256 y + 128 - y0) * dx - 128 * dy) / (256 * dy)), 0, Ws): the first column whose
    centre is at or right of the crossing.  Sorted by (f, y, c), crossings 2k and 2k + 1 bound a span [c0, c1) of row y of feature f:
    the even-odd rule per feature, so ring orientation does not matter, holes and multipolygon parts need nothing special, a pixel
    centre exactly on an edge belongs to exactly one side, and features that share an edge partition the pixels along it.  The bits
    are those of tests/zones_ref.py on every run.  Launches: the scanlines per edge, their scan, one composite f << 32 | y << 16 | c
    per crossing (its edge found by binary search in the scan), the radix sort of zonal_quantiles with F rows (4 value passes and one
    per started byte of F - 1), and the fill: the raster set to -1, then one wave64 per span lowering its pixels to f with an integer
    atomic minimum.  One pair of integers is read on the host: X, the number of crossings, and the number of edges refused (a
    coordinate beyond the bound, a feature outside 0 .. F - 1: ValueError, as are an odd X -- rings that are not closed -- and X >
    2^31 - 1).  Scratch: 4 B per edge, 16 B per crossing (two buffers of composites, max(X, F) long) and 1 KiB of counters per 4096
    crossings.  The inputs are left unchanged.  No edge, no crossing: all -1."""
    name = "rasterize_zones"
    if not torch.is_tensor(edges) or edges.dtype != torch.int32 or edges.dim() != 2 or edges.shape[1] != 4 or not edges.is_contiguous():
        raise ValueError(f"{name}: edges is a contiguous int32 device tensor [E, 4]")
    if not torch.is_tensor(feature) or feature.dtype != torch.int32 or feature.dim() != 1 or not feature.is_contiguous() \
            or feature.shape[0] != edges.shape[0] or feature.device != edges.device:
        raise ValueError(f"{name}: feature is a contiguous int32 vector [E] on the edges' device")
    for v, what in ((Hs, "Hs"), (Ws, "Ws")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_ZONE_SIDE:
            raise ValueError(f"{name}: {what} is an int in 0 .. {MAX_ZONE_SIDE}, got {v!r}")
    if count is not None and (isinstance(count, bool) or not isinstance(count, (int, np.integer)) or not 0 <= int(count) <= 2 ** 31 - 1):
        raise ValueError(f"{name}: count is the number of features, an int in 0 .. 2^31 - 1, got {count!r}")
    E = edges.shape[0]
    if E > 2 ** 31 - 1:
        raise ValueError(f"{name}: at most 2^31 - 1 edges")
    require_gpu(edges)
    Hs, Ws, dev = int(Hs), int(Ws), edges.device
    lib, st = _lib.load(), stream_ptr()
    F = int(count) if count is not None else (int(feature.max().item()) + 1 if E else 0)
    zones = torch.empty((Hs, Ws), dtype=torch.int32, device=dev)
    counts = torch.empty(E, dtype=torch.int32, device=dev)
    info = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.check(lib.ksmi_scene_zone_rows(edges.data_ptr(), feature.data_ptr(), E, max(F, 0), Hs, Ws, counts.data_ptr(), info.data_ptr(), st),
               "scene_zone_rows")
    X, refused = info.tolist()                                          # the one host read
    if refused:
        raise ValueError(f"{name}: {refused} edges with a coordinate beyond +-{MAX_ZONE_COORD} or a feature outside 0 .. {F - 1}")
    if X > 2 ** 31 - 1:
        raise ValueError(f"{name}: {X} crossings, more than 2^31 - 1")
    if X % 2:
        raise ValueError(f"{name}: an odd number of crossings ({X}): the edges of a feature do not form closed rings")
    ordered = None
    if X and Hs * Ws:
        _scan(counts, counts, "scan_i32")
        n_keys = max(X, F)                                              # the sort takes no more rows than composites: all ones pad them
        keys, alt = torch.empty(n_keys, dtype=torch.int64, device=dev), torch.empty(n_keys, dtype=torch.int64, device=dev)
        need = int(lib.ksmi_scene_quantile_scratch(n_keys))
        scratch = torch.empty(need, dtype=torch.int32, device=dev)
        _lib.check(lib.ksmi_scene_zone_crossings(edges.data_ptr(), feature.data_ptr(), counts.data_ptr(), E, X, Hs, Ws, keys.data_ptr(), n_keys,
                                                 st), "scene_zone_crossings")
        _lib.check(lib.ksmi_scene_quantile_sort(keys.data_ptr(), alt.data_ptr(), n_keys, F, scratch.data_ptr(), need, st), "scene_quantile_sort")
        ordered = keys if int(lib.ksmi_scene_quantile_passes(F)) % 2 == 0 else alt
    _lib.check(lib.ksmi_scene_zone_fill(None if ordered is None else ordered.data_ptr(), X if ordered is not None else 0, F, Hs, Ws,
                                        zones.data_ptr(), st), "scene_zone_fill")
    return zones


def _clip_ring(p, x_lo, x_hi, y_lo, y_hi):
    """Sutherland-Hodgman: the ring p float64 [n, 2] against the box, in the order left, right, top, bottom.  An intersection is
    computed from the edge's lexicographically smaller end, so an edge shared by two rings is cut at the same point in both."""
    for axis, bound, keep_above in ((0, x_lo, True), (0, x_hi, False), (1, y_lo, True), (1, y_hi, False)):
        if p.shape[0] == 0:
            break
        a, b = p, np.roll(p, -1, axis=0)
        ina = a[:, axis] >= bound if keep_above else a[:, axis] <= bound
        inb = np.roll(ina, -1)
        swap = (a[:, 0] > b[:, 0]) | ((a[:, 0] == b[:, 0]) & (a[:, 1] > b[:, 1]))
        lo, hi = np.where(swap[:, None], b, a), np.where(swap[:, None], a, b)
        cut = ina != inb                                                # there lo and hi differ along the axis
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (bound - lo[:, axis]) / (hi[:, axis] - lo[:, axis])
            hit = lo + t[:, None] * (hi - lo)                           # used only where cut
        hit[:, axis] = bound
        both = np.empty((p.shape[0], 2, 2), np.float64)                 # per edge: its start if inside, then its cut
        both[:, 0], both[:, 1] = a, hit
        p = both[np.stack((ina, cut), axis=1)]
    return p


def zone_edges(features, Hs, Ws, pixel_scale=None, origin=None):
    """The edge table of a vector layer for rasterize_zones, on the host -> ZoneEdges(edges int32 [E, 4], feature int32 [E], count),
    numpy arrays; count = len(features).

    features: a list with one list of rings per feature (exterior rings, holes and multipolygon parts alike: the even-odd rule needs
    no distinction); a ring is a sequence of (X, Y) or (X, Y, Z) map coordinates, closed or not.  In float64 px = (X - ox) / sx and py
    = (oy - Y) / sy with pixel_scale = (sx, sy) and origin = (ox, oy) as geotiff.read returns them: the inverse of what
    polygons_geojson writes (scale (1, 1) and origin (0, 0) without georeferencing).  A closing vertex equal to the first is dropped.
    A ring that leaves the box [-Ws, 2 Ws] x [-Hs, 2 Hs] is clipped against it (Sutherland-Hodgman: left, right, top, bottom); a ring
    inside the box is untouched.  Then q = rint(256 p), half to even, in units of 1/256 pixel, so every vertex is within the
    coordinate bound of rasterize_zones.  A ring of fewer than 3 vertices gives no edge.  A clipped ring is accurate to 1/256 pixel,
    like any vertex: where an edge is cut, its new end is rounded as every vertex is, and the edge may move by that much."""
    for v, what in ((Hs, "Hs"), (Ws, "Ws")):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= MAX_ZONE_SIDE:
            raise ValueError(f"zone_edges: {what} is an int in 0 .. {MAX_ZONE_SIDE}, got {v!r}")
    sx, sy = (1.0, 1.0) if pixel_scale is None else (float(pixel_scale[0]), float(pixel_scale[1]))
    ox, oy = (0.0, 0.0) if origin is None else (float(origin[0]), float(origin[1]))
    Hs, Ws = int(Hs), int(Ws)
    tables, owners = [], []
    for f, rings in enumerate(features):
        for ring in rings:
            a = np.asarray(ring, np.float64)
            if a.size == 0:
                continue
            if a.ndim != 2 or a.shape[1] < 2:
                raise ValueError(f"zone_edges: a ring of feature {f} is no sequence of (X, Y) positions")
            p = np.stack(((a[:, 0] - ox) / sx, (oy - a[:, 1]) / sy), axis=1)
            if not np.isfinite(p).all():
                raise ValueError(f"zone_edges: a ring of feature {f} has a coordinate that is not finite")
            if p.shape[0] > 1 and (p[0] == p[-1]).all():
                p = p[:-1]
            if (p[:, 0] < -Ws).any() or (p[:, 0] > 2 * Ws).any() or (p[:, 1] < -Hs).any() or (p[:, 1] > 2 * Hs).any():
                p = _clip_ring(p, -float(Ws), 2.0 * Ws, -float(Hs), 2.0 * Hs)
            q = np.rint(256.0 * p).astype(np.int64)
            if q.shape[0] < 3:
                continue
            tables.append(np.concatenate((q, np.roll(q, -1, axis=0)), axis=1))
            owners.append(np.full(q.shape[0], f, np.int64))
    edges = np.concatenate(tables, axis=0) if tables else np.empty((0, 4), np.int64)
    owner = np.concatenate(owners) if owners else np.empty(0, np.int64)
    return ZoneEdges(np.ascontiguousarray(edges.astype(np.int32)), np.ascontiguousarray(owner.astype(np.int32)), len(features))


def zones_from_geojson(obj, Hs, Ws, pixel_scale=None, origin=None, key=None):
    """A GeoJSON object (a dict: a FeatureCollection, a Feature or a bare geometry) -> (ZoneEdges, ids) through zone_edges.

    Feature f of the file is row f: a Polygon gives its rings, a MultiPolygon the rings of all its parts, any other geometry and a
    null geometry keep their index with no ring (and so no pixel).  Z values are ignored.  A "crs" member is ignored with a printed
    note: coordinates are taken in the raster's own coordinate reference system, as polygons_geojson writes them.  ids[f] =
    properties[key], or f when key is None."""
    name = "zones_from_geojson"
    if not isinstance(obj, dict) or "type" not in obj:
        raise ValueError(f"{name}: a GeoJSON object (a dict with a \"type\")")
    if "crs" in obj:
        print(f"{name}: the \"crs\" member is ignored: coordinates are taken in the raster's own coordinate reference system")
    if obj["type"] == "FeatureCollection":
        members = list(obj.get("features") or [])
    elif obj["type"] == "Feature":
        members = [obj]
    else:
        members = [{"type": "Feature", "properties": {}, "geometry": obj}]
    features, ids = [], []
    for f, member in enumerate(members):
        geometry = member.get("geometry") if isinstance(member, dict) else None
        kind = geometry.get("type") if isinstance(geometry, dict) else None
        if kind == "Polygon":
            rings = list(geometry.get("coordinates") or [])
        elif kind == "MultiPolygon":
            rings = [ring for part in geometry.get("coordinates") or [] for ring in part]
        else:
            rings = []
        features.append(rings)
        if key is None:
            ids.append(f)
        else:
            properties = member.get("properties") if isinstance(member, dict) else None
            if not isinstance(properties, dict) or key not in properties:
                raise ValueError(f"{name}: feature {f} has no property {key!r}")
            ids.append(properties[key])
    return zone_edges(features, Hs, Ws, pixel_scale, origin), ids


# ---------------------------------------------------------------------------------------------------- the scene loop
def predict_scene(forward, rasters, norms, window=224, stride=112, batch=32, weight="hann", nodata=None, score=None, raw=False,
                  invalid_class=3, mmu=None, connectivity=4, tta=None):
    """A class map of a whole scene.

    rasters: device float32 [C_i, Hs, Ws], one per model input (e.g. pre, post, DEM), all of one size.
    norms:   per raster (mean, std, clamp), each one value per channel: clamp >= 0 clamps to [0, clamp] and maps NaN to clamp,
             clamp < 0 leaves the value and maps NaN to the mean (the DEM); then (v - mean) / std.
    forward: callable on the list of [B, C_i, h, w] window batches -> logits [B, K, h, w] (cd_forward / seg_forward, or any stub).
    window, stride: of the square windows, 1 <= stride <= window; weight: "hann" or "uniform" (blend_weights).
    nodata:  the sentinel of the rasters (None: only NaN is missing); one value, or one per raster.
    raw:     gather raw values (nodata -> NaN) for a model that normalises inside its first convolution (cd_forward(..., norms)).
    score:   None, "logits" (the blended mean logits) or "softmax".
    mmu:     None, or the minimum mapping unit in pixels: the class map goes through one pass of `sieve` at `connectivity` (4 or 8)
             over the model's K classes.  The scores are returned unchanged: they describe the blend, not the sieved map.
    tta:     None or "none": one pass.  A name of VIEW_SETS ("hflip": identity and x flip; "flips": the four flips; "d4": those and
             their transposes) or a tuple of distinct view codes 0 .. 7 (taken in ascending order): every window goes through the model
             once per view (scene_gather_view), the logits are turned back (scene_unview) and all views enter the blend with the
             window's weight (scene_accumulate_views), so the map is the weighted mean over windows and views, in logit space, and its
             bits still do not depend on `batch`.  V views cost V times the model time and a [V, batch, K, h, w] float32 buffer.
             (0,) takes this path and gives the bits of None.
    Returns (classes uint8 [Hs, Ws] with `invalid_class` where some input is missing, scores float32 [K, Hs, Ws] or None)."""
    if score not in SCORES:
        raise ValueError(f'predict_scene: score is None, "logits" or "softmax", got {score!r}')
    views = _views(tta)
    if mmu is not None and connectivity not in (4, 8):
        raise ValueError(f"predict_scene: connectivity is 4 or 8, got {connectivity!r}")
    if not rasters or len(norms) != len(rasters):
        raise ValueError("predict_scene: one (mean, std, clamp) per raster")
    for r in rasters:
        _check_raster(r, "predict_scene: every raster")
    dev = rasters[0].device
    Hs, Ws = rasters[0].shape[1:]
    if any(r.shape[1:] != (Hs, Ws) or r.device != dev for r in rasters):
        raise ValueError("predict_scene: the rasters have one size and one device")
    nodatas = list(nodata) if isinstance(nodata, (list, tuple)) else [nodata] * len(rasters)
    if len(nodatas) != len(rasters):
        raise ValueError("predict_scene: nodata is one value or one per raster")
    h = w = int(window)
    sy = sx = int(stride)
    if int(batch) < 1:
        raise ValueError("predict_scene: batch >= 1")
    ys_h, xs_h = window_grid(Hs, Ws, h, w, sy, sx)
    wt_h = blend_weights(h, w, weight)            # strictly positive on a grid that covers the scene: wsum > 0 at every pixel
    dev_norms = []
    for r, nm in zip(rasters, norms):
        vecs = [torch.as_tensor([float(v) for v in (p if hasattr(p, "__len__") else [p] * r.shape[0])], dtype=torch.float32) for p in nm]
        if len(vecs) != 3 or any(v.numel() != r.shape[0] for v in vecs) or bool((vecs[1] == 0).any()):
            raise ValueError("predict_scene: a norm is (mean, std, clamp) with one non-zero std per channel of its raster")
        dev_norms.append(None if raw else tuple(v.to(dev) for v in vecs))
    ys, xs, wt = torch.from_numpy(ys_h).to(dev), torch.from_numpy(xs_h).to(dev), torch.from_numpy(wt_h).to(dev)
    total = len(ys_h) * len(xs_h)
    acc = wsum = slabs = None

    def window_logits(i0, n, view):
        if view is None:
            tiles = [scene_gather(r, ys, xs, i0, n, h, w, nm, nd) for r, nm, nd in zip(rasters, dev_norms, nodatas)]
        else:
            tiles = [scene_gather_view(r, ys, xs, i0, n, h, w, view, nm, nd) for r, nm, nd in zip(rasters, dev_norms, nodatas)]
        logits = forward(tiles).float().contiguous()
        if logits.dim() != 4 or logits.shape[0] != n or logits.shape[2:] != (h, w) or not 1 <= logits.shape[1] <= MAX_CLASSES:
            raise ValueError(f"predict_scene: forward returned {tuple(logits.shape)}, expected [{n}, K <= {MAX_CLASSES}, {h}, {w}]")
        return logits

    with torch.no_grad():
        for i0 in range(0, total, int(batch)):
            n = min(int(batch), total - i0)                               # the ragged last batch passes its own n
            logits = window_logits(i0, n, None if views is None else views[0])
            if acc is None:
                K = logits.shape[1]
                acc = torch.zeros((K, Hs, Ws), dtype=torch.float32, device=dev)
                wsum = torch.zeros((Hs, Ws), dtype=torch.float32, device=dev)
                if views is not None:                                     # one buffer per scene; a ragged batch uses its head
                    slabs = torch.empty(len(views) * min(int(batch), total) * K * h * w, dtype=torch.float32, device=dev)
            if views is None:
                scene_accumulate(logits, ys, xs, i0, wt, acc, wsum)
                continue
            stack = slabs[:len(views) * n * K * h * w].view(len(views), n, K, h, w)
            for j, v in enumerate(views):
                if j:
                    logits = window_logits(i0, n, v)
                if logits.shape[1] != K:
                    raise ValueError(f"predict_scene: forward returned {logits.shape[1]} classes after {K}")
                scene_unview(logits, v, out=stack[j])
            scene_accumulate_views(stack, ys, xs, i0, wt, acc, wsum)
        valid = None
        for r, nd in zip(rasters, nodatas):
            valid = scene_valid(r, nd, valid)
        classes, scores = scene_finalize(acc, wsum, valid, score, invalid_class)
        if mmu is not None:
            classes, _ = sieve(classes, mmu, connectivity, invalid_class, acc.shape[0])
        return classes, scores


# ---------------------------------------------------------------------------------------------------- model adapters
def cd_forward(model, method, norms=None):
    """forward for predict_scene over rasters [date A, date B(, dem)]: model(xA, xB[, dem]); the last output for ChangeFormer, as
    eval_change_detection takes it.  norms (the list predict_scene gets; use with raw=True): the model normalises inside its first
    convolution, configured as training.change_detection_trainer.fuse_input_pipeline does (the date's channels, then the DEM's)."""
    if norms is not None:
        if not hasattr(model, "set_input_pipeline"):
            raise _lib.KsmiError(f"{type(model).__name__} has no fused input pipeline: predict with raw=False")
        as_lists = lambda nm: [[float(v) for v in p] for p in nm]
        if len(norms) < 2 or as_lists(norms[0]) != as_lists(norms[1]):
            raise ValueError("cd_forward: the two dates share one (mean, std, clamp)")
        per = [[float(v) for nm in (list(norms[:1]) + list(norms[2:])) for v in nm[j]] for j in range(3)]
        model.set_input_pipeline(*per)
    own_tail = hasattr(model, "set_input_pipeline")            # SNUNet_ECAM.forward(xA, xB, dem): the concat as an address choice

    def forward(xs):
        xa, xb = xs[0], xs[1]
        if len(xs) == 3 and own_tail:
            out = model(xa, xb, xs[2])
        elif len(xs) == 3:
            out = model(torch.cat((xa, xs[2]), dim=1), torch.cat((xb, xs[2]), dim=1))
        else:
            out = model(xa, xb)
        return out[-1] if str(method).lower() == "changeformer" else out
    return forward


def seg_forward(model, inputs=("pre_event_1", "pre_event_2", "post_event"), dem=False):
    """forward for predict_scene over rasters [post, (dem), then the pre-event dates in the order of synthetic.seg_inputs]: their
    channel concatenation, which is all seg_inputs does once the rasters are in that order"""
    want = 1 + (1 if dem else 0) + len(set(inputs) - {"post_event"})

    def forward(xs):
        if len(xs) != want:
            raise ValueError(f"seg_forward: {want} rasters for inputs {tuple(inputs)}" + (" with the DEM" if dem else "") + f", got {len(xs)}")
        return model(xs[0] if len(xs) == 1 else torch.cat(xs, dim=1))
    return forward
