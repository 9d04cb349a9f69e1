#!/usr/bin/env python3
"""Map a whole Sentinel-1 scene with a trained checkpoint: windowed inference with on-device blending (kurosiwo_amd/scene.py).

  python predict.py --task cd --method snunet --checkpoint best.pt \\
      --post VV.tif VH.tif --pre1 VV.tif VH.tif [--pre2 ...] [--dem dem.tif] \\
      --out flood.tif [--score softmax --score_out prob.tif] \\
      [--window 224 --stride 112 --weight hann --batch_size 32 --precision bf16] [--tta hflip] \\
      [--mmu 12 --connectivity 4 --sieve_passes 1] [--report flood.json] \\
      [--polygons flood.geojson --polygon_classes 1 2] [--components components.csv] \\
      [--depth_out depth.tif [--depth_dem dem.tif] [--depth_classes 1 2] [--percentiles 50 90]] \\
      [--zones districts.geojson [--zone_key NAME] [--zones_out zones.csv] [--zones_raster zones.tif] [--zone_classes 1 2]]

Each date takes one or more GeoTIFFs whose bands are concatenated in the order given; all rasters have one size.  The file's own
nodata tag is the sentinel of its date (--nodata overrides it); a pixel where any input is NaN or the sentinel becomes class 3
("Invalid pixels").  The DEM's gaps are filled on the host as the loaders fill them, and the DEM is standardised with the loaders'
constants.  The class raster is a Deflate-compressed uint8 GeoTIFF in tiles of 256 with the first post file's georeferencing and
nodata = 3; the scores, where asked for, a float32 multi-band file written the same way.  The scene, the accumulators and the outputs
live on one device: a scene that does not fit is outside this tool, as are --slope and SLC products.

--tta SET runs every window through the model once per view of SET and blends all views on the device, each with the window's weight
(kurosiwo_amd.scene.predict_scene(tta=SET): the mean over windows and views is taken in logit space, as the windows' already is;
probabilities are not averaged).  none (the default): one pass.  hflip: the window and its left-right mirror image, the orientation
the training augmentation (HorizontalFlip, configs/augmentations/augmentation.json) has shown the model.  flips: the four
combinations of the left-right and the up-down flip.  d4: those four and their transposes, all eight symmetries of the square.
flips and d4 show the model orientations it was not trained on: whether they help depends on the model.  V views cost V times the
model time and V * batch_size * classes * window^2 * 4 bytes more device memory; the map does not depend on --batch_size.

--mmu N applies a minimum mapping unit on the device before the map is written (kurosiwo_amd.scene.sieve): every connected component
(--connectivity 4: joined by edges, 8: by edges and corners) of fewer than N pixels takes the class most of its edge neighbours in
components of at least N pixels have; invalid pixels are never changed and never vote; --sieve_passes repeats the pass on its own
output.  The scores of --score_out describe the blend, not the sieved map.  --report FILE.json writes what the map holds, counted on
the class map as written: "pixel_counts" per class 0 .. 3, "pixel_area" (the product of the first post file's pixel scale, in map
units squared; null without georeferencing), "class_area" per class, "mmu", "connectivity", "passes" and "components_removed".

--polygons FILE.geojson writes the class map as written (after --mmu) as a vector layer, traced on the device
(kurosiwo_amd.scene.polygonize, polygons_geojson): one Polygon feature per edge-connected component of the classes of
--polygon_classes (default 1 2: the two water classes), whatever --connectivity the sieve ran with; the exterior ring first
(counter-clockwise), then its holes; vertices are pixel corners in the georeferencing of the first post file (pixel coordinates with
y negated without one), collinear vertices dropped; properties "class", "pixels" and "area".  No "crs" member is written: the
coordinates are in the raster's own coordinate reference system.

Every component also carries statistics reduced on the device, keyed by the component labels (kurosiwo_amd.scene.component_stats,
zonal_stats: integers and key-ordered extremes, the same bits on every run; no raster is read back for them).  --polygons with
--depth_out: a feature gains "depth_pixels" (its pixels with a finite depth), "depth_max", "depth_mean" (the fixed-point sum of the
depths at 16 fractional bits / 2^16 / depth_pixels, in float64; both null without such a pixel) and "volume" (that sum / 2^16 *
"pixel_area"; null without georeferencing).  --polygons with --score softmax: "confidence", the mean over the component of the softmax band of the component's own class (sums at 30 fractional bits; null where
the class has no band or no finite score); --score logits adds nothing.  A feature that gains any of these also gets a "bbox"
member [west, south, east, north] (the corners of its pixels' bounding box) and the properties "centroid_x", "centroid_y" (the mean
pixel centre, in map coordinates); --polygons alone writes what it always wrote.  --components FILE.csv writes the same statistics without the
polygons, one row per component of --polygon_classes in ascending label (the smallest linear index y * width + x of its pixels); it
needs neither --polygons nor the GeoJSON writer.  The header row is
  label,class,pixels,x0,y0,x1,y1,centroid_x,centroid_y
then ,depth_pixels,depth_max,depth_mean,volume with --depth_out and ,confidence with --score softmax: x0 .. y1 are the inclusive
pixel indices of the bounding box, floats are written so that they read back to the same float64, and a null is an empty field.
--report then gains a key "components": "count" (the components of --polygon_classes) and "largest" ({"label", "pixels"} of the one
with the most pixels, the smallest label on a tie; null without a component); only with --polygons or --components.

--depth_out FILE.tif writes the water depth of the class map as written (after --mmu), computed on the device
(kurosiwo_amd.scene.flood_depth) as FwDET does (Cohen et al. 2018): the DEM at the shore pixels -- water of --depth_classes (default
1 2) with a valid dry edge neighbour inside the scene; the scene border and invalid pixels make no shore -- is handed to every water
pixel from its nearest shore pixel by exact Euclidean distance, wherever in the scene that pixel lies, and the DEM is subtracted,
clamped at zero.  The DEM is --depth_dem, else the file of --dem; it has the scene's size and is read raw, in metres: its nodata tag
and NaN become NaN, no gap is filled and nothing is standardised (the model's copy of --dem is another matter).  The raster is a
float32 Deflate GeoTIFF in tiles of 256 with nodata NaN and the first post file's georeferencing: 0 on dry land, NaN at invalid
pixels, at water without a DEM value and where the scene has no shore at all.  --report then gains a key "depth": "water_pixels",
"with_depth" (those with a finite depth), "max" and "mean" over them, and "volume" (their sum in float64 times "pixel_area"; null
without georeferencing).  FwDET's smoothing filter, cost-distance allocation and a DEM on another grid are outside this tool.

--percentiles P [P ...] (percents, whole numbers of basis points, each once: 50 90 97.5) adds percentiles of the depth, which a few pixels that
took their level from another water body's shore hardly move, where they move the mean and the maximum a lot.  It needs --depth_out
and one of --components, --polygons, --report.  The depth raster still on the device is sorted per component on the device
(kurosiwo_amd.scene.component_quantiles, zonal_quantiles: a segmented radix sort and a selection; the same bits on every run) and
nothing is read back but the tables.  Every row of --components and every feature of --polygons gains one column or property per
percentile after "volume": "depth_p" and the percent with trailing zeros stripped and "." written as "_" (depth_p50, depth_p97_5),
the percentile over the component's pixels with a finite depth, interpolated linearly between the two neighbouring sorted values in
float64 as np.percentile does (the position c * (n - 1) / 10000 taken in exact integers); null for a component without such a
pixel.  The "depth" key of --report gains "percentiles": {"p50": ..., "p90": ...} over all pixels of --depth_classes with a finite
depth (one zone: the whole water surface); null values without such a pixel.  Percentiles of the confidence and weighted
percentiles are outside this tool.

--zones FILE.geojson describes the map as written (after --mmu) per feature of a vector layer -- districts, parcels, river reaches --
and needs one of --zones_out, --zones_raster, --report.  The file is a FeatureCollection, a Feature or a bare geometry; Polygon and
MultiPolygon features give zones, any other and a null geometry keep their index without a pixel, so zone f is always feature f of
the file.  Coordinates are taken in the raster's own coordinate reference system through the first post file's georeferencing
(pixel coordinates with y negated without one), the inverse of what --polygons writes; a "crs" member is ignored with a note.  The
polygons are rasterised on the device (kurosiwo_amd.scene.zones_from_geojson, rasterize_zones): a pixel belongs to the first feature
whose polygons cover its centre under the even-odd rule, decided in integers at 1/256 pixel, so features that share an edge
partition the pixels along it; the rasters are still on the device, and every number below comes from
kurosiwo_amd.scene.zonal_stats and zonal_quantiles keyed by that zone raster.  More features than scene pixels are refused.
--zones_out FILE.csv has one row per feature in file order; a feature without a pixel gets zeros and empty cells.  The header row is
  zone,id,pixels,valid,class_0,class_1,class_2,class_3,flooded,flooded_area,flooded_fraction
zone is the feature's index and id its property --zone_key (the index without one); pixels counts the zone's pixels in the scene and
valid those not of class 3; flooded counts the pixels of --zone_classes (default 1 2), flooded_area = flooded * "pixel_area" (empty
without georeferencing) and flooded_fraction = flooded / valid (empty when valid is 0).  With --depth_out follow
,depth_pixels,depth_max,depth_mean,volume over the zone's pixels of --depth_classes, as in --components, and with --percentiles the
depth_pNN columns.  --zones_raster FILE.tif writes the zone raster itself: int32, nodata -1, Deflate in tiles of 256.  --report gains
a key "zones": "features", "with_pixels" (those with a pixel in the scene) and "pixels" (the scene's pixels in any zone).
Reprojection of the layer, line and point features, an all-touched rule and fractional coverage are outside this tool."""
import argparse
import csv
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from kurosiwo_amd import geotiff                                            # noqa: E402
from kurosiwo_amd.config import load_json5, update_config                   # noqa: E402
from kurosiwo_amd.model_utilities import initialize_cd_model, initialize_segmentation_model      # noqa: E402
from kurosiwo_amd.scene import (basis_points, cd_forward, component_quantiles, component_stats, flood_depth, label_components,      # noqa: E402
                                percentile_name, polygonize, polygons_geojson, predict_scene, quantile_values, rasterize_zones, seg_forward,
                                select_classes, sieve, zonal_geometry, zonal_quantiles, zonal_stats, zones_from_geojson)

CD_METHODS = ("snunet", "changeformer", "siam-conc", "siam-diff", "bit-cd")

parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
parser.add_argument("--task", choices=("cd", "segmentation"), default=None, help="default: what the method decides")
parser.add_argument("--method", required=True)
parser.add_argument("--backbone", default=None)
parser.add_argument("--checkpoint", required=True)
parser.add_argument("--post", nargs="+", required=True)
parser.add_argument("--pre1", nargs="+", default=None)
parser.add_argument("--pre2", nargs="+", default=None)
parser.add_argument("--dem", default=None)
parser.add_argument("--slope", action="store_true", default=False)
parser.add_argument("--nodata", type=float, default=None, help="sentinel of the SAR rasters (default: each file's nodata tag)")
parser.add_argument("--out", required=True)
parser.add_argument("--score", choices=("logits", "softmax"), default=None)
parser.add_argument("--score_out", default=None)
parser.add_argument("--window", type=int, default=224)
parser.add_argument("--stride", type=int, default=112)
parser.add_argument("--weight", choices=("hann", "uniform"), default="hann")
parser.add_argument("--batch_size", type=int, default=32)
parser.add_argument("--precision", choices=("bf16", "fp32"), default="bf16")
parser.add_argument("--tta", choices=("none", "hflip", "flips", "d4"), default="none",
                    help="test-time views blended on the device: the window and its mirror image / the four flips / all eight symmetries")
parser.add_argument("--raw", action="store_true", default=False,
                    help="hand raw windows to a model that normalises inside its first convolution (snunet)")
parser.add_argument("--mmu", type=int, default=None, help="minimum mapping unit in pixels: smaller components take their neighbours' class")
parser.add_argument("--connectivity", type=int, choices=(4, 8), default=4)
parser.add_argument("--sieve_passes", type=int, default=1)
parser.add_argument("--report", default=None, help="FILE.json: per-class pixel counts and areas of the map as written")
parser.add_argument("--polygons", default=None, help="FILE.geojson: the components of --polygon_classes of the map as written, as polygons")
parser.add_argument("--polygon_classes", type=int, nargs="+", default=[1, 2])
parser.add_argument("--components", default=None, help="FILE.csv: one row of statistics per component of --polygon_classes of the map as written")
parser.add_argument("--depth_out", default=None, help="FILE.tif: the water depth of the map as written, in the DEM's unit")
parser.add_argument("--depth_dem", default=None, help="the DEM the depth is taken from, raw, on the scene's grid (default: the file of --dem)")
parser.add_argument("--depth_classes", type=int, nargs="+", default=[1, 2])
parser.add_argument("--percentiles", type=float, nargs="+", default=None,
                    help="percents (50 90 97.5): percentiles of the depth per component and over all water; needs --depth_out and a table")
parser.add_argument("--zones", default=None, help="FILE.geojson: polygons (districts, parcels) to describe the map as written by")
parser.add_argument("--zone_key", default=None, help="the property that names a feature of --zones (default: its index)")
parser.add_argument("--zones_out", default=None, help="FILE.csv: one row of statistics per feature of --zones")
parser.add_argument("--zones_raster", default=None, help="FILE.tif: the int32 zone raster of --zones, nodata -1")
parser.add_argument("--zone_classes", type=int, nargs="+", default=[1, 2], help="the classes counted as flooded per zone")


def read_date(paths, nodata):
    """the files of one date -> (float32 [bands, H, W], sentinel or None, info of the first file)"""
    parts, first, sentinel = [], None, nodata
    for p in paths:
        a, meta = geotiff.read(p, dtype=np.float32, squeeze=False)
        if first is None:
            first = meta
        if nodata is None and meta["nodata"] is not None and not np.isnan(meta["nodata"]):
            if sentinel is not None and sentinel != meta["nodata"]:
                raise SystemExit(f"predict.py: the files of one date carry different nodata tags ({sentinel} and {meta['nodata']}): pass --nodata")
            sentinel = meta["nodata"]
        parts.append(a)
    if any(a.shape[1:] != parts[0].shape[1:] for a in parts):
        raise SystemExit(f"predict.py: rasters of different sizes: {[a.shape for a in parts]}")
    return np.concatenate(parts, axis=0), sentinel, first


def read_dem(path):
    """the DEM as the loaders read it: the sentinel and NaN are gaps, filled from the nearest valid cell on the host"""
    a, meta = geotiff.read(path, dtype=np.float32, squeeze=False)
    if a.shape[0] != 1:
        raise SystemExit(f"predict.py: the DEM has one band, {path} has {a.shape[0]}")
    if meta["nodata"] is not None and not np.isnan(meta["nodata"]):
        a[a == np.float32(meta["nodata"])] = np.nan
    return geotiff.fill_nodata(np.ascontiguousarray(a))


def read_raw_dem(path):
    """the DEM for --depth_out: its values as they are, the nodata tag and NaN as NaN; no gap is filled and nothing is standardised"""
    a, meta = geotiff.read(path, dtype=np.float32, squeeze=False)
    if a.shape[0] != 1:
        raise SystemExit(f"predict.py: the DEM has one band, {path} has {a.shape[0]}")
    a = np.ascontiguousarray(a[0])
    if meta["nodata"] is not None and not np.isnan(meta["nodata"]):
        a[a == np.float32(meta["nodata"])] = np.nan
    return a


COMPONENT_COLUMNS = ("label", "class", "pixels", "x0", "y0", "x1", "y1", "centroid_x", "centroid_y")
DEPTH_COLUMNS = ("depth_pixels", "depth_max", "depth_mean", "volume")
DEPTH_FRAC_BITS, SCORE_FRAC_BITS = 16, 30


def percentile_columns(pcts):
    """the column names of the basis points pcts: depth_p50, depth_p97_5"""
    return tuple("depth_" + percentile_name(c) for c in pcts)


def percentile_cells(zq):
    """the "linear" percentiles of band 0 of a ZonalQuantiles -> one list per percentile, one value per row; None without a finite value"""
    some = (zq.valid[0] > 0).cpu().numpy().tolist()
    return [[v if ok else None for v, ok in zip(column, some)] for column in quantile_values(zq, "linear")[0].tolist()]


def component_table(classes, written, select, depth, score, area, pixel_scale, origin, percents=None):
    """the statistics of the components of the classes `select` of the device map `classes` (`written`: its host copy) -> (Zonal,
    {column: one value per row}): the columns of --components after "label", in order; depth (device float32 [Hs, Ws] or None) adds
    DEPTH_COLUMNS and, with `percents`, one column per percentile; score (device softmax [K, Hs, Ws] or None) adds "confidence".
    None is a null."""
    labels = label_components(classes, 4)
    geom = deep = component_stats(classes, select, values=depth, labels=labels, frac_bits=DEPTH_FRAC_BITS)
    zone, count, box = geom.zone.cpu().numpy(), geom.count.cpu().numpy(), geom.bbox.cpu().numpy()
    _, cx, cy = zonal_geometry(geom, pixel_scale, origin)
    own = written.ravel()[zone].astype(np.int64)
    cols = {"class": own.tolist(), "pixels": count.tolist(), "x0": box[:, 0].tolist(), "y0": box[:, 1].tolist(), "x1": box[:, 2].tolist(),
            "y1": box[:, 3].tolist(), "centroid_x": cx.tolist(), "centroid_y": cy.tolist()}
    if depth is not None:
        n, top, total = deep.valid[0].cpu().numpy(), deep.vmax[0].cpu().numpy(), deep.vsum[0].cpu().numpy()
        metres = total / float(2 ** DEPTH_FRAC_BITS)
        cols["depth_pixels"] = n.tolist()
        cols["depth_max"] = [float(v) if k else None for v, k in zip(top.tolist(), n.tolist())]
        cols["depth_mean"] = [m / k if k else None for m, k in zip(metres.tolist(), n.tolist())]
        cols["volume"] = [None if area is None else m * area for m in metres.tolist()]
        if percents:
            zq = component_quantiles(classes, depth, percents, select, labels=labels)
            assert torch.equal(zq.zone, geom.zone) and torch.equal(zq.valid, deep.valid)
            cols.update(zip(percentile_columns(zq.percentiles), percentile_cells(zq)))
    if score is not None:
        conf = component_stats(classes, select, values=score, labels=labels, frac_bits=SCORE_FRAC_BITS)
        n, total = conf.valid.cpu().numpy(), conf.vsum.cpu().numpy()
        rows = np.arange(zone.size)
        band = np.minimum(own, score.shape[0] - 1)
        k = np.where(own < score.shape[0], n[band, rows], 0).tolist()
        part = (total[band, rows] / float(2 ** SCORE_FRAC_BITS)).tolist()
        cols["confidence"] = [p / c if c else None for p, c in zip(part, k)]
    return geom, cols


def write_components(path, zonal, cols):
    """--components: the header row, then one row per component; repr of a float reads back to the same float64, a null is empty"""
    names = list(cols)
    cell = lambda v: "" if v is None else repr(v) if isinstance(v, float) else str(v)
    with open(path, "w") as f:
        f.write(",".join(["label"] + names) + "\n")
        for r, z in enumerate(zonal.zone.cpu().numpy().tolist()):
            f.write(",".join([str(z)] + [cell(cols[k][r]) for k in names]) + "\n")


ZONE_COLUMNS = ("zone", "id", "pixels", "valid", "class_0", "class_1", "class_2", "class_3", "flooded", "flooded_area", "flooded_fraction")


def zone_table(zones, ids, classes, flooded, area, depth, depth_classes, percents=None):
    """the statistics of the F = len(ids) features of the device zone raster `zones` over the device map `classes` -> {column: one
    value per feature}: the columns of --zones_out, in order; depth (device float32 [Hs, Ws] or None) adds DEPTH_COLUMNS over the
    pixels of depth_classes and, with `percents`, one column per percentile.  Every number is a row of zonal_stats or
    zonal_quantiles put at its zone id; a feature without a row keeps zeros and nulls.  None is a null."""
    F = len(ids)

    def spread(zone, column, fill=0):
        out = [fill] * F
        for z, v in zip(zone.cpu().numpy().tolist(), column.cpu().numpy().tolist()):
            out[z] = v
        return out

    def pixels_of(where):
        rows = zonal_stats(zones, None, where)
        return spread(rows.zone, rows.count)

    per_class = [pixels_of(select_classes(classes, (k,))) for k in range(4)]
    cols = {"zone": list(range(F)), "id": list(ids), "pixels": pixels_of(None)}
    cols["valid"] = [n - k for n, k in zip(cols["pixels"], per_class[3])]
    cols.update((f"class_{k}", per_class[k]) for k in range(4))
    cols["flooded"] = pixels_of(select_classes(classes, flooded))
    cols["flooded_area"] = [None if area is None else n * area for n in cols["flooded"]]
    cols["flooded_fraction"] = [n / v if v else None for n, v in zip(cols["flooded"], cols["valid"])]
    if depth is not None:
        water = select_classes(classes, depth_classes)
        deep = zonal_stats(zones, depth, water, frac_bits=DEPTH_FRAC_BITS)
        n, top = spread(deep.zone, deep.valid[0]), spread(deep.zone, deep.vmax[0], 0.0)
        metres = [v / float(2 ** DEPTH_FRAC_BITS) for v in spread(deep.zone, deep.vsum[0])]
        cols["depth_pixels"] = n
        cols["depth_max"] = [float(v) if k else None for v, k in zip(top, n)]
        cols["depth_mean"] = [m / k if k else None for m, k in zip(metres, n)]
        cols["volume"] = [None if area is None else m * area for m in metres]
        if percents:
            zq = zonal_quantiles(zones, depth, percents, water)
            assert torch.equal(zq.zone, deep.zone) and torch.equal(zq.valid, deep.valid)
            for name, column in zip(percentile_columns(zq.percentiles), percentile_cells(zq)):
                cols[name] = [None] * F
                for z, v in zip(zq.zone.cpu().numpy().tolist(), column):
                    cols[name][z] = v
    return cols


def write_zones(path, cols):
    """--zones_out: the header row, then one row per feature; cells as in --components, quoted where an id needs it"""
    names = list(cols)
    cell = lambda v: "" if v is None else repr(v) if isinstance(v, float) else str(v)
    with open(path, "w", newline="") as f:
        out = csv.writer(f, lineterminator="\n")
        out.writerow(names)
        for r in range(len(cols["zone"])):
            out.writerow([cell(cols[k][r]) for k in names])


def load_model(configs, model_configs, checkpoint):
    if configs["task"] == "cd":
        configs["resume_checkpoint"] = checkpoint
        return initialize_cd_model(configs, model_configs, "test")
    model = initialize_segmentation_model(configs, model_configs)
    ck = torch.load(checkpoint, map_location=configs["device"], weights_only=False)
    if isinstance(ck, torch.nn.Module):                 # main.py saves the whole module for the segmentation task
        return ck.to(configs["device"])
    model.load_state_dict(ck["model_state_dict"] if "model_state_dict" in ck else ck)
    return model


def main(argv=None):
    args = parser.parse_args(argv)
    if args.slope:
        raise SystemExit("predict.py: --slope is not supported: the slope of a whole scene is not computed here (train and map with --dem)")
    if (args.score is None) != (args.score_out is None):
        raise SystemExit("predict.py: --score and --score_out come together")
    if args.sieve_passes < 1:
        raise SystemExit("predict.py: --sieve_passes >= 1")
    if any(not 0 <= c <= 62 for c in args.polygon_classes):
        raise SystemExit("predict.py: --polygon_classes takes class values 0 .. 62")
    if any(not 0 <= c <= 62 for c in args.depth_classes):
        raise SystemExit("predict.py: --depth_classes takes class values 0 .. 62")
    depth_dem = args.depth_dem or args.dem
    if args.depth_out is not None and depth_dem is None:
        raise SystemExit("predict.py: --depth_out needs a DEM: pass --depth_dem (or --dem)")
    pcts = ()
    if args.percentiles is not None:
        if args.depth_out is None or (args.components is None and args.polygons is None and args.report is None):
            raise SystemExit("predict.py: --percentiles needs --depth_out and one of --components, --polygons, --report")
        try:
            pcts = basis_points(args.percentiles, "predict.py: --percentiles")
        except ValueError as e:
            raise SystemExit(str(e)) from None
        if len(set(pcts)) != len(pcts):
            raise SystemExit("predict.py: --percentiles names a percentile twice")
    if args.zones is None and (args.zone_key is not None or args.zones_out is not None or args.zones_raster is not None):
        raise SystemExit("predict.py: --zone_key, --zones_out and --zones_raster need --zones")
    if args.zones is not None and args.zones_out is None and args.zones_raster is None and args.report is None:
        raise SystemExit("predict.py: --zones needs one of --zones_out, --zones_raster, --report")
    if any(not 0 <= c <= 62 for c in args.zone_classes):
        raise SystemExit("predict.py: --zone_classes takes class values 0 .. 62")
    layer = None
    if args.zones is not None:
        with open(args.zones) as f:
            layer = json.load(f)
    method = args.method.lower()
    task = args.task or ("cd" if method in CD_METHODS else "segmentation")
    dates = [(n, p) for n, p in (("pre_event_1", args.pre1), ("pre_event_2", args.pre2)) if p]
    if task == "cd" and len(dates) != 1:
        raise SystemExit("predict.py: change detection takes --post and exactly one of --pre1 / --pre2")
    inputs = [n for n, _ in dates] + ["post_event"]

    configs = load_json5(os.path.join(ROOT, "configs", "config.json"))
    configs["method"], configs["task"] = method, task
    model_configs = load_json5(os.path.join(ROOT, "configs", "method", method, method.replace("-", "_") + ".json"))
    if args.backbone is not None:
        model_configs["backbone"] = args.backbone
    configs.update(model_configs)
    configs = update_config(configs, SimpleNamespace(inputs=inputs, dem=args.dem is not None, slope=False), root=ROOT)
    configs["precision"] = args.precision
    if configs.get("slc"):
        raise SystemExit("predict.py: SLC products are not supported")
    dev = torch.device(configs["device"])

    post, post_nd, geo = read_date(args.post, args.nodata)
    pres = [read_date(p, args.nodata) for _, p in dates]
    raw_dem = None
    if args.depth_out is not None:
        raw_dem = read_raw_dem(depth_dem)
        if raw_dem.shape != post.shape[1:]:
            raise SystemExit(f"predict.py: the DEM of --depth_out is {raw_dem.shape[0]} x {raw_dem.shape[1]}, the scene {post.shape[1]} x "
                             f"{post.shape[2]}: a DEM on another grid is not resampled here")
    sar = (list(configs["data_mean"]), list(configs["data_std"]), [configs["clamp_input"]] * len(configs["data_mean"]))
    if task == "cd":                                    # the order of cd_inputs: [date A, date B(, dem)]
        rasters, nodatas = [pres[0][0], post], [pres[0][1], post_nd]
    else:                                               # the order of seg_inputs: [post(, dem), pre dates]
        rasters, nodatas = [post], [post_nd]
    norms = [sar] * len(rasters)
    if args.dem is not None:
        rasters.append(read_dem(args.dem))
        nodatas.append(None)
        norms = norms + [([configs["dem_mean"]], [configs["dem_std"]], [-1.0])]
    if task != "cd":
        rasters += [p[0] for p in pres]
        nodatas += [p[1] for p in pres]
        norms = norms + [sar] * len(pres)
    if any(r.shape[1:] != post.shape[1:] for r in rasters):
        raise SystemExit(f"predict.py: rasters of different sizes: {[tuple(r.shape) for r in rasters]}")
    if any(r.shape[0] != len(n[0]) for r, n in zip(rasters, norms)):
        raise SystemExit(f'predict.py: every date has the {len(sar[0])} bands {configs["channels"]}, got {[r.shape[0] for r in rasters]}')

    model = load_model(configs, model_configs, args.checkpoint).eval()
    if task == "cd":
        forward = cd_forward(model, method, norms if args.raw else None)
    else:
        if args.raw:
            raise SystemExit("predict.py: --raw needs a model with a fused input pipeline (snunet)")
        forward = seg_forward(model, inputs, dem=args.dem is not None)
    classes, score = predict_scene(forward, [torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in rasters], norms, window=args.window,
                                   stride=args.stride, batch=args.batch_size, weight=args.weight, nodata=nodatas, score=args.score,
                                   raw=args.raw, tta=args.tta)
    removed = 0
    if args.mmu is not None:                            # class 3 is the invalid class of the map: a vote table of at least 4 rows
        classes, gone = sieve(classes, args.mmu, args.connectivity, invalid_class=3, num_classes=max(4, int(configs["num_classes"])),
                              passes=args.sieve_passes)
        removed = int(gone.item())
    where = dict(compression="deflate", tile=(256, 256), pixel_scale=geo["pixel_scale"], origin=geo["origin"])
    written = classes.cpu().numpy()
    geotiff.write(args.out, written, nodata=3, **where)
    print(f"wrote {args.out}: {classes.shape[0]} x {classes.shape[1]} classes" + (
        f", {removed} components below {args.mmu} pixels removed" if args.mmu is not None else ""))
    scale = geo["pixel_scale"]
    area = None if scale is None else float(scale[0]) * float(scale[1])
    depth_report = depth_dev = None
    if args.depth_out is not None:                      # on the map as written: after --mmu
        depth_dev = flood_depth(classes, torch.from_numpy(raw_dem).to(dev), water=args.depth_classes, invalid_class=3)
        depth = depth_dev.cpu().numpy()
        geotiff.write(args.depth_out, depth, nodata=float("nan"), **where)
        deep = depth[np.isin(written, args.depth_classes) & np.isfinite(depth)].astype(np.float64)
        depth_report = {"water_pixels": int(np.isin(written, args.depth_classes).sum()), "with_depth": int(deep.size),
                        "max": float(deep.max()) if deep.size else None, "mean": float(deep.mean()) if deep.size else None,
                        "volume": None if area is None else float(deep.sum()) * area}
        if pcts and args.report is not None:            # one zone: the whole water surface, from the tensor still on the device
            surface = zonal_quantiles(torch.zeros_like(classes, dtype=torch.int32), depth_dev, args.percentiles,
                                      select_classes(classes, args.depth_classes))
            cells = percentile_cells(surface) if surface.zone.numel() else [[None]] * len(pcts)
            depth_report["percentiles"] = {percentile_name(c): cell[0] for c, cell in zip(pcts, cells)}
        print(f"wrote {args.depth_out}: depth at {depth_report['with_depth']} of {depth_report['water_pixels']} pixels of classes "
              f"{' '.join(str(c) for c in args.depth_classes)}" + (f", at most {depth_report['max']:.3f}" if deep.size else ""))
    zonal = cols = None
    if args.polygons is not None or args.components is not None:        # the statistics stay on the device until the tables are read
        zonal, cols = component_table(classes, written, args.polygon_classes, depth_dev, score if args.score == "softmax" else None, area,
                                      geo["pixel_scale"], geo["origin"], args.percentiles if pcts else None)
        assert tuple(["label"] + list(cols)) == COMPONENT_COLUMNS + (DEPTH_COLUMNS + percentile_columns(pcts) if depth_dev is not None else ()) + (
            ("confidence",) if args.score == "softmax" else ())
    if args.components is not None:
        write_components(args.components, zonal, cols)
        print(f"wrote {args.components}: {zonal.zone.numel()} components of classes {' '.join(str(c) for c in args.polygon_classes)}")
    zones_report = None
    if layer is not None:                               # on the map as written, the rasters still on the device
        try:
            table, zone_ids = zones_from_geojson(layer, classes.shape[0], classes.shape[1], geo["pixel_scale"], geo["origin"], key=args.zone_key)
        except ValueError as e:
            raise SystemExit(f"predict.py: --zones: {e}") from None
        if table.count > classes.numel():
            raise SystemExit(f"predict.py: --zones has {table.count} features, the scene {classes.numel()} pixels: more zones than pixels "
                             "cannot be told apart")
        zones = rasterize_zones(torch.from_numpy(table.edges).to(dev), torch.from_numpy(table.feature).to(dev), classes.shape[0],
                                classes.shape[1], count=table.count)
        if args.zones_raster is not None:
            geotiff.write(args.zones_raster, zones.cpu().numpy(), nodata=-1, **where)
            print(f"wrote {args.zones_raster}: the zones of {table.count} features")
        if args.zones_out is not None:
            zcols = zone_table(zones, zone_ids, classes, args.zone_classes, area, depth_dev, args.depth_classes, args.percentiles if pcts else None)
            assert tuple(zcols) == ZONE_COLUMNS + (DEPTH_COLUMNS + percentile_columns(pcts) if depth_dev is not None else ())
            write_zones(args.zones_out, zcols)
            inside = zcols["pixels"]
            print(f"wrote {args.zones_out}: {table.count} zones, flooded classes {' '.join(str(c) for c in args.zone_classes)}")
        else:
            inside = zonal_stats(zones).count.cpu().numpy().tolist()
        zones_report = {"features": table.count, "with_pixels": sum(1 for n in inside if n), "pixels": int(sum(inside))}
    if args.report is not None:
        counts = np.bincount(written.ravel(), minlength=4).tolist()
        report = {"pixel_counts": counts, "pixel_area": area, "class_area": None if area is None else [area * c for c in counts],
                  "mmu": args.mmu, "connectivity": args.connectivity, "passes": args.sieve_passes, "components_removed": removed}
        if depth_report is not None:
            report["depth"] = depth_report
        if zonal is not None:
            sizes, ids = cols["pixels"], zonal.zone.cpu().numpy().tolist()
            top = int(np.argmax(sizes)) if sizes else None                # the first maximum: the smallest label on a tie
            report["components"] = {"count": len(ids), "largest": None if top is None else {"label": ids[top], "pixels": sizes[top]}}
        if zones_report is not None:
            report["zones"] = zones_report
        with open(args.report, "w") as f:
            json.dump(report, f, indent=1)
        print(f"wrote {args.report}")
    if args.polygons is not None:
        rings = polygonize(classes, select=args.polygon_classes)
        extra = {k: v for k, v in cols.items() if k in DEPTH_COLUMNS + percentile_columns(pcts) or k == "confidence"}
        collection = polygons_geojson(rings, written, pixel_scale=geo["pixel_scale"], origin=geo["origin"],
                                      attributes=(zonal, extra) if extra else None)
        with open(args.polygons, "w") as f:
            json.dump(collection, f)
        print(f"wrote {args.polygons}: {len(collection['features'])} features, {rings.label.numel()} rings of classes "
              f"{' '.join(str(c) for c in args.polygon_classes)}")
    if score is not None:
        geotiff.write(args.score_out, score.cpu().numpy(), nodata=float("nan"), **where)
        print(f"wrote {args.score_out}: {score.shape[0]} bands of {args.score}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
