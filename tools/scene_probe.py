"""Where a whole-scene pass spends its time (kurosiwo_amd/scene.py: predict_scene; the numbers behind profiles/scene_probe.txt).

    python tools/scene_probe.py [--size 4480] [--window 224] [--stride 112] [--batch 32] [--precision bf16] [--repeats 5] [--out FILE]
                                [--mmu N [--connectivity 4] [--sieve_only]] [--polygons [--polygons_only]] [--tta SET [SET ...]] [--depth] [--zonal] [--quantiles]
                                [--zones]

A synthetic size x size scene with two dates of 2 channels (seeded, NaNs planted), SNUNet-ECAM (base_channel 32) in eval mode.
After one warm-up pass (code objects, the plans of the full and of the ragged batch) every figure is the median of `repeats` passes:
  pass       predict_scene end to end between two HIP events on the one stream -> windows/s and scene pixels/s
  split      the same loop with an event after each stage of each batch: gather (one launch per raster), forward, accumulate, and
             valid + finalize once per pass; the event pairs are read after the pass's final synchronise
  blend A/B  the blend alone on one fixed batch of logits reused for every batch of the grid: ksmi_scene_accumulate against the same
             sums written as the torch slice loop on the device (acc[:, y:y+h, x:x+w] += weight * logits[i]; wsum[...] += weight)
  bytes/s    of the accumulate launches: logits read once, weight read per window cell, acc and wsum read and written once per touched
             pixel per launch (counted from the grid), over their summed event time; next to the measured HBM rate the README quotes
  sieve      with --mmu N (the numbers behind profiles/sieve_probe.txt): one pass of the minimum mapping unit on a size x size class map
             of three contents -- one class everywhere (a single component: the contended count), speckle_scene of tests/sieve_ref.py,
             a one-pixel checkerboard (at 4-connectivity every pixel its own component) -- as the event time of each entry point:
             ksmi_scene_label (3 launches), ksmi_scene_component_sizes (memset + 1), ksmi_scene_sieve_vote (2), ksmi_scene_sieve_apply
             (1), and their sum; where scipy is installed, scipy.ndimage.label per class on the host for the same map.  --sieve_only
             skips the model passes above.
  polygons   with --polygons (the numbers behind profiles/polygon_probe.txt): kurosiwo_amd.scene.polygonize on a size x size class map of
             the same three contents (the one class is class 1; classes 1 and 2 selected), as the event time of each stage: the
             4-connectivity labels it starts from, ksmi_scene_edge_count, the four scans (pixels, ring heads, ring lengths, turn flags),
             ksmi_scene_edge_emit, the two phases of ksmi_scene_ring_trace (ring minima, ranks), the assembly (ring_heads, ring_table,
             ring_order, ring_verts), and their sum without the labels; then polygons_geojson on the host by the wall clock, where the
             map has at most --geojson_max_rings rings (a Python list per ring: the checkerboard's ten million would take minutes).
             --polygons_only skips the model passes above.
  tta        with --tta SET [SET ...] of none, hflip, flips, d4 (the numbers behind profiles/tta_probe.txt), instead of the passes above:
             per set the pass (predict_scene(tta=SET) end to end) and its split with an event after each stage of each view of each
             batch: gather (ksmi_scene_gather_view, one launch per raster), forward (the model and the fp32 copy of its logits),
             unview (ksmi_scene_unview) and accumulate (ksmi_scene_accumulate_views, one launch per batch); then the launches alone,
             back to back between two events, at one batch and at all windows of the grid: gather_view and unview per view code (0 .. 3
             index arithmetic, 4 .. 7 through the LDS tile transposer), and ksmi_scene_accumulate_views over 8 views against 8
             ksmi_scene_accumulate launches on the same logits.
  depth      with --depth (the numbers behind profiles/depth_probe.txt), instead of the passes above: kurosiwo_amd.scene.flood_depth on a
             size x size class map of three contents -- no water, speckle_scene of tests/sieve_ref.py, one lake (a disc of radius 1500
             at size 4480, scaled with the size: the longest searches a flood map gives) -- over a smooth synthetic DEM, as the event
             time of each stage: shore (ksmi_scene_shore and ksmi_scene_select), cols (ksmi_scene_edt_cols), rows (ksmi_scene_edt_rows
             over the water pixels), depth (ksmi_scene_depth), and their sum; then nearest_feature without `where` on a map whose one
             feature is pixel (0, 0): every pixel walks out to column 0, the worst case of the outward search (at most 3 repeats).
  zonal      with --zonal (the numbers behind profiles/zonal_probe.txt), instead of the passes above: kurosiwo_amd.scene.zonal_stats keyed by
             the 4-connectivity labels of a size x size class map, `where` = its classes 1 and 2, of four contents -- one class
             everywhere (one zone of size^2 pixels: everything the pass combines lands on one row), speckle_scene of
             tests/sieve_ref.py, one lake (the disc of --depth), a one-pixel checkerboard (every selected pixel its own zone: nothing
             to combine, the slot table overflows) -- for B = 0, 1 and 4 value bands, as the event time of each stage: mark
             (ksmi_scene_zonal_mark), scan (ksmi_scan_i32), tables (ksmi_scene_zonal_tables), accumulate (ksmi_scene_zonal_accumulate:
             keys, the pass, keys back), and their sum; the labels they start from are timed apart.  Next to them, in the same call
             on the same maps, the event time of flood_depth and of polygonize end to end.
  quantiles  with --quantiles (the numbers behind profiles/quantile_probe.txt), instead of the passes above:
             kurosiwo_amd.scene.zonal_quantiles with three percentiles (50, 90, 99) of one value band keyed by the 4-connectivity labels
             of a size x size class map, `where` = its classes 1 and 2, of five contents -- the four of --zonal and "sparse": the lake
             with a `where` that keeps one lake pixel in sixteen, about 2 % of the scene.  The value raster is flood_depth of the map
             over the smooth DEM of --depth; a map without a shore (one class everywhere) has no depth, and the DEM itself stands in.
             Per map: the event time of zonal_quantiles end to end, the number of radix passes, and the event time of each stage of
             the same sequence: rows (ksmi_scene_zonal_mark, ksmi_scan_i32 and the read of N, ksmi_scene_quantile_zones), keys
             (ksmi_scene_quantile_keys), sort (ksmi_scene_quantile_sort), select (ksmi_scene_quantile_select).  The yardstick, in the
             same process and alternated with it repeat by repeat, is the library route the project would otherwise call, written
             with torch ops only: the presence flags by index_fill_, their cumsum and the read of N, int64 composites, torch.sort,
             torch.searchsorted for the segment bounds and a gather; its valid, lower and higher are checked equal to
             zonal_quantiles' bit for bit.
  zones      with --zones (the numbers behind profiles/zones_probe.txt), instead of the passes above: kurosiwo_amd.scene.rasterize_zones
             on a size x size scene for three vector layers -- one polygon over the whole scene (4 edges, spans as long as a row), a
             100 x 100 grid of squares turned by 10 degrees about the middle (shared edges, spans of about 45 pixels), and the rings
             polygonize gives for speckle_scene of tests/sieve_ref.py, rasterised back (millions of spans of a pixel or two; the
             result is checked against the component labels).  Per layer: the event time of rasterize_zones end to end, the number
             of radix passes, and the event time of each stage of the same sequence: rows (ksmi_scene_zone_rows and the read of X),
             scan (ksmi_scan_i32), crossings (ksmi_scene_zone_crossings), sort (ksmi_scene_quantile_sort), fill
             (ksmi_scene_zone_fill: the memset and the spans); then, in the same call, the zonal_stats call that follows it (no
             value band).
One json object per line on stdout, appended to --out when given."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
MEASURED_HBM_TBS = 5.9               # README.md: the box's measured HBM ceiling


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4480)
    ap.add_argument("--window", type=int, default=224)
    ap.add_argument("--stride", type=int, default=112)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mmu", type=int, default=None)
    ap.add_argument("--connectivity", type=int, choices=(4, 8), default=4)
    ap.add_argument("--sieve_only", action="store_true", default=False)
    ap.add_argument("--polygons", action="store_true", default=False)
    ap.add_argument("--polygons_only", action="store_true", default=False)
    ap.add_argument("--geojson_max_rings", type=int, default=2_000_000)
    ap.add_argument("--depth", action="store_true", default=False)
    ap.add_argument("--zonal", action="store_true", default=False)
    ap.add_argument("--quantiles", action="store_true", default=False)
    ap.add_argument("--zones", action="store_true", default=False)
    ap.add_argument("--tta", nargs="+",choices=("none", "hflip", "flips", "d4"), default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.scene import (blend_weights, cd_forward, predict_scene, scene_accumulate, scene_finalize, scene_gather, scene_valid,
                                    window_grid)
    from kurosiwo_amd.snunet import SNUNet_ECAM
    if not torch.cuda.is_available():
        raise SystemExit("scene_probe: no GPU: nothing here can be measured on the host")
    ev = lambda: torch.cuda.Event(enable_timing=True)
    med = statistics.median
    lines = []

    def emit(**kv):
        line = json.dumps(kv)
        print(line, flush=True)
        lines.append(line)

    def finish():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")

    if a.depth:
        depth_probe(a, emit, ev, med)
        return finish()
    if a.zonal:
        zonal_probe(a, emit, ev, med)
        return finish()
    if a.quantiles:
        quantile_probe(a, emit, ev, med)
        return finish()
    if a.zones:
        zones_probe(a, emit, ev, med)
        return finish()
    if a.mmu is not None:
        sieve_probe(a, emit, ev, med)
        if a.sieve_only and not a.polygons:
            return finish()
    if a.polygons:
        polygon_probe(a, emit, ev, med)
        if a.polygons_only or a.sieve_only:
            return finish()
    data = load_json5(os.path.join(HERE, "configs", "train", "data_config.json"))
    norm = (data["data_mean"], data["data_std"], [data["clamp_input"]] * 2)
    dev, S, h, K = torch.device("cuda"), a.size, a.window, 3
    g = torch.Generator(device="cpu").manual_seed(4480)
    rasters = []
    for _ in range(2):
        r = (torch.randn((2, S, S), generator=g) * 0.08 + 0.06).to(dev)
        r[0, 100:140, 200:260] = float("nan")
        rasters.append(r)
    torch.manual_seed(0)
    model = SNUNet_ECAM(2, K, base_channel=32, precision=a.precision).to(dev).eval()
    forward = cd_forward(model, "snunet")
    ys_h, xs_h = window_grid(S, S, h, h, a.stride, a.stride)
    total = len(ys_h) * len(xs_h)
    starts = list(range(0, total, a.batch))
    ys, xs = torch.from_numpy(ys_h).to(dev), torch.from_numpy(xs_h).to(dev)
    wt = torch.from_numpy(blend_weights(h, h, "hann")).to(dev)
    dev_norm = tuple(torch.tensor(v, dtype=torch.float32, device=dev) for v in norm)
    if a.tta:
        tta_probe(a, emit, ev, med, forward, rasters, norm, dev_norm, ys, xs, wt, starts, total, K)
        return finish()

    def whole():
        e0, e1 = ev(), ev()
        e0.record()
        out = predict_scene(forward, rasters, [norm, norm], window=h, stride=a.stride, batch=a.batch, weight="hann")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out[0]

    _, first = whole()                                                         # warm-up
    runs = [whole() for _ in range(a.repeats)]
    assert all(torch.equal(first, c) for _, c in runs)                         # the map is the same in every pass, bit for bit
    t = med([ms for ms, _ in runs])
    emit(what="pass", size=S, window=h, stride=a.stride, batch=a.batch, precision=a.precision, windows=total, batches=len(starts),
         ms_median=round(t, 2), ms_all=[round(ms, 2) for ms, _ in runs], windows_per_s=round(total / t * 1e3, 1),
         scene_mpixels_per_s=round(S * S / t * 1e-3, 2), classes=torch.bincount(first.flatten().long(), minlength=4).tolist())

    def split():
        marks, acc, wsum = [], torch.zeros((K, S, S), device=dev), torch.zeros((S, S), device=dev)
        with torch.no_grad():
            for i0 in starts:
                n = min(a.batch, total - i0)
                e = [ev() for _ in range(4)]
                e[0].record()
                tiles = [scene_gather(r, ys, xs, i0, n, h, h, dev_norm, None) for r in rasters]
                e[1].record()
                logits = forward(tiles).float().contiguous()
                e[2].record()
                scene_accumulate(logits, ys, xs, i0, wt, acc, wsum)
                e[3].record()
                marks.append(e)
            f0, f1 = ev(), ev()
            f0.record()
            valid = None
            for r in rasters:
                valid = scene_valid(r, None, valid)
            cls, _ = scene_finalize(acc, wsum, valid, None, 3)
            f1.record()
        torch.cuda.synchronize()
        assert torch.equal(cls, first)
        return [sum(e[j].elapsed_time(e[j + 1]) for e in marks) for j in range(3)] + [f0.elapsed_time(f1)]
    parts = [split() for _ in range(a.repeats)]
    gat, fwd, accu, fin = (med(p[j] for p in parts) for j in range(4))
    emit(what="split", gather_ms=round(gat, 3), forward_ms=round(fwd, 2), accumulate_ms=round(accu, 3), valid_finalize_ms=round(fin, 3),
         scene_kernels_ms=round(gat + accu + fin, 3), scene_kernels_over_forward=round((gat + accu + fin) / fwd, 4))

    # the blend alone: one fixed batch of logits serves every batch of the grid
    lg = (torch.rand((a.batch, K, h, h), generator=g) * 16 - 8).to(dev)
    origins = [(int(y), int(x)) for y in ys_h for x in xs_h]

    def blend(kernel):
        acc, wsum = torch.zeros((K, S, S), device=dev), torch.zeros((S, S), device=dev)
        e0, e1 = ev(), ev()
        e0.record()
        for i0 in starts:
            n = min(a.batch, total - i0)
            if kernel:
                scene_accumulate(lg[:n], ys, xs, i0, wt, acc, wsum)
            else:
                for j in range(n):
                    y, x = origins[i0 + j]
                    acc[:, y:y + h, x:x + h] += wt * lg[j]
                    wsum[y:y + h, x:x + h] += wt
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), acc, wsum
    _, acc_k, wsum_k = blend(True)
    _, acc_t, wsum_t = blend(False)
    same = bool(torch.equal(acc_k, acc_t) and torch.equal(wsum_k, wsum_t))
    tk, tt = [], []
    for _ in range(a.repeats):                                                 # alternating
        tk.append(blend(True)[0])
        tt.append(blend(False)[0])
    touched = 0
    for i0 in starts:                                                          # pixels under the union of each launch's windows
        n = min(a.batch, total - i0)
        rows = {}
        for y, x in origins[i0:i0 + n]:
            rows.setdefault(y, []).append(x)
        cover = np.zeros((S, S), bool)
        for y, cols in rows.items():
            for x in cols:
                cover[y:y + h, x:x + h] = True
        touched += int(cover.sum())
    nbytes = total * K * h * h * 4 + total * h * h * 4 + touched * (K + 1) * 2 * 4
    emit(what="blend", kernel_ms_median=round(med(tk), 3), torch_slice_loop_ms_median=round(med(tt), 2), torch_over_kernel=round(med(tt) / med(tk), 1),
         same_bits=same, accumulate_bytes=nbytes, accumulate_tb_per_s=round(nbytes / med(tk) * 1e-9, 3), measured_hbm_tb_per_s=MEASURED_HBM_TBS,
         launches=len(starts))
    finish()


def tta_probe(a, emit, ev, med, forward, rasters, norm, dev_norm, ys, xs, wt, starts, total, K):
    """predict_scene(tta=SET) per set of a.tta: the pass, its split by stage, then the view launches alone"""
    import torch
    from kurosiwo_amd.scene import (VIEW_SETS, predict_scene, scene_accumulate, scene_accumulate_views, scene_finalize, scene_gather,
                                    scene_gather_view, scene_unview, scene_valid)
    S, h, dev = a.size, a.window, rasters[0].device
    for name in a.tta:
        views = None if name == "none" else VIEW_SETS[name]
        V = 1 if views is None else len(views)

        def whole():
            e0, e1 = ev(), ev()
            e0.record()
            out = predict_scene(forward, rasters, [norm, norm], window=h, stride=a.stride, batch=a.batch, weight="hann", tta=name)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1), out[0]
        _, first = whole()                                                     # warm-up
        runs = [whole() for _ in range(a.repeats)]
        assert all(torch.equal(first, c) for _, c in runs)                     # the map is the same in every pass, bit for bit
        t = med([ms for ms, _ in runs])
        emit(what="tta_pass", tta=name, views=V, size=S, window=h, stride=a.stride, batch=a.batch, precision=a.precision, windows=total,
             batches=len(starts), ms_median=round(t, 2), ms_all=[round(ms, 2) for ms, _ in runs], windows_per_s=round(total / t * 1e3, 1),
             classes=torch.bincount(first.flatten().long(), minlength=4).tolist())

        def split():
            stages, blends = [], []
            acc, wsum = torch.zeros((K, S, S), device=dev), torch.zeros((S, S), device=dev)
            slabs = None if views is None else torch.empty(V * a.batch * K * h * h, device=dev)
            with torch.no_grad():
                for i0 in starts:
                    n = min(a.batch, total - i0)
                    stack = None if views is None else slabs[:V * n * K * h * h].view(V, n, K, h, h)
                    for j, v in enumerate(views or (None,)):
                        e = [ev() for _ in range(4)]
                        e[0].record()
                        if v is None:
                            tiles = [scene_gather(r, ys, xs, i0, n, h, h, dev_norm, None) for r in rasters]
                        else:
                            tiles = [scene_gather_view(r, ys, xs, i0, n, h, h, v, dev_norm, None) for r in rasters]
                        e[1].record()
                        logits = forward(tiles).float().contiguous()
                        e[2].record()
                        if v is not None:
                            scene_unview(logits, v, out=stack[j])
                        e[3].record()
                        stages.append(e)
                    b = (ev(), ev())
                    b[0].record()
                    if views is None:
                        scene_accumulate(logits, ys, xs, i0, wt, acc, wsum)
                    else:
                        scene_accumulate_views(stack, ys, xs, i0, wt, acc, wsum)
                    b[1].record()
                    blends.append(b)
                f0, f1 = ev(), ev()
                f0.record()
                valid = None
                for r in rasters:
                    valid = scene_valid(r, None, valid)
                cls, _ = scene_finalize(acc, wsum, valid, None, 3)
                f1.record()
            torch.cuda.synchronize()
            assert torch.equal(cls, first)
            return [sum(e[j].elapsed_time(e[j + 1]) for e in stages) for j in range(3)] + [sum(b0.elapsed_time(b1) for b0, b1 in blends),
                                                                                           f0.elapsed_time(f1)]
        parts = [split() for _ in range(a.repeats)]
        gat, fwd, unv, accu, fin = (med(p[j] for p in parts) for j in range(5))
        glue = gat + unv + accu + fin
        emit(what="tta_split", tta=name, views=V, gather_ms=round(gat, 3), forward_ms=round(fwd, 2), unview_ms=round(unv, 3),
             accumulate_ms=round(accu, 3), valid_finalize_ms=round(fin, 3), glue_ms=round(glue, 3), model_share=round(fwd / (fwd + glue), 4),
             glue_share=round(glue / (fwd + glue), 4))

    def per_launch_us(fn, reps):
        """median over a.repeats of: `reps` launches back to back between two events, per launch"""
        fn()
        out = []
        for _ in range(a.repeats):
            e0, e1 = ev(), ev()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3 / reps)
        return round(med(out), 2)

    i0 = starts[len(starts) // 2]
    for label, j0, n, reps in (("batch", i0, min(a.batch, total - i0), 100), ("grid", 0, total, 5)):
        out = torch.empty((n, rasters[0].shape[0], h, h), device=dev)
        gather = {"plain": per_launch_us(lambda: scene_gather(rasters[0], ys, xs, j0, n, h, h, dev_norm, None, out=out), reps)}
        for v in range(8):
            gather[str(v)] = per_launch_us(lambda: scene_gather_view(rasters[0], ys, xs, j0, n, h, h, v, dev_norm, None, out=out), reps)
        del out
        x, y = torch.randn((n, K, h, h), device=dev), torch.empty((n, K, h, h), device=dev)
        unview = {str(v): per_launch_us(lambda: scene_unview(x, v, out=y), reps) for v in range(8)}
        copy = per_launch_us(lambda: y.copy_(x), reps)
        emit(what="tta_launches", shape=label, windows=n, gather_bytes=2 * n * rasters[0].shape[0] * h * h * 4, unview_bytes=2 * n * K * h * h * 4,
             gather_us=gather, unview_us=unview, torch_copy_us=copy,
             gather_transposed_over_flipped=round(med(gather[str(v)] for v in (4, 5, 6, 7)) / med(gather[str(v)] for v in (0, 1, 2, 3)), 2),
             unview_transposed_over_flipped=round(med(unview[str(v)] for v in (4, 5, 6, 7)) / med(unview[str(v)] for v in (0, 1, 2, 3)), 2))
        del x, y
    n = min(a.batch, total - i0)
    lg = torch.rand((8, n, K, h, h), device=dev) * 16 - 8
    acc, wsum = torch.zeros((K, S, S), device=dev), torch.zeros((S, S), device=dev)

    def eight():
        for v in range(8):
            scene_accumulate(lg[v], ys, xs, i0, wt, acc, wsum)
    one_us = per_launch_us(lambda: scene_accumulate_views(lg, ys, xs, i0, wt, acc, wsum), 50)
    eight_us = per_launch_us(eight, 50)
    single_us = per_launch_us(lambda: scene_accumulate(lg[0], ys, xs, i0, wt, acc, wsum), 50)
    emit(what="tta_accumulate", windows=n, views=8, accumulate_views_us=one_us, eight_accumulate_launches_us=eight_us,
         one_accumulate_launch_us=single_us, eight_over_one=round(eight_us / one_us, 2))


def depth_probe(a, emit, ev, med):
    """flood_depth on three maps of a.size x a.size, timed per entry point, then nearest_feature on a map with one feature"""
    import numpy as np
    import torch
    from kurosiwo_amd import _lib, scene
    from kurosiwo_amd.runtime import stream_ptr
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import sieve_ref
    S, water, lib, st = a.size, (1, 2), _lib.load(), stream_ptr()
    mask = sum(1 << c for c in water)
    yy, xx = np.mgrid[0:S, 0:S]
    radius = 1500 * S // 4480
    lake = ((yy - S // 2) ** 2 + (xx - S // 2) ** 2 <= radius * radius).astype(np.uint8)
    maps = {"no_water": np.zeros((S, S), np.uint8), "speckle": sieve_ref.speckle_scene(4480, S, S), "lake": lake}
    dem = torch.from_numpy((100.0 + 20.0 * np.sin(yy / 97.0) * np.cos(xx / 131.0)).astype(np.float32)).cuda()
    del yy, xx, lake
    ptr = lambda t: t.data_ptr()
    chk = _lib.check
    new = lambda dtype: torch.empty((S, S), dtype=dtype, device="cuda")
    stages = ("shore", "cols", "rows", "depth")
    for name, m in maps.items():
        d = torch.from_numpy(m).cuda()

        def one_pass():
            edge, wet, near_y, dist2, nearest, depth = (new(t) for t in (torch.uint8, torch.uint8, torch.int32, torch.int32, torch.int32,
                                                                         torch.float32))
            e = [ev() for _ in range(5)]
            e[0].record()
            chk(lib.ksmi_scene_shore(ptr(d), ptr(dem), mask, 3, S, S, ptr(edge), st), "scene_shore")
            chk(lib.ksmi_scene_select(ptr(d), mask, S * S, ptr(wet), st), "scene_select")
            e[1].record()
            chk(lib.ksmi_scene_edt_cols(ptr(edge), S, S, ptr(near_y), st), "scene_edt_cols")
            e[2].record()
            chk(lib.ksmi_scene_edt_rows(ptr(near_y), ptr(wet), S, S, ptr(dist2), ptr(nearest), st), "scene_edt_rows")
            e[3].record()
            chk(lib.ksmi_scene_depth(ptr(d), ptr(dem), ptr(nearest), mask, 3, S * S, ptr(depth), None, st), "scene_depth")
            e[4].record()
            torch.cuda.synchronize()
            return [e[j].elapsed_time(e[j + 1]) for j in range(4)], depth, dist2, int(edge.sum())
        _, first, dist2, shore_pixels = one_pass()                             # warm-up
        whole = scene.flood_depth(d, dem, water)
        assert torch.equal(first.view(torch.int32), whole.view(torch.int32))   # the staged sequence is flood_depth
        runs = [one_pass() for _ in range(a.repeats)]
        assert torch.equal(first.view(torch.int32), runs[-1][1].view(torch.int32))      # equal bits
        t = [med(r[0][j] for r in runs) for j in range(4)]
        wet = (d == 1) | (d == 2)
        far = int(dist2[wet & (dist2 < scene.EDT_FAR)].max()) if shore_pixels else None
        emit(what="depth", content=name, size=S, water_pixels=int(wet.sum()), shore_pixels=shore_pixels, largest_dist2=far,
             **{k + "_ms": round(v, 3) for k, v in zip(stages, t)}, total_ms=round(sum(t), 3), mpixels_per_s=round(S * S / sum(t) * 1e-3, 1))
        del runs, first, whole, dist2
    one = torch.zeros((S, S), dtype=torch.uint8, device="cuda")
    one[0, 0] = 1                                                              # every pixel walks out to column 0: the longest search

    def transform():
        e = [ev() for _ in range(3)]
        e[0].record()
        near_y = scene.nearest_feature_columns(one)
        e[1].record()
        dist2, nearest = scene.nearest_feature_rows(near_y)
        e[2].record()
        torch.cuda.synchronize()
        return [e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])], dist2, nearest
    _, dist2, nearest = transform()                                            # warm-up
    ramp = torch.arange(S, device="cuda", dtype=torch.int32) ** 2
    assert torch.equal(dist2, ramp[:, None] + ramp[None, :]) and not bool(nearest.any())
    runs = [transform()[0] for _ in range(min(a.repeats, 3))]
    cols, rows = (med(r[j] for r in runs) for j in range(2))
    emit(what="nearest_feature", content="single_feature_at_0_0", size=S, cols_ms=round(cols, 3), rows_ms=round(rows, 3),
         total_ms=round(cols + rows, 3), mpixels_per_s=round(S * S / (cols + rows) * 1e-3, 1))


def zonal_probe(a, emit, ev, med):
    """zonal_stats on four maps of a.size x a.size for B = 0, 1, 4, timed per entry point; flood_depth and polygonize beside them"""
    import numpy as np
    import torch
    from kurosiwo_amd import _lib, scene
    from kurosiwo_amd.runtime import stream_ptr
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import sieve_ref
    S, lib, st = a.size, _lib.load(), stream_ptr()
    HW = S * S
    yy, xx = np.mgrid[0:S, 0:S]
    radius = 1500 * S // 4480
    lake = ((yy - S // 2) ** 2 + (xx - S // 2) ** 2 <= radius * radius).astype(np.uint8)
    maps = {"one_class": np.ones((S, S), np.uint8), "speckle": sieve_ref.speckle_scene(4480, S, S), "lake": lake,
            "checkerboard": ((yy + xx) & 1).astype(np.uint8)}
    dem = torch.from_numpy((100.0 + 20.0 * np.sin(yy / 97.0) * np.cos(xx / 131.0)).astype(np.float32)).cuda()
    del yy, xx, lake
    g = torch.Generator(device="cpu").manual_seed(4480)
    values = torch.randn((4, S, S), generator=g).cuda()
    values[1, 100:140, 200:260] = float("nan")
    ptr = lambda t: None if t is None else t.data_ptr()
    chk = _lib.check
    need = int(lib.ksmi_scan_i32_scratch(HW))
    stages = ("mark", "scan", "tables", "accumulate")

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    for name, m in maps.items():
        d = torch.from_numpy(m).cuda()
        labels_ms = med(timed(lambda: scene.label_components(d, 4))[0] for _ in range(a.repeats + 1))
        labels, where = scene.label_components(d, 4), scene.select_classes(d, (1, 2))
        for B in (0, 1, 4):
            v = values[:B].contiguous() if B else None

            def one_pass():
                present, row = (torch.empty(HW, dtype=torch.int32, device="cuda") for _ in range(2))
                total = torch.zeros(1, dtype=torch.int64, device="cuda")
                scratch = torch.empty(max(need, 1), dtype=torch.int32, device="cuda")
                e = [ev() for _ in range(5)]
                e[0].record()
                chk(lib.ksmi_scene_zonal_mark(ptr(labels), ptr(where), HW, ptr(present), st), "scene_zonal_mark")
                e[1].record()
                chk(lib.ksmi_scan_i32(ptr(present), ptr(row), HW, ptr(total), ptr(scratch), need, st), "scan_i32")
                e[2].record()
                N = int(total.item())                                          # the one host read: the tables are sized by it
                i32 = lambda *s: torch.empty(s, dtype=torch.int32, device="cuda")
                i64 = lambda *s: torch.empty(s, dtype=torch.int64, device="cuda")
                z = scene.Zonal(i32(N), i32(N), i32(N, 4), i64(N), i64(N), i32(B, N), torch.empty((B, N), device="cuda"),
                                torch.empty((B, N), device="cuda"), i64(B, N), 16)
                band = [ptr(t) if B else None for t in (z.valid, z.vmin, z.vmax, z.vsum)]
                f = [ev() for _ in range(3)]
                f[0].record()
                if N:
                    chk(lib.ksmi_scene_zonal_tables(ptr(present), ptr(row), HW, N, B, ptr(z.zone), ptr(z.count), ptr(z.bbox), ptr(z.sum_x),
                                                    ptr(z.sum_y), *band, st), "scene_zonal_tables")
                f[1].record()
                if N:
                    chk(lib.ksmi_scene_zonal_accumulate(ptr(labels), ptr(where), ptr(v), B, S, S, 16, ptr(row), N, ptr(z.count), ptr(z.bbox),
                                                        ptr(z.sum_x), ptr(z.sum_y), *band, st), "scene_zonal_accumulate")
                f[2].record()
                torch.cuda.synchronize()
                return [e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), f[0].elapsed_time(f[1]), f[1].elapsed_time(f[2])], z
            _, first = one_pass()                                              # warm-up
            whole = scene.zonal_stats(labels, v, where, 16)
            same = lambda p, q: all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
                                    for x, y in zip(p[:-1], q[:-1]))
            assert same(first, whole)                                          # the staged sequence is zonal_stats
            runs = [one_pass() for _ in range(a.repeats)]
            assert same(first, runs[-1][1])                                    # equal bits
            t = [med(r[0][j] for r in runs) for j in range(4)]
            emit(what="zonal", content=name, size=S, bands=B, zones=int(first.zone.numel()), largest_zone=int(first.count.max()) if first.zone.numel() else 0,
                 labels_ms=round(labels_ms, 3), **{k + "_ms": round(x, 3) for k, x in zip(stages, t)}, total_ms=round(sum(t), 3),
                 mpixels_per_s=round(HW / sum(t) * 1e-3, 1))
            del runs, first, whole
        depth_ms = med(timed(lambda: scene.flood_depth(d, dem))[0] for _ in range(a.repeats + 1))
        polygon_ms = med(timed(lambda: scene.polygonize(d, (1, 2), labels=labels))[0] for _ in range(min(a.repeats, 3) + 1))
        emit(what="zonal_beside", content=name, size=S, flood_depth_ms=round(depth_ms, 3), polygonize_ms=round(polygon_ms, 3))
        del d, labels, where


def quantile_probe(a, emit, ev, med):
    """zonal_quantiles on five maps of a.size x a.size, timed whole and per stage, against torch.sort on the same composites"""
    import numpy as np
    import torch
    from kurosiwo_amd import _lib, scene
    from kurosiwo_amd.runtime import stream_ptr
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import sieve_ref
    S, lib, st = a.size, _lib.load(), stream_ptr()
    HW = S * S
    percents = (50, 90, 99)
    pcts = scene.basis_points(percents)
    P = len(pcts)
    yy, xx = np.mgrid[0:S, 0:S]
    radius = 1500 * S // 4480
    lake = ((yy - S // 2) ** 2 + (xx - S // 2) ** 2 <= radius * radius).astype(np.uint8)
    maps = {"one_class": np.ones((S, S), np.uint8), "speckle": sieve_ref.speckle_scene(4480, S, S), "lake": lake,
            "checkerboard": ((yy + xx) & 1).astype(np.uint8), "sparse": lake}
    dem = torch.from_numpy((100.0 + 20.0 * np.sin(yy / 97.0) * np.cos(xx / 131.0)).astype(np.float32)).cuda()
    del yy, xx, lake
    g = torch.Generator(device="cpu").manual_seed(4480)
    thin = (torch.rand((S, S), generator=g) < 1.0 / 16.0).to(torch.uint8).cuda()
    ptr = lambda t: None if t is None else t.data_ptr()
    chk = _lib.check
    scan_need, sort_need = int(lib.ksmi_scan_i32_scratch(HW)), int(lib.ksmi_scene_quantile_scratch(HW))
    host_pcts = (_lib.C.c_int32 * P)(*pcts)
    stages = ("rows", "keys", "sort", "select")
    bits = lambda t: t.view(torch.int32)

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def staged(labels, where, v):
        present, row = (torch.empty(HW, dtype=torch.int32, device="cuda") for _ in range(2))
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        scratch = torch.empty(max(scan_need, 1), dtype=torch.int32, device="cuda")
        keys, alt = (torch.empty(HW, dtype=torch.int64, device="cuda") for _ in range(2))
        counters = torch.empty(sort_need, dtype=torch.int32, device="cuda")
        e = [ev() for _ in range(5)]
        e[0].record()
        chk(lib.ksmi_scene_zonal_mark(ptr(labels), ptr(where), HW, ptr(present), st), "scene_zonal_mark")
        chk(lib.ksmi_scan_i32(ptr(present), ptr(row), HW, ptr(total), ptr(scratch), scan_need, st), "scan_i32")
        N = int(total.item())                                                  # the one host read
        zone, valid = torch.empty(N, dtype=torch.int32, device="cuda"), torch.empty((1, N), dtype=torch.int32, device="cuda")
        lower, higher = (torch.empty((1, P, N), dtype=torch.float32, device="cuda") for _ in range(2))
        chk(lib.ksmi_scene_quantile_zones(ptr(present), ptr(row), HW, N, ptr(zone), st), "scene_quantile_zones")
        e[1].record()
        chk(lib.ksmi_scene_quantile_keys(ptr(labels), ptr(where), ptr(v), ptr(row), HW, N, ptr(keys), st), "scene_quantile_keys")
        e[2].record()
        chk(lib.ksmi_scene_quantile_sort(ptr(keys), ptr(alt), HW, N, ptr(counters), sort_need, st), "scene_quantile_sort")
        e[3].record()
        ordered = keys if lib.ksmi_scene_quantile_passes(N) % 2 == 0 else alt
        chk(lib.ksmi_scene_quantile_select(ptr(ordered), HW, N, host_pcts, P, ptr(valid), ptr(lower), ptr(higher), st), "scene_quantile_select")
        e[4].record()
        torch.cuda.synchronize()
        return [e[j].elapsed_time(e[j + 1]) for j in range(4)], scene.ZonalQuantiles(zone, valid, lower, higher, pcts)

    def library_route(labels, where, v):
        """the same table through torch ops: flags, cumsum, int64 composites, torch.sort, searchsorted, gather"""
        z = labels.view(-1).long()
        w = v.view(-1)
        live = (z >= 0) & (z < HW) & (where.view(-1) != 0)
        present = torch.zeros(HW, dtype=torch.int64, device="cuda").index_fill_(0, z[live], 1)
        row = torch.cumsum(present, 0) - present
        N = int(present.sum().item())                                          # the same one host read
        part = live & torch.isfinite(w)
        b = bits(w).long() & 0xFFFFFFFF
        key = b ^ torch.where(b >> 31 != 0, 0xFFFFFFFF, 0x80000000)
        comp = torch.where(part, (row[z.clamp(0, HW - 1)] << 32) | key, torch.iinfo(torch.int64).max)
        ordered = torch.sort(comp).values
        bounds = torch.searchsorted(ordered, torch.arange(N + 1, dtype=torch.int64, device="cuda") << 32)
        n = bounds[1:] - bounds[:-1]
        c = torch.tensor(pcts, dtype=torch.int64, device="cuda")[:, None]
        pos = c * (n - 1).clamp(min=0)[None, :]
        k, frac = pos // 10000, pos % 10000
        top = HW - 1
        unkey = lambda q: (q ^ torch.where(q >> 31 != 0, 0x80000000, 0xFFFFFFFF)).to(torch.int32)      # wraps to the float's bits
        pick = lambda i: torch.where(n[None, :] > 0, unkey(ordered[(bounds[:-1][None, :] + i).clamp(max=top)] & 0xFFFFFFFF), 0x7FC00000)
        return n.to(torch.int32), pick(k), pick(k + (frac > 0))

    for name, m in maps.items():
        d = torch.from_numpy(m).cuda()
        labels, where = scene.label_components(d, 4), scene.select_classes(d, (1, 2))
        if name == "sparse":
            where = where * thin
        v = scene.flood_depth(d, dem)
        if not bool(torch.isfinite(v).any()):                                  # no shore: the DEM stands in for the depth
            v = dem
        _, first = staged(labels, where, v)                                    # warm-up
        whole = scene.zonal_quantiles(labels, v, percents, where)
        same = lambda p, q: all(torch.equal(bits(x) if x.dtype == torch.float32 else x, bits(y) if y.dtype == torch.float32 else y)
                                for x, y in zip(p[:-1], q[:-1]))
        assert same(first, whole)                                              # the staged sequence is zonal_quantiles
        n, lo, hi = library_route(labels, where, v)                            # warm-up, and the check
        assert torch.equal(n, whole.valid[0]) and torch.equal(lo.to(torch.int32), bits(whole.lower[0])) and torch.equal(
            hi.to(torch.int32), bits(whole.higher[0]))
        del n, lo, hi
        ours, theirs, split = [], [], []
        for _ in range(a.repeats):                                             # alternated
            ours.append(timed(lambda: scene.zonal_quantiles(labels, v, percents, where))[0])
            theirs.append(timed(lambda: library_route(labels, where, v))[0])
            t, again = staged(labels, where, v)
            split.append(t)
        assert same(first, again)                                              # equal bits
        t = [med(r[j] for r in split) for j in range(4)]
        N = int(first.zone.numel())
        emit(what="quantiles", content=name, size=S, percentiles=P, zones=N, taking_part=int(whole.valid.sum()),
             kept_by_where=round(float(where.count_nonzero()) / HW, 4), radix_passes=int(lib.ksmi_scene_quantile_passes(N)),
             zonal_quantiles_ms=round(med(ours), 3), torch_sort_route_ms=round(med(theirs), 3), ratio=round(med(ours) / med(theirs), 3),
             **{k + "_ms": round(x, 3) for k, x in zip(stages, t)}, staged_total_ms=round(sum(t), 3))
        del d, labels, where, v, first, whole, again


def zones_probe(a, emit, ev, med):
    """rasterize_zones on three vector layers over a.size x a.size, timed whole and per stage, and the zonal_stats call after it"""
    import numpy as np
    import torch
    from kurosiwo_amd import _lib, scene
    from kurosiwo_amd.runtime import stream_ptr
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import sieve_ref
    S, lib, st = a.size, _lib.load(), stream_ptr()
    ptr = lambda t: None if t is None else t.data_ptr()
    chk = _lib.check
    stages = ("rows", "scan", "crossings", "sort", "fill")

    def timed(fn):
        e0, e1 = ev(), ev()
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def staged(edges, feature, F):
        E = edges.shape[0]
        zones = torch.empty((S, S), dtype=torch.int32, device="cuda")
        counts = torch.empty(E, dtype=torch.int32, device="cuda")
        info = torch.empty(2, dtype=torch.int64, device="cuda")
        total = torch.zeros(1, dtype=torch.int64, device="cuda")
        scan_need = int(lib.ksmi_scan_i32_scratch(E))
        scratch = torch.empty(max(scan_need, 1), dtype=torch.int32, device="cuda")
        e = [ev() for _ in range(6)]
        e[0].record()
        chk(lib.ksmi_scene_zone_rows(ptr(edges), ptr(feature), E, F, S, S, ptr(counts), ptr(info), st), "scene_zone_rows")
        X, refused = info.tolist()                                             # the one host read
        assert not refused and X % 2 == 0 and 0 < X < 2 ** 31
        e[1].record()
        chk(lib.ksmi_scan_i32(ptr(counts), ptr(counts), E, ptr(total), ptr(scratch), scan_need, st), "scan_i32")
        e[2].record()
        n_keys = max(X, F)
        keys, alt = (torch.empty(n_keys, dtype=torch.int64, device="cuda") for _ in range(2))
        sort_need = int(lib.ksmi_scene_quantile_scratch(n_keys))
        counters = torch.empty(sort_need, dtype=torch.int32, device="cuda")
        chk(lib.ksmi_scene_zone_crossings(ptr(edges), ptr(feature), ptr(counts), E, X, S, S, ptr(keys), n_keys, st), "scene_zone_crossings")
        e[3].record()
        chk(lib.ksmi_scene_quantile_sort(ptr(keys), ptr(alt), n_keys, F, ptr(counters), sort_need, st), "scene_quantile_sort")
        e[4].record()
        ordered = keys if lib.ksmi_scene_quantile_passes(F) % 2 == 0 else alt
        chk(lib.ksmi_scene_zone_fill(ptr(ordered), X, F, S, S, ptr(zones), st), "scene_zone_fill")
        e[5].record()
        torch.cuda.synchronize()
        lengths = (ordered[1:X:2] & 0xFFFF) - (ordered[0:X:2] & 0xFFFF)
        return [e[j].elapsed_time(e[j + 1]) for j in range(5)], zones, X, float(lengths.double().mean())

    def ring_layer(rings):
        """the ring table of polygonize as an edge table, vertices times 256, one feature per component in ascending label"""
        V = rings.verts.shape[0]
        k = torch.arange(V, dtype=torch.int64, device="cuda")
        start = rings.start.long()
        ring = torch.searchsorted(start[1:].contiguous(), k, right=True)
        nxt = torch.where(k + 1 == start[1:][ring], start[:-1][ring], k + 1)
        labels, rank = torch.unique(rings.label, return_inverse=True)
        edges = (torch.cat((rings.verts, rings.verts[nxt]), dim=1) * 256).contiguous()
        return edges, rank[ring].to(torch.int32).contiguous(), int(labels.numel()), labels

    layers = {}
    rect = np.array([[-256, -256], [S * 256 + 256, -256], [S * 256 + 256, S * 256 + 256], [-256, S * 256 + 256]], np.int64)
    layers["one_polygon"] = (np.concatenate((rect, np.roll(rect, -1, axis=0)), axis=1).astype(np.int32), np.zeros(4, np.int32), 1)
    n, turn = 100, np.deg2rad(10.0)
    gy, gx = np.mgrid[0:n + 1, 0:n + 1].astype(np.float64) * (S / n) - S / 2.0
    px, py = S / 2.0 + gx * np.cos(turn) - gy * np.sin(turn), S / 2.0 + gx * np.sin(turn) + gy * np.cos(turn)
    q = np.rint(256.0 * np.stack((px, py), axis=2)).astype(np.int64)           # shared corners round once: the squares partition
    quad = np.stack((q[:-1, :-1], q[:-1, 1:], q[1:, 1:], q[1:, :-1]), axis=2).reshape(n * n, 4, 2)
    layers["grid_100x100_turned_10"] = (np.concatenate((quad, np.roll(quad, -1, axis=1)), axis=2).reshape(-1, 4).astype(np.int32),
                                        np.repeat(np.arange(n * n), 4).astype(np.int32), n * n)
    classes = torch.from_numpy(sieve_ref.speckle_scene(4480, S, S)).cuda()
    rings = scene.polygonize(classes)
    edges, feature, F, labels = ring_layer(rings)
    layers["speckle_rings"] = (edges, feature, F)
    boundary_edges = int(scene.boundary_edges(classes, scene.label_components(classes, 4))[0].numel())
    del rings

    for name, (edges, feature, F) in layers.items():
        if not torch.is_tensor(edges):
            edges, feature = torch.from_numpy(edges).cuda(), torch.from_numpy(feature).cuda()
        _, first, X, mean_span = staged(edges, feature, F)                     # warm-up
        whole = scene.rasterize_zones(edges, feature, S, S, count=F)
        assert torch.equal(first, whole)                                       # the staged sequence is rasterize_zones
        if name == "speckle_rings":                                            # back to the components they were traced from
            lab = scene.label_components(classes, 4)
            rank = torch.searchsorted(labels, lab).to(torch.int32)
            assert torch.equal(whole, torch.where(scene.select_classes(classes, (1, 2)) != 0, rank, torch.full_like(rank, -1)))
            del lab, rank
        scene.zonal_stats(whole)                                               # warm-up
        ours, after, split = [], [], []
        for _ in range(a.repeats):
            ours.append(timed(lambda: scene.rasterize_zones(edges, feature, S, S, count=F))[0])
            after.append(timed(lambda: scene.zonal_stats(whole))[0])
            t, again, _, _ = staged(edges, feature, F)
            split.append(t)
        assert torch.equal(first, again)                                       # equal bits
        t = [med(r[j] for r in split) for j in range(5)]
        emit(what="zones", content=name, size=S, edges=int(edges.shape[0]), features=F, crossings=X, spans=X // 2,
             mean_span_pixels=round(mean_span, 2), pixels_in_a_zone=int((whole >= 0).sum()), radix_passes=int(lib.ksmi_scene_quantile_passes(F)),
             **({"unit_boundary_edges": boundary_edges} if name == "speckle_rings" else {}),
             rasterize_zones_ms=round(med(ours), 3), **{k + "_ms": round(x, 3) for k, x in zip(stages, t)}, staged_total_ms=round(sum(t), 3),
             zonal_stats_after_ms=round(med(after), 3))
        del edges, feature, first, whole, again


def sieve_probe(a, emit, ev, med):
    """one pass of the sieve on three maps of a.size x a.size, timed per entry point"""
    import time
    import numpy as np
    import torch
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import stream_ptr
    from kurosiwo_amd.scene import component_sizes, label_components
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import sieve_ref
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    S, K, mmu, conn, lib, st = a.size, 4, a.mmu, a.connectivity, _lib.load(), stream_ptr()
    yy, xx = np.mgrid[0:S, 0:S]
    maps = {"one_class": np.zeros((S, S), np.uint8), "speckle": sieve_ref.speckle_scene(4480, S, S), "checkerboard": ((yy + xx) & 1).astype(np.uint8)}
    del yy, xx
    votes = torch.empty((K, S, S), dtype=torch.int32, device="cuda")
    for name, m in maps.items():
        d = torch.from_numpy(m).cuda()
        out, removed = torch.empty_like(d), torch.zeros(1, dtype=torch.int32, device="cuda")
        ptr = lambda t: t.data_ptr()

        def one_pass():
            e = [ev() for _ in range(5)]
            removed.zero_()
            e[0].record()
            lab = label_components(d, conn)
            e[1].record()
            size = component_sizes(lab)
            e[2].record()
            _lib.check(lib.ksmi_scene_sieve_vote(ptr(d), ptr(lab), ptr(size), mmu, 3, K, S, S, ptr(votes), st), "scene_sieve_vote")
            e[3].record()
            _lib.check(lib.ksmi_scene_sieve_apply(ptr(d), ptr(lab), ptr(size), ptr(votes), mmu, 3, K, S * S, ptr(out), ptr(removed), st),
                       "scene_sieve_apply")
            e[4].record()
            torch.cuda.synchronize()
            return [e[j].elapsed_time(e[j + 1]) for j in range(4)], lab, size
        _, lab, size = one_pass()                                              # warm-up
        components = int((size > 0).sum())
        first = (lab.clone(), out.clone(), int(removed.item()))
        runs = [one_pass() for _ in range(a.repeats)]
        assert torch.equal(runs[-1][1], first[0]) and torch.equal(out, first[1]) and int(removed.item()) == first[2]      # equal bits
        t = [med(r[0][j] for r in runs) for j in range(4)]
        host = None
        if ndimage is not None:
            structure = np.ones((3, 3), int) if conn == 8 else None
            t0 = time.perf_counter()
            n = sum(ndimage.label(m == c, structure)[1] for c in np.unique(m))
            host = round((time.perf_counter() - t0) * 1e3, 1)
            assert n == components
        emit(what="sieve", content=name, size=S, mmu=mmu, connectivity=conn, components=components, removed=first[2],
             label_ms=round(t[0], 3), sizes_ms=round(t[1], 3), vote_ms=round(t[2], 3), apply_ms=round(t[3], 3), total_ms=round(sum(t), 3),
             mpixels_per_s=round(S * S / sum(t) * 1e-3, 1), scipy_label_host_ms=host)


def polygon_probe(a, emit, ev, med):
    """polygonize on three maps of a.size x a.size, timed per stage; the sequence of kurosiwo_amd.scene.polygonize with an event
    between its stages"""
    import time
    import numpy as np
    import torch
    from kurosiwo_amd import _lib, scene
    from kurosiwo_amd.runtime import stream_ptr
    sys.path.insert(0, os.path.join(HERE, "tests"))
    import sieve_ref
    S, select, lib, st = a.size, (1, 2), _lib.load(), stream_ptr()
    mask = sum(1 << c for c in select)
    yy, xx = np.mgrid[0:S, 0:S]
    maps = {"one_class": np.ones((S, S), np.uint8), "speckle": sieve_ref.speckle_scene(4480, S, S), "checkerboard": ((yy + xx) & 1).astype(np.uint8)}
    del yy, xx
    ptr = lambda t: t.data_ptr()
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")
    stages = ("label", "count", "scans", "emit", "trace_min", "trace_rank", "assembly")
    for name, m in maps.items():
        d = torch.from_numpy(m).cuda()

        def one_pass():
            t = dict.fromkeys(stages, 0.0)
            marks = []

            def stage(key, fn):
                e0, e1 = ev(), ev()
                e0.record()
                out = fn()
                e1.record()
                marks.append((key, e0, e1))
                return out
            chk = _lib.check
            lab = stage("label", lambda: scene.label_components(d, 4))
            offs = i32(S * S)
            stage("count", lambda: chk(lib.ksmi_scene_edge_count(ptr(d), ptr(lab), mask, S, S, ptr(offs), st), "scene_edge_count"))
            E = int(stage("scans", lambda: scene._scan(offs, offs, "scan_i32")).item())
            eid, succ, ring_min, rank, ridx, scratch = i32(E), i32(E), i32(E), i32(E), i32(E), i32(4 * E)
            stage("emit", lambda: chk(lib.ksmi_scene_edge_emit(ptr(d), ptr(lab), mask, S, S, ptr(offs), E, ptr(eid), ptr(succ), st), "scene_edge_emit"))
            for key, phase in (("trace_min", 1), ("trace_rank", 2)):
                stage(key, lambda: chk(lib.ksmi_scene_ring_trace(ptr(succ), E, phase, ptr(ring_min), ptr(rank), ptr(scratch), 4 * E, st),
                                       "scene_ring_trace"))
            del scratch
            stage("assembly", lambda: chk(lib.ksmi_scene_ring_heads(ptr(ring_min), E, ptr(ridx), st), "scene_ring_heads"))
            R = int(stage("scans", lambda: scene._scan(ridx, ridx, "scan_i32")).item())
            ring_id, label, roff = i32(R), i32(R), i32(R)
            stage("assembly", lambda: chk(lib.ksmi_scene_ring_table(ptr(eid), ptr(succ), ptr(ring_min), ptr(rank), ptr(ridx), ptr(lab), S * S, E, R,
                                                                    ptr(ring_id), ptr(label), ptr(roff), st), "scene_ring_table"))
            stage("scans", lambda: scene._scan(roff, roff, "scan_i32"))
            oeid, oring, voff = i32(E), i32(E), i32(E)
            stage("assembly", lambda: chk(lib.ksmi_scene_ring_order(ptr(eid), ptr(succ), ptr(ring_min), ptr(rank), ptr(ridx), ptr(roff), E, R,
                                                                    ptr(oeid), ptr(oring), ptr(voff), st), "scene_ring_order"))
            V = int(stage("scans", lambda: scene._scan(voff, voff, "scan_i32")).item())
            verts, start, area2 = i32(2 * V).view(V, 2), i32(R + 1), torch.empty(R, dtype=torch.int64, device="cuda")
            stage("assembly", lambda: chk(lib.ksmi_scene_ring_verts(ptr(oeid), ptr(oring), ptr(voff), E, R, V, S, ptr(verts), ptr(start),
                                                                    ptr(area2), st), "scene_ring_verts"))
            torch.cuda.synchronize()
            for key, e0, e1 in marks:
                t[key] += e0.elapsed_time(e1)
            return t, scene.Rings(label, ring_id, start, area2, verts), E
        _, first, E = one_pass()                                               # warm-up
        whole = scene.polygonize(d, select)
        assert all(torch.equal(x, y) for x, y in zip(first, whole))            # the staged sequence is polygonize
        runs = [one_pass() for _ in range(a.repeats)]
        assert all(torch.equal(x, y) for x, y in zip(first, runs[-1][1]))      # equal bits
        t = {k: med(r[0][k] for r in runs) for k in stages}
        total = sum(v for k, v in t.items() if k != "label")
        R, V = first.label.numel(), first.verts.shape[0]
        host, features = None, None
        if R <= a.geojson_max_rings:
            t0 = time.perf_counter()
            features = len(scene.polygons_geojson(first, d, pixel_scale=(10.0, 10.0), origin=(500000.0, 4100000.0))["features"])
            host = round((time.perf_counter() - t0) * 1e3, 1)
        emit(what="polygons", content=name, size=S, select=list(select), edges=E, rings=R, vertices=V, features=features,
             rounds_per_phase=max(E - 1, 0).bit_length(), **{k + "_ms": round(v, 3) for k, v in t.items()},
             total_without_label_ms=round(total, 3), mpixels_per_s=round(S * S / total * 1e-3, 1), geojson_host_ms=host)
        del runs, first, whole


if __name__ == "__main__":
    main()
