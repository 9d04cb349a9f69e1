"""Grid cells per second of the TRAIN loader that prepare_loaders hands out for --dem [--slope] on a GRD archive (page cache warm), tensors
on the device: the A/B behind profiles/slope_loader_ab.txt.

    python tools/slope_loader_probe.py make ROOT [--cells 32] [--records 6912]
    python tools/slope_loader_probe.py run ROOT --label NAME [--slope 1] [--batches 200] [--warmup 16] [--workers 8] [--threads 16]
                                               [--tree DIR] [--out FILE]

make: `cells` distinct grid-cell folders (tools/make_synthetic_archive.py; writing one takes about a second) and a train index of
`records` entries that walk over them round-robin, so one pass of the shuffled, drop_last train loader is records / 32 batches; every
record is decoded from its files like any other.
run: one process, one configuration, one pass.  --tree DIR imports the package, tools/ and tests/ from another checkout (the parent
commit) instead of this one.  The loader's iterator is created before the first device call (a per-sample DataLoader forks its workers
there).  Every batch is complete on the device (stream synchronised) when its time is taken; the first `warmup` batches are left out.
Reported: cells/s over the whole timed window, and the median over groups of 8 consecutive batches (a DataLoader with 8 workers
delivers in bursts of 8, so single-batch intervals say little).  One json line on stdout, appended to --out when given."""
import argparse
import gzip
import json
import os
import pickle
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 32
SLOPE_MEAN, SLOPE_STD = 2.1277, 67.5048          # configs/train/data_config.json


def use_tree(tree):
    for sub in ("tests", "tools", ""):
        sys.path.insert(0, os.path.join(tree, sub) if sub else tree)


def make(root, cells, records):
    from make_synthetic_archive import make as make_archive
    from test_dataset_cpu import TRAIN, VAL, TEST
    os.makedirs(os.path.join(root, "pickle"), exist_ok=True)
    tr, _ = make_archive(root, TRAIN, tiles_per_act=max(1, cells // len(TRAIN)), seed=1)
    te, _ = make_archive(root, VAL + TEST, tiles_per_act=2, seed=2)
    distinct = list(tr.values())
    index = {f"{r:08x}": dict(distinct[r % len(distinct)]) for r in range(records)}
    pickle.dump(index, gzip.open(os.path.join(root, "pickle", "train.gz"), "wb"))
    pickle.dump(te, gzip.open(os.path.join(root, "pickle", "test.gz"), "wb"))
    print(json.dumps({"made": root, "distinct_cells": len(distinct), "train_records": len(index)}))


def run(a):
    import torch
    from test_dataset_cpu import _configs
    from kurosiwo_amd.data import prepare_loaders
    os.environ["KSMI_DATA"] = "archive"
    cfg = _configs(a.root, dem=True, slope=bool(a.slope), slope_mean=SLOPE_MEAN, slope_std=SLOPE_STD, device="cuda", batch_size=BATCH,
                   num_workers=a.workers, loader_threads=a.threads)
    train, _, _ = prepare_loaders(cfg)
    need = a.warmup + a.batches
    if len(train) < need:
        raise SystemExit(f"the train index gives {len(train)} batches, {need} wanted: make the archive with more --records")
    it = iter(train)
    stream = None
    stamps = []
    for k, b in enumerate(it):
        if k >= need:
            break
        if stream is None:
            stream = torch.cuda.current_stream()
        tensors = [b[p] if b[p].is_cuda else b[p].to("cuda", non_blocking=True) for p in (2, 6, 9, 10)]
        stream.synchronize()
        assert tensors[3].shape == (BATCH, 1, 224, 224)
        stamps.append(time.perf_counter())
    if hasattr(it, "close"):
        it.close()                                   # (the batch loader's producer thread ends)
    del it                                           # (a DataLoader's workers end)
    t = stamps[a.warmup - 1:]                        # t[0]: the end of the warm-up
    groups = [8 * BATCH / (t[i + 8] - t[i]) for i in range(0, len(t) - 8, 8)]
    out = dict(label=a.label, loader=type(train).__name__, slope=bool(a.slope), batch=BATCH, batches=len(t) - 1, warmup=a.warmup,
               workers=a.workers, threads=a.threads, cells_per_s=round((len(t) - 1) * BATCH / (t[-1] - t[0]), 1),
               cells_per_s_median_of_8_batch_groups=round(statistics.median(groups), 1),
               cells_per_s_min_max_of_groups=[round(min(groups), 1), round(max(groups), 1)])
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("make", "run"))
    ap.add_argument("root")
    ap.add_argument("--cells", type=int, default=32)
    ap.add_argument("--records", type=int, default=BATCH * 216)
    ap.add_argument("--label", default="")
    ap.add_argument("--slope", type=int, default=1)
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    use_tree(os.path.abspath(a.tree))
    if a.what == "make":
        make(a.root, a.cells, a.records)
    else:
        run(a)


if __name__ == "__main__":
    main()
