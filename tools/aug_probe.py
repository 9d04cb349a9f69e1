"""Timing probe of the augmentation-view kernel (csrc/augment.hip) against its yardstick ksmi_sar_preprocess, HIP events on one
stream in one process, plus the rate of the SSL batch loader on a synthetic archive.

    python tools/aug_probe.py [--out profiles/aug_probe.txt] [--tiles 256] [--threads 16]
"""
import argparse
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def timed(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(iters)])) * 1e3          # microseconds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tiles", type=int, default=256, help="grid cells of the synthetic archive (0: skip the loader part)")
    ap.add_argument("--threads", type=int, default=16)
    a = ap.parse_args()
    from kurosiwo_amd import augment as A
    from kurosiwo_amd.data import preprocess_gpu
    lines = []
    B, C = 32, 6
    g = torch.Generator().manual_seed(0)
    raw = (torch.rand((B, C, 224, 224), generator=g) * 0.2 - 0.01)
    raw[torch.rand(raw.shape, generator=g) < 0.01] = float("nan")
    raw = raw.cuda()
    mean, std = torch.tensor([0.0953, 0.0264] * 3, device="cuda"), torch.tensor([0.0427, 0.0215] * 3, device="cuda")
    pipe = A.Pipeline(crop=(1.0, (0.2, 1.0), (3 / 4, 4 / 3)), hflip=0.5)
    rows = torch.from_numpy(pipe.sample_params(random.Random(0), B)).cuda()
    ident = torch.tensor([[0, 0, 224, 224, 0, 0]] * B, dtype=torch.int32, device="cuda")
    out = torch.empty_like(raw)
    t_pre = timed(lambda: preprocess_gpu(raw, mean, std, 0.15, out=out))
    t_id = timed(lambda: A.apply(raw, ident, mean, std, 0.15, out=out))
    t_aug = timed(lambda: A.apply(raw, rows, mean, std, 0.15, out=out))
    gb = 2 * raw.numel() * 4 / 1e9
    lines.append(f"batch [{B}, {C}, 224, 224] fp32, median of 50 launches, HIP events")
    lines.append(f"ksmi_sar_preprocess           {t_pre:8.1f} us  ({gb / t_pre * 1e6:7.0f} GB/s read+write)")
    lines.append(f"ksmi_augment_views identity   {t_id:8.1f} us  ratio {t_id / t_pre:.2f}")
    lines.append(f"ksmi_augment_views scale .2-1 {t_aug:8.1f} us  ratio {t_aug / t_pre:.2f}")
    if a.tiles:
        from make_synthetic_archive import make
        from kurosiwo_amd.dataset import SSLBatchLoader, SSLDataset
        with tempfile.TemporaryDirectory() as root:
            make(root, [101, 102, 103, 104], tiles_per_act=a.tiles // 4, seed=1, dem=False)
            cfg = dict(root_path=root, channels=["vv", "vh"], clamp_input=0.15, checkpoint_path=root)
            ld = SSLBatchLoader(SSLDataset(cfg), 32, device="cuda", threads=a.threads, seed=1)
            for _ in ld:                      # page cache + allocator warm-up
                pass
            t0, n = time.perf_counter(), 0
            for _ in range(3):
                for (img,) in ld:
                    n += img.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            lines.append(f"SSLBatchLoader batch 32, {a.threads} decode threads: {n / 32 / dt:.1f} batches/s, {n / dt:.0f} cells/s, {6 * n / dt:.0f} tiles/s")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()
