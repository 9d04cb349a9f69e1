#!/usr/bin/env python3
"""Train-step throughput of UNet++(resnet18) next to Unet(resnet18) on the same box, timed the way bench.py times `--model unet`:
SegTrainStep (forward + cross entropy + backward + Adam) on bench.py's synthetic batch (seed 999), `--warmup` steps, then `--steps`
steps between one HIP event per step boundary; tiles/s from the wall clock of the timed region, ms from the events.

  python tools/bench_unetpp.py [--batch 32] [--precision bf16] [--steps 20] [--warmup 5] [--models unet,unetplusplus] [--ab]

One JSON line per model.  --ab adds the same-box A/B of the fused BatchNorm-apply + x2 upsample pass (ksmi_affine_relu_upsample2)
against the two-launch pair inside the UNet++ step: the knob KSMI_UNETPP_FUSED_UP=0 / 1 is read when a plan is built, and the two
variants are timed alternately (`--rounds` times each) so that clock drift lands on both."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402


def build(name, B, precision, dev):
    from kurosiwo_amd.synthetic import make_batch, seg_inputs
    from kurosiwo_amd.trainer import SegTrainStep
    from kurosiwo_amd.unet import Unet
    from kurosiwo_amd.unetpp import UnetPlusPlus
    torch.manual_seed(999)
    cls = {"unet": Unet, "unetplusplus": UnetPlusPlus}[name]
    model = cls("resnet18", encoder_weights=None, in_channels=2, classes=3, precision=precision).to(dev).train()
    step = SegTrainStep(model, B, loss_function="cross_entropy", lr=1e-3, bucket_mb=8.0, image_size=(224, 224))
    x, mask = seg_inputs(make_batch(B, 224, 224, seed=999, channels=2), ("post_event",))
    step.set_batch(x.to(dev), mask.to(dev))
    return step


def timed(step, steps, warmup):
    for _ in range(max(warmup, 1)):
        step.run()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        step.run()
    marks[steps].record()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))
    return {"tiles_per_s": round(step.B * steps / dt, 2), "ms_per_step": round(dt / steps * 1e3, 3), "ms_per_step_p50": round(ms[len(ms) // 2], 3),
            "ms_per_step_min_max": [round(ms[0], 3), round(ms[-1], 3)], "loss": float(step.loss_out[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--models", default="unet,unetplusplus")
    ap.add_argument("--ab", action="store_true", help="A/B of KSMI_UNETPP_FUSED_UP inside the UNet++ step")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    box = torch.cuda.get_device_name(0)
    for name in [m for m in args.models.split(",") if m]:
        r = timed(build(name, args.batch, args.precision, dev), args.steps, args.warmup)
        print(json.dumps({"model": name, "batch": args.batch, "precision": args.precision, "steps": args.steps, "warmup": args.warmup, "box": box, **r}),
              flush=True)
    if args.ab:
        steps = {}
        for knob in ("0", "1"):
            os.environ["KSMI_UNETPP_FUSED_UP"] = knob
            steps[knob] = build("unetplusplus", args.batch, args.precision, dev)
        os.environ.pop("KSMI_UNETPP_FUSED_UP")
        for rnd in range(args.rounds):
            for knob in ("0", "1"):
                r = timed(steps[knob], args.steps, args.warmup if rnd == 0 else 1)
                print(json.dumps({"ab": "KSMI_UNETPP_FUSED_UP", "value": knob, "round": rnd, "batch": args.batch, "precision": args.precision,
                                  "box": box, **r}), flush=True)


if __name__ == "__main__":
    main()
