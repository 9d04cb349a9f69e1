#!/usr/bin/env python3
"""Text dump of the launch lists of every model family's plans, for refactors of the plan builders that must not move a launch:
run it on two commits in the same environment and compare the outputs (byte-identical, or `diff` shows the entry that moved).

  python tools/plan_fingerprint.py [--device cpu] [--families snunet,mae,...] > plans.txt ; sha256sum plans.txt

Per plan (every family, constructors as in bench.py; FC-Siam-diff and the other three BIT-CD networks under names of their own; train and eval, bf16 and fp32, 224 x 224, a small batch so that the
convolutional plans fit in host memory; SNUNet also with base_channel 16 at 32 x 32, with tail=1 and with sync_bn) and per list
(packs, fwd, bwd) one line per entry: index, entry name, meta (every key; callables by their presence) and the resolved arguments.
Scalars are literal.  A descriptor passed by reference (ConvDesc, WgradDesc, ...) and the pack / row-sum descriptor tables are
expanded field by field.  Every address, top-level or inside a descriptor, is replaced by the order of its first appearance in the
plan's dump (@0, @1, ...): aliasing and buffer reuse stay visible, absolute addresses do not.  Then `param_ready` and the scratch
table `_need`.  Not a test: every performance change legitimately alters the output.

  python tools/plan_fingerprint.py --arenas > arenas.txt

dumps the parameter arenas instead, for refactors of the model classes that must not move a parameter: every model above (one
precision: the arenas are fp32 either way) plus SNUNet at three more (in_channels, base_channel), each built under
torch.manual_seed(999): the arena lengths, every state_dict() entry in order (key, dtype, shape, sha256 of its bytes) and the
offset tables `_poff`, `_boff`, `_ioff`."""
import argparse
import ctypes as C
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from kurosiwo_amd import _lib  # noqa: E402

# entry points whose first argument is a descriptor table in device memory, args[1] entries long
TABLES = {"ksmi_pack_weights_batched": _lib.PackDesc, "ksmi_reduce_rows_batched": _lib.RowsumDesc,
          "ksmi_reduce_rows_batched_wide": _lib.RowsumDesc}


class Dump:
    def __init__(self, plan, out):
        self.plan, self.out, self.ids = plan, out, {}

    def addr(self, v):
        if hasattr(v, "value"):
            v = v.value
        if not v:
            return "null"
        return f"@{self.ids.setdefault(int(v), len(self.ids))}"

    def field(self, ctype, v):
        if ctype is C.c_void_p:
            return self.addr(v)
        if isinstance(v, C.Structure):
            return self.struct(v)
        if isinstance(v, C.Array):
            return "[" + ",".join(self.field(v._type_, x) for x in v) + "]"
        return repr(v)

    def struct(self, s):
        return type(s).__name__ + "{" + " ".join(f"{k}={self.field(t, getattr(s, k))}" for k, t in s._fields_) + "}"

    def table(self, ptr, n, desc):
        """the n descriptors of a table the plan uploaded (the tensor stays in plan.keep)"""
        t = next(k for k in self.plan.keep if isinstance(k, torch.Tensor) and k.dtype == torch.uint8 and k.data_ptr() == ptr)
        arr = (desc * n).from_buffer_copy(t.cpu().numpy().tobytes())
        return "[" + ",".join(self.struct(d) for d in arr) + "]"

    def arg(self, ctype, v):
        if hasattr(v, "_obj"):                                     # ctypes.byref(descriptor)
            return f"&{self.addr(C.addressof(v._obj))}:{self.struct(v._obj)}"
        if isinstance(v, C.Array):
            return f"{self.addr(C.addressof(v))}:{self.field(type(v), v)}"
        if _lib.sig_codes([ctype]) == "p":
            return self.addr(v)
        return repr(v.value if hasattr(v, "value") else v)

    def entry(self, i, fn, args, name, meta):
        m = " ".join(f"{k}={'<callable>' if callable(v) else repr(v)}" for k, v in sorted(meta.items()))
        if fn is None:                                             # "@wait", "@wait_side", "@allreduce"
            a = [f"tensor{tuple(x.shape)}{self.addr(x.data_ptr())}" if isinstance(x, torch.Tensor) else repr(x) for x in args]
        else:
            types = _lib.SIGNATURES[name][1][:-1]
            assert len(types) == len(args), (name, len(types), len(args))
            a = [self.arg(t, v) for t, v in zip(types, args)]
            if name in TABLES:
                a[0] += ":" + self.table(args[0], args[1], TABLES[name])
        self.out.write(f"{i} {name} | {m} | {' '.join(a)}\n")

    def run(self, title):
        p = self.plan
        self.out.write(f"==== {title}: packs {len(p.packs.calls)} fwd {len(p.fwd.calls)} bwd {len(p.bwd.calls)}\n")
        for lname in ("packs", "fwd", "bwd"):
            self.out.write(f"-- {lname}\n")
            for i, call in enumerate(getattr(p, lname).calls):
                self.entry(i, *call)
        self.out.write("-- param_ready\n")
        for k in sorted(p.param_ready):
            self.out.write(f"{k} {p.param_ready[k]}\n")
        self.out.write("-- need\n")
        for k in sorted(p._need):
            self.out.write(f"{k} {p._need[k]}\n")


def models(family, precision):
    """(title, model, plan arguments of the train plan, of the eval plan) as bench.py constructs each family"""
    H = W = 224
    if family == "snunet":
        from kurosiwo_amd.snunet import SNUNet_ECAM
        yield "snunet B4", SNUNet_ECAM(2, 3, base_channel=32, precision=precision), (4, H, W, True, True), (4, H, W, False, False)
        yield "snunet bc16 32x32 B2", SNUNet_ECAM(2, 3, base_channel=16, precision=precision), (2, 32, 32, True, True), (2, 32, 32, False, False)
        yield "snunet tail=1 B2", SNUNet_ECAM(3, 3, base_channel=32, precision=precision), (2, H, W, True, True, 1), (2, H, W, False, False, 1)
        m = SNUNet_ECAM(2, 3, base_channel=32, precision=precision)
        m.sync_bn = True
        yield "snunet sync_bn B2", m, (2, H, W, True, True), (2, H, W, False, False)
    elif family == "changeformer":
        from kurosiwo_amd.changeformer import ChangeFormerV6
        yield ("changeformer B2", ChangeFormerV6(input_nc=2, output_nc=3, decoder_softmax=True, embed_dim=256, precision=precision),
               (2, H, W, True, True), (2, H, W, False, False))
    elif family == "unet":
        from kurosiwo_amd.unet import Unet
        yield ("unet B2", Unet("resnet18", encoder_weights=None, in_channels=2, classes=3, precision=precision),
               (2, H, W, True, True), (2, H, W, False, False))
    elif family == "siam-conc":
        from kurosiwo_amd.fcsiam import SiamUnet_conc
        yield "siam-conc B2", SiamUnet_conc(2, 3, precision=precision), (2, H, W, True, True), (2, H, W, False, False)
    elif family == "bit-cd":
        from kurosiwo_amd.bitcd import define_G
        yield ("bit-cd base_transformer_pos_s4_dd8 B2", define_G({"net_G": "base_transformer_pos_s4_dd8"}, 2, precision=precision),
               (2, H, W, True, True), (2, H, W, False, False))
    elif family == "siam-diff":
        from kurosiwo_amd.fcsiam import SiamUnet_diff
        yield "siam-diff B2", SiamUnet_diff(2, 3, precision=precision), (2, H, W, True, True), (2, H, W, False, False)
    elif family == "bit-cd-variants":
        from kurosiwo_amd.bitcd import define_G
        for net_g in ("base_resnet18", "base_transformer_pos_s4", "base_transformer_pos_s4_dd8_dedim8"):
            yield f"bit-cd {net_g} B2", define_G({"net_G": net_g}, 2, precision=precision), (2, H, W, True, True), (2, H, W, False, False)
    elif family == "unetplusplus":
        from kurosiwo_amd.unetpp import UnetPlusPlus
        yield ("unetplusplus B2", UnetPlusPlus("resnet18", encoder_weights=None, in_channels=2, classes=3, precision=precision),
               (2, H, W, True, True), (2, H, W, False, False))
    elif family == "floodvit":
        from kurosiwo_amd.floodvit import FinetunerSegmentation, ViT
        enc = ViT(image_size=224, patch_size=16, num_classes=1000, dim=1024, depth=24, heads=16, mlp_dim=2048, channels=6)
        yield "floodvit B2", FinetunerSegmentation(enc, {"decoder": True, "num_classes": 3}, precision=precision), (2, True, True), (2, False, False)
    elif family == "mae":
        from kurosiwo_amd.config import load_json5
        from kurosiwo_amd.mae import build_mae
        mc = load_json5(os.path.join(ROOT, "configs/method/mae/mae.json"))
        yield "mae B2", build_mae(mc, precision=precision, channels=2), (2, True), (2, False)
    else:
        raise SystemExit(f"unknown family {family}")


# (new families are appended: the dump of the earlier names, and its hash in LABNOTES, stays comparable across commits)
FAMILIES = ("snunet", "changeformer", "unet", "siam-conc", "bit-cd", "floodvit", "mae", "siam-diff", "bit-cd-variants", "unetplusplus")


def arena_models(family):
    yield from ((title, model) for title, model, _, _ in models(family, "bf16"))
    if family == "snunet":
        from kurosiwo_amd.snunet import SNUNet_ECAM
        for c, n in ((3, 16), (4, 8), (1, 32)):
            yield f"snunet c{c} bc{n}", SNUNet_ECAM(c, 3, base_channel=n)


def dump_arenas(families, out):
    for family in families:
        it = arena_models(family)
        while True:
            torch.manual_seed(999)                                 # (the generator builds the next model inside next())
            try:
                title, model = next(it)
            except StopIteration:
                break
            out.write(f"==== {title}: params {model.flat_params.numel()} buffers {model.flat_buffers.numel()} "
                      f"counters {model.flat_counters.numel()}\n")
            for k, v in model.state_dict().items():
                digest = hashlib.sha256(v.detach().contiguous().numpy().tobytes()).hexdigest()
                out.write(f"{k} {v.dtype} {tuple(v.shape)} {digest}\n")
            for name in ("_poff", "_boff", "_ioff"):
                out.write(f"-- {name}\n")
                for k, o in getattr(model, name).items():
                    out.write(f"{k} {o}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    ap.add_argument("--families", default=",".join(FAMILIES))
    ap.add_argument("--arenas", action="store_true", help="dump the parameter arenas (CPU) instead of the launch lists")
    args = ap.parse_args()
    if args.arenas:
        dump_arenas(args.families.split(","), sys.stdout)
        return
    dev = torch.device(args.device)
    for family in args.families.split(","):
        for precision in ("bf16", "fp32"):
            torch.manual_seed(999)
            for title, model, train_args, eval_args in models(family, precision):
                model = model.to(dev).train()
                Dump(model.plan(*train_args), sys.stdout).run(f"{title} {precision} train")
                model.eval()
                Dump(model.plan(*eval_args), sys.stdout).run(f"{title} {precision} eval")
                del model
            sys.stdout.flush()


if __name__ == "__main__":
    main()
