"""Integer oracles, data builders and case tables of the convolution family (csrc/conv_api.hip and its routes into igemm.hip,
igemm2.hip, igemm3.hip, igemm4.hip, wgrad3.hip, the token weight gradient of gemm2.hip and the four slab reducers), shared by
tests/test_gpu_conv_exact.py and tests/test_conv_ref_cpu.py.

With small-integer operands every fp32 partial sum of a convolution is an integer below 2^24, hence exact: summation order, split,
ring depth, MFMA shape and multiply-add contraction cannot change a bit, and the oracle is F.conv2d (and its autograd) in float64
followed by ONE rounding to the storage type (bf16: round to nearest even).  A kernel that drops, doubles or misplaces one term
fails a bit comparison.  The builders assert the preconditions on the CPU for every case (exact() / sum_exact()): every
|accumulator| (from the convolution of the absolute values), every channel's sum |v| and sum v^2 (or sum |v * xhat|) over the WHOLE
tensor -- so that any partition into statistics rows is exact too -- stay below 2^24 quanta.

Data rules: activations and dY integers in [-2, 2]; weights uniform in {-1, 0, 1} (dense: a thinned weight hides a wrong address);
bias, old destinations, residuals, mask / gate arguments integers in [-4, 4] (zeros present: an argument of exactly 0 drops the
value, the `> 0` edge); means integers; rstd in {1/2, 1, 2}; affine and mask scales +-{1/2, 1, 2}; shifts integers; alpha 1/2 or
1/4.  The rounding cases (`big`) use x in [-8, 8], w in [-4, 4] on maps small enough that the statistics stay exact: at least a
tenth of their outputs are not bf16 values before the store and exact ties occur, so a store that rounds half up, truncates, or
sums the unrounded accumulator into the statistics fails.

What the kernels do, as read from the epilogues (igemm_epilogue.h, igemm3.hip, igemm4.hip) and restated by conv_forward():
    v = [relu](alpha * (acc + bias) + resid); mask: v = 0 where m * scale + shift <= 0; statistics of the value rounded to the
    storage type, BEFORE an accumulate: (sum q, sum q^2), with a mask (sum q, sum q * xhat); store round(v + old).
    gate: total = acc + old, zeroed where gate_src <= 0, rounded ONCE, stored; statistics (sum t, sum t * zhat) of the stored total.

Each case carries the route it is meant to reach (`route`): forward [generation, and for igemm4 WM, NF] from
ksmi_conv_dispatch_info, weight gradient [core, reducer, nsplit > 1, bias mode] from ksmi_conv_wgrad_dispatch_info.  Both hooks
are host-only, so the CPU file asserts every route and a row that silently lands on another kernel fails without a GPU.  Only the
run-time knobs are used (KSMI_IGEMM3_CUS, KSMI_IGEMM4_CUS, KSMI_IGEMM4_VAR, KSMI_WGRAD3_WGS, KSMI_WGRAD3_NST).  Switches latched in
a `static` at first use cannot be flipped in-process, so weight-gradient core 2 (the first-generation token GEMM behind
KSMI_GEMM2_TN_OFF) and the three opt-in igemm4 schedules (KSMI_IG4_NW4 / _DEEP / _CHUNK) are out of reach of these files.

Input gradients ("dgrad": the mirrored layer N -> K with flipped, transposed weights, no bias) have rows on every generation and every
igemm4 variant, in bf16 and fp32, wherever the hook keeps the mirror on the generation of its forward row.  Mirrors that change
generation have no row of their own, because the kernel they reach is already covered by the rows of that generation (the hook's
answer in brackets): 32 -> 8 / 16 / 24, 64 -> 128 at 14 x 14, 16 -> 4 x 8 and 64 -> 160 at 35 x 53 [all igemm3: at most two chunks];
fp32 16 -> 8 and 32 -> 16 / 128 [igemm2: whole 16-channel chunks].  The mirrors of the 2- / 3-class heads read a source of channel
stride 8 with 2 or 3 real channels and those of the stride-2 and 4 x 4 layers are phase convolutions: neither is one 3 x 3 descriptor.
The rows x 1 "linear" rows build the descriptor of functional.linear through make_conv (2560 channels: 80 chunks, past the 72 the
chunk tables hold); functional.linear itself is not called.  The composition cases run on igemm3, igemm4 and igemm2; the first
generation has no 3 x 3 layer whose forward, input gradient and functional.conv3x3_wgrad all stay on it."""
import ctypes as C
import functools
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_ref as E  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
LIMIT = 2.0 ** 24
NAN = float("nan")
ints, pick, exact_f32, sum_exact = E.ints, E.pick, E.exact_f32, E.sum_exact
POW2 = [0.5, 1.0, 2.0]
SPOW2 = [-2.0, -1.0, -0.5, 0.5, 1.0, 2.0]


# ------------------------------------------------------------------------------------------------------------------------------
# rounding and layout
# ------------------------------------------------------------------------------------------------------------------------------
def bf16_rne_bits(x32):
    """fp32 -> bf16 bit patterns (int32 in [0, 65536)), round to nearest even, by integer arithmetic on the fp32 bits (finite inputs)"""
    u = x32.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).to(torch.int32)


def stored(x, dtype, what="value"):
    """an exact float64 value as a kernel stores it: + 0.0 (the accumulators start at +0.0), then one rounding to nearest even"""
    return exact_f32(x + 0.0, what).float().to(dtype)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def below_limit(x, what):
    top = float(x.abs().max()) if x.numel() else 0.0
    assert top < LIMIT, f"{what}: {top} is not below 2^24"
    return top


# ------------------------------------------------------------------------------------------------------------------------------
# forward cases
# ------------------------------------------------------------------------------------------------------------------------------
def fwd(name, route, B, H, W, cs, N, k=3, stride=1, pad=None, dtype=BF16, knobs=None, stats=True, bias=True, aff=False, mask=False,
        gate=False, acc=False, extras=None, ostride=None, ndst=1, pack="fwd", big=False, phase=None, seed=0, max_pix=256, uneven=False, kernel=""):
    """One forward descriptor.  cs: channels of the virtual-concat sources; pack: "fwd" (y = conv2d(x, w[N, K, k, k])), "dgrad" (the
    input gradient of the mirrored 3 x 3 layer, weights wl[K, N, 3, 3] flipped and transposed by the packer), "deconv" (the 1 x 1
    pixel-shuffle store of ConvTranspose2d(k2, s2), w[K, N / 4, 2, 2]); phase = (py, px): a 2 x 2 stride-1 phase convolution with
    that top / left padding and strided output placement; extras = alpha (with resid and relu_out); route = [generation(, WM, NF)]"""
    pad = (1 if k == 3 else 0) if pad is None else pad
    return dict(name=name, route=list(route), B=B, H=H, W=W, cs=list(cs), N=N, k=k, stride=stride, pad=pad, dtype=dtype,
                knobs=dict(knobs or {}), stats=stats, bias=bias, aff=aff, mask=mask, gate=gate, acc=acc, extras=extras, ostride=ostride,
                ndst=ndst, pack=pack, big=big, phase=phase, seed=seed, max_pix=max_pix, uneven=uneven, kernel=kernel)


G3 = lambda cus: {"KSMI_IGEMM3_CUS": str(cus)}                      # noqa: E731
G4 = lambda var, cus: {"KSMI_IGEMM4_VAR": var, "KSMI_IGEMM4_CUS": str(cus)}      # noqa: E731


# Grids.  A persistent kernel starts gx0 = CUS * (workgroups per CU) / gy workgroups and then equalises: rounds = ceil(tiles / gx0),
# gx = ceil(tiles / rounds).  The last round is uneven (some workgroups have run out of tiles: the prefetch of a tile that does not
# exist, a statistics row that holds fewer tiles) only when tiles % gx != 0, and a tile edge is ragged only when the kernel's own patch
# does not divide the map -- neither follows from an odd-looking map size, so the rows marked `uneven` are chosen with the hooks and
# tests/test_conv_ref_cpu.py asserts rounds > 1, tiles % gx != 0 and a partial last tile row AND column for each of them:
#   P2 (igemm3 instances with two workgroups per CU: one chunk, 32 columns): 35 x 29 with 128-pixel patches (12 x 10: 9 tiles),
#      CUS 1 -> 2 workgroups x 5 rounds, CUS 3 -> 5 x 2
#   P1 (one workgroup per CU: 64 columns, two chunks, two column tiles): 2 x 31 x 25 (16 x 13 patches: 8 tiles), CUS 1 -> one workgroup
#      walks all 8, CUS 3 -> 3 x 3
#   igemm4 <4,x> and the 2 x 2 phases: 35 x 53 (9 x 27 patches: 8 tiles), CUS 3 -> 3 x 3;  <8,x>: the 512-pixel patch needs 2 x 37 x 41
#      (19 x 21: 8 tiles) for the same -- 3034 pixels, past the 2000 the small-range statistics were sized for, so those two rows rely on
#      the builder's own assertion of the 2^24 condition (sum v^2 stays below 4e6 there)
GRID3 = {"P2": dict(B=1, H=35, W=29, max_pix=128, cus=(1, 3), uneven=(True, True)),
         "P1": dict(B=2, H=31, W=25, max_pix=256, cus=(1, 3), uneven=(False, True)),
         "S2": dict(B=1, H=57, W=57, max_pix=256, cus=(1, 3), uneven=(True, True))}


def _grids3(name, grid, cs, N, **kw):
    """a 3 x 3 igemm3 row at the default grid (31 x 25, ragged) and on two shrunken grids of the preset `grid`"""
    g = GRID3[grid]
    rows = [fwd(name, [3], 1, 31, 25, cs, N, **kw)]
    for cus, un in zip(g["cus"], g["uneven"]):
        rows.append(fwd(f"{name} cus{cus}", [3], g["B"], g["H"], g["W"], cs, N, max_pix=g["max_pix"], knobs=G3(cus), uneven=un, **kw))
    return rows


UN3 = dict(knobs=G3(3), uneven=True)
FWD_CASES = (
    # ---- igemm3, 3 x 3
    _grids3("ig3 32->32", "P2", [32], 32)
    + _grids3("ig3 32->64 WN2", "P1", [32], 64, kernel="igemm3_kernel<3, 3, 1, 2, ")
    + _grids3("ig3 64->32 two chunks", "P1", [64], 32, kernel="igemm3_kernel<3, 3, 2, 1, ")
    + _grids3("ig3 32+32->32 concat", "P1", [32, 32], 32)
    + [r for c in (8, 16, 24) for r in _grids3(f"ig3 {c}->32 partial chunk", "P2", [c], 32)]
    + _grids3("ig3 40->16 partial second chunk", "P1", [40], 16)
    + _grids3("ig3 16->2 stride 8", "P2", [16], 2, ostride=8)
    + _grids3("ig3 32->3 stride 8", "P2", [32], 3, ostride=8)
    + _grids3("ig3 16->3x16 three destinations", "P1", [16], 48, ndst=3)
    + _grids3("ig3 32->32 affine", "P2", [32], 32, aff=True)
    + _grids3("ig3 16->16 mask", "P2", [16], 16, mask=True, bias=False)
    + _grids3("ig3 dgrad 32->32", "P2", [32], 32, pack="dgrad", bias=False)
    + _grids3("ig3 dgrad 64->32", "P1", [64], 32, pack="dgrad", bias=False)
    + _grids3("ig3 dgrad 16->16+16+16", "P1", [16], 48, ndst=3, pack="dgrad", bias=False, stats=False)
    + _grids3("ig3 3x3 stride 2 32->32", "S2", [32], 32, stride=2)
    + _grids3("ig3 bf16 16+8->16", "P1", [16, 8], 16)
    + [fwd("ig3 one tile 64->32", [3], 2, 9, 7, [64], 32),
       fwd("ig3 rounding", [3], 1, 9, 7, [64], 32, big=True, knobs=G3(3))]          # (one tile: the map that keeps sum v^2 exact)
    # ---- igemm3, 2 x 2 stride 2 (the deconv2x2 input gradient) and the 1 x 1 pixel-shuffle store (deconv2x2 forward): 8 or 16
    #      ragged tiles on 3 x 3 or 6 x 3 workgroups
    + [fwd("ig3 2x2s2 32->32", [3], 2, 54, 66, [32], 32, k=2, stride=2, bias=False, max_pix=128, kernel="igemm3_kernel<2, 2, 1, ", **UN3),
       fwd("ig3 2x2s2 64->32", [3], 2, 34, 50, [64], 32, k=2, stride=2, bias=False, kernel="igemm3_kernel<2, 2, 2, ", **UN3),
       fwd("ig3 2x2s2 128->32", [3], 2, 26, 26, [128], 32, k=2, stride=2, bias=False, max_pix=64, kernel="igemm3_kernel<2, 2, 4, ", **UN3)]
    + [fwd(f"ig3 deconv {c}->4x16 stats", [3], 1, 27, 33, [c], 64, k=1, pack="deconv", max_pix=128,
           kernel=f"igemm3_kernel<1, 1, {c // 32}, 2, false, 1, ", **UN3) for c in (64, 128, 256)]
    + [fwd("ig3 deconv 64->4x64 NTI4", [3], 1, 27, 33, [64], 256, k=1, pack="deconv", stats=False, max_pix=128,
           kernel="igemm3_kernel<1, 1, 2, 2, false, 4, ", **UN3),
       fwd("ig3 deconv 128->4x32 NTI2", [3], 1, 27, 33, [128], 128, k=1, pack="deconv", stats=False, max_pix=128,
           kernel="igemm3_kernel<1, 1, 4, 2, false, 2, ", **UN3)]
    # ---- igemm4: every variant forced on a small grid, plus the default choice
    + [fwd("ig4 <4,4> 96->128", [4, 4, 4], 1, 35, 53, [96], 128, knobs=G4("4,4", 3), uneven=True),
       fwd("ig4 <8,4> 96->64", [4, 8, 4], 1, 35, 53, [96], 64, knobs=G4("8,4", 3)),
       fwd("ig4 <8,4> 96->64 uneven", [4, 8, 4], 2, 37, 41, [96], 64, knobs=G4("8,4", 3), uneven=True),
       fwd("ig4 <4,2> 160->64", [4, 4, 2], 1, 35, 53, [160], 64, knobs=G4("4,2", 3), uneven=True),
       fwd("ig4 <4,2> 160->64 one patch", [4, 4, 2], 2, 14, 14, [160], 64, knobs=G4("4,2", 4)),
       fwd("ig4 <8,2> 96->32", [4, 8, 2], 1, 35, 53, [96], 32, knobs=G4("8,2", 3)),
       fwd("ig4 <8,2> 96->32 uneven", [4, 8, 2], 2, 37, 41, [96], 32, knobs=G4("8,2", 3), uneven=True),
       fwd("ig4 default grid 96->32", [4, 8, 2], 2, 130, 126, [96], 32, stats=False),
       fwd("ig4 concat 32+32+64->128", [4, 4, 4], 1, 35, 53, [32, 32, 64], 128, knobs=G4("4,4", 3), uneven=True),
       fwd("ig4 affine 96->64", [4, 8, 4], 2, 14, 14, [96], 64, aff=True, knobs=G4("8,4", 3)),
       fwd("ig4 affine 96->64 <4,2>", [4, 4, 2], 1, 35, 53, [96], 64, aff=True, stats=False, knobs=G4("4,2", 3), uneven=True),
       fwd("ig4 mask 64->64", [4, 4, 2], 1, 35, 53, [64], 64, mask=True, bias=False, knobs=G4("4,2", 3), uneven=True),
       fwd("ig4 mask 64->32", [4, 8, 2], 2, 14, 14, [64], 32, mask=True, bias=False, knobs=G4("8,2", 3)),
       fwd("ig4 gate 64->64", [4, 4, 2], 1, 35, 53, [64], 64, gate=True, bias=False, knobs=G4("4,2", 3), uneven=True),
       fwd("ig4 gate accumulate 96->128", [4, 4, 4], 2, 14, 14, [96], 128, gate=True, acc=True, bias=False, knobs=G4("4,4", 5)),
       fwd("ig4 gate accumulate 64->32", [4, 8, 2], 1, 35, 53, [64], 32, gate=True, acc=True, bias=False, knobs=G4("8,2", 3)),
       fwd("ig4 accumulate 64->64", [4, 8, 4], 1, 35, 53, [64], 64, acc=True, knobs=G4("8,4", 3)),
       fwd("ig4 alpha resid relu 64->128", [4, 4, 4], 2, 14, 14, [64], 128, extras=0.5, knobs=G4("4,4", 5)),
       fwd("ig4 alpha resid relu 64->64", [4, 4, 2], 1, 35, 53, [64], 64, extras=0.25, knobs=G4("4,2", 3), uneven=True),
       fwd("ig4 128->2 stride 8", [4, 8, 2], 1, 35, 53, [128], 2, ostride=8, knobs=G4("8,2", 3)),
       fwd("ig4 96->3 stride 8", [4, 8, 2], 2, 14, 14, [96], 3, ostride=8, knobs=G4("8,2", 3)),
       fwd("ig4 dgrad <8,4> 128->64", [4, 8, 4], 2, 14, 14, [128], 64, pack="dgrad", bias=False, knobs=G4("8,4", 3)),
       fwd("ig4 dgrad <4,4> 96->128", [4, 4, 4], 1, 35, 53, [96], 128, pack="dgrad", bias=False, knobs=G4("4,4", 3), uneven=True),
       fwd("ig4 dgrad <4,2> 96->64", [4, 4, 2], 1, 35, 53, [96], 64, pack="dgrad", bias=False, knobs=G4("4,2", 3), uneven=True),
       fwd("ig4 dgrad <8,2> 96->32", [4, 8, 2], 2, 37, 41, [96], 32, pack="dgrad", bias=False, knobs=G4("8,2", 3), uneven=True),
       fwd("ig4 phase (0,0) 64->128", [4, 4, 4], 1, 35, 53, [64], 128, k=2, phase=(0, 0), knobs=G4("4,4", 3), uneven=True),
       fwd("ig4 phase (1,1) 64->128", [4, 4, 4], 1, 35, 53, [64], 128, k=2, phase=(1, 1), knobs=G4("4,4", 3), uneven=True),
       fwd("ig4 rounding", [4, 4, 2], 1, 9, 7, [96], 64, big=True, knobs=G4("4,2", 4))]
    # ---- igemm2: what the persistent kernels refuse
    + [fwd("ig2 small map 128->64", [2], 1, 14, 14, [128], 64),
       fwd("ig2 partial 16+16+16->16", [2], 1, 31, 25, [16, 16, 16], 16),
       fwd("ig2 partial 8x4->16", [2], 2, 9, 7, [8, 8, 8, 8], 16),
       fwd("ig2 alpha resid relu 128->64", [2], 1, 14, 14, [128], 64, extras=0.25),
       fwd("ig2 accumulate 128->64", [2], 1, 14, 14, [128], 64, acc=True, stats=False),
       fwd("ig2 3x3 stride 2 96->32", [2], 2, 17, 13, [96], 32, stride=2),
       fwd("ig2 4x4 stride 2 32->32", [2], 1, 18, 14, [32], 32, k=4, stride=2, pad=1),
       fwd("ig2 linear 2560->64 uniform chunks", [2], 1, 70, 1, [2560], 64, k=1),
       fwd("ig2 linear accumulate 96->48", [2], 1, 70, 1, [96], 48, k=1, acc=True, stats=False),
       fwd("ig2 dgrad 128->128", [2], 1, 14, 14, [128], 128, pack="dgrad", bias=False),
       fwd("ig2 dgrad fp32 48->32", [2], 1, 12, 9, [48], 32, dtype=F32, pack="dgrad", bias=False),
       fwd("ig2 rounding", [2], 1, 9, 7, [96], 64, big=True)]
    + [fwd(f"ig2 fp32 {c}->32", [2], 1, 12, 9, [c], 32, dtype=F32) for c in (16, 48, 128)]
    # ---- first generation: sources that are not whole chunks where no later kernel takes them.  Its bf16 rows are the only users
    #      of the general LDS-tile epilogue in bf16, hence the bf16 rounding case
    + [fwd("ig1 fp32 8->16", [1], 1, 12, 9, [8], 16, dtype=F32),
       fwd("ig1 fp32 24->16", [1], 2, 9, 7, [24], 16, dtype=F32),
       fwd("ig1 bf16 16+8+16->16", [1], 1, 31, 25, [16, 8, 16], 16),
       fwd("ig1 dgrad fp32 24->16", [1], 2, 9, 7, [24], 16, dtype=F32, pack="dgrad", bias=False),
       fwd("ig1 dgrad bf16 16+8+16->16", [1], 1, 31, 25, [16, 8, 16], 16, pack="dgrad", bias=False),
       fwd("ig1 rounding 24+8+24->16", [1], 1, 9, 7, [24, 8, 24], 16, big=True)]
)
FWD_BY_NAME = {c["name"]: c for c in FWD_CASES}
assert len(FWD_BY_NAME) == len(FWD_CASES)


def out_hw(c):
    if c["phase"] is not None:
        return c["H"], c["W"]
    return (c["H"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"] - c["k"]) // c["stride"] + 1


def _seed(c):
    return 1000 + 37 * sum(map(ord, c["name"])) + c["seed"]


# one plain case per forward generation that also runs on gaussian data under the tolerance of the earlier suites (GAUSS_TOL * max |ref|):
# the same descriptor, packer and oracle code, so an oracle mistake that integers hide (a transposed weight that happens to be
# symmetric in distribution cannot hide, but a wrong scale or a dropped bias on zero-mean data could) shows up there
GAUSS_CASES = ["ig3 32->32 cus3", "ig4 <8,4> 96->64 uneven", "ig2 small map 128->64", "ig1 bf16 16+8+16->16"]
GAUSS_TOL = 2.5e-2


@functools.lru_cache(maxsize=None)
def make_forward(name, gauss=False):
    """every tensor of a forward case on the host: what the kernel reads (storage dtype, NHWC) and what it must leave behind.
    gauss: the same case on bf16-quantised gaussian data and He-scaled weights; nothing is exact then and no precondition is asserted"""
    c = FWD_BY_NAME[name]
    s, dt = _seed(c), c["dtype"]
    B, H, W, cs, N, k = c["B"], c["H"], c["W"], c["cs"], c["N"], c["k"]
    K, (Ho, Wo) = sum(cs), out_hw(c)
    xr, wr = (8, 4) if c["big"] else (2, 1)
    if gauss:
        assert name in GAUSS_CASES and c["pack"] == "fwd" and not (c["aff"] or c["mask"] or c["gate"] or c["acc"] or c["extras"] or c["big"])
        return _make_forward_gauss(c)
    xs = [ints((B, ci, H, W), -xr, xr, s + i) for i, ci in enumerate(cs)]
    t = {"xs": [stored(nhwc(x), dt) for x in xs]}
    src = torch.cat(xs, 1)
    if c["aff"]:
        sc, sh = pick(SPOW2, (K,), s + 10), ints((K,), -2, 2, s + 11)
        t["scale"], t["shift"] = sc.float(), sh.float()
        src = torch.relu(exact_f32(src * sc.view(1, -1, 1, 1), "x * scale") + sh.view(1, -1, 1, 1))
        assert torch.equal(src.float().to(dt).double(), src), "the transformed operand is not a storage value"
    # ---- weights and the linear part, with the accumulator bound from the absolute values
    if c["pack"] == "deconv":
        co = N // 4
        w = ints((K, co, 2, 2), -wr, wr, s + 20)
        wmat = w.permute(2, 3, 1, 0).reshape(N, K, 1, 1)                  # column j = (dy * 2 + dx) * co + n
        conv = lambda a, ww: F.conv2d(a, ww)                              # noqa: E731
    elif c["pack"] == "dgrad":
        w = ints((K, N, 3, 3), -wr, wr, s + 20)                           # the mirrored layer: N channels -> K channels
        wmat = w
        conv = lambda a, ww: F.conv_transpose2d(a, ww, padding=1)         # noqa: E731  (= autograd of conv2d wrt its input)
    else:
        w = ints((N, K, k, k), -wr, wr, s + 20)
        wmat = w
        if c["phase"] is not None:
            py, px = c["phase"]
            conv = lambda a, ww: F.conv2d(F.pad(a, (px, 1 - px, py, 1 - py)), ww)      # noqa: E731
        else:
            conv = lambda a, ww: F.conv2d(a, ww, stride=c["stride"], padding=c["pad"])  # noqa: E731
    t["w"] = w.float()
    y = conv(src, wmat)
    mag = conv(src.abs(), wmat.abs())
    assert y.shape == (B, N, Ho, Wo), (y.shape, (B, N, Ho, Wo))
    if c["bias"]:
        nb = N // 4 if c["pack"] == "deconv" else N
        b = ints((nb,), -4, 4, s + 30)
        t["bias"] = b.float()
        bcol = b.repeat(4) if c["pack"] == "deconv" else b
        y, mag = y + bcol.view(1, -1, 1, 1), mag + bcol.abs().view(1, -1, 1, 1)
    t["acc_max"] = below_limit(mag, "accumulator")
    v = y
    if c["extras"]:
        r = ints((B, N, Ho, Wo), -4, 4, s + 40)
        t["resid"] = stored(nhwc(r), dt)
        v = torch.relu(exact_f32(exact_f32(v * c["extras"], "alpha * (acc + bias)") + r, "+ resid"))
    xh = None
    if c["mask"]:
        m = ints((B, N, Ho, Wo), -4, 4, s + 50)
        mean, rstd, msc, msh = ints((N,), -2, 2, s + 51), pick(POW2, (N,), s + 52), pick(SPOW2, (N,), s + 53), ints((N,), -2, 2, s + 54)
        msh[::2] = 0.0                                                   # the argument is exactly 0 wherever m is: the `> 0` edge
        arg = exact_f32(m * msc.view(1, -1, 1, 1), "m * scale") + msh.view(1, -1, 1, 1)
        assert int((arg == 0).sum()) > 0
        v = torch.where(arg > 0, v, torch.zeros((), dtype=F64))
        xh = exact_f32(exact_f32(m - mean.view(1, -1, 1, 1), "m - mean") * rstd.view(1, -1, 1, 1), "xhat")
        t["mask"] = (stored(nhwc(m), dt), mean.float(), rstd.float(), msc.float(), msh.float())
    old = None
    if c["acc"]:
        old = ints((B, N, Ho, Wo), -4, 4, s + 60)
        t["old"] = stored(nhwc(old), dt)
    if c["gate"]:
        gs, z = ints((B, N, Ho, Wo), -4, 4, s + 70), ints((B, N, Ho, Wo), -4, 4, s + 71)
        mean, rstd = ints((N,), -2, 2, s + 72), pick(POW2, (N,), s + 73)
        assert int((gs == 0).sum()) > 0
        tot = exact_f32(v + old, "total gradient") if old is not None else v
        tot = torch.where(gs > 0, tot, torch.zeros((), dtype=F64))
        q = stored(tot, dt, "gated total")                               # ONE rounding of the total (igemm4.hip, GATE branch)
        out = q
        xh = exact_f32(exact_f32(z - mean.view(1, -1, 1, 1), "z - mean") * rstd.view(1, -1, 1, 1), "zhat")
        t["gate"] = (stored(nhwc(gs), dt), stored(nhwc(z), dt), mean.float(), rstd.float())
    else:
        q = stored(v, dt, "result")
        out = stored(exact_f32(v + old, "result + old"), dt) if old is not None else q    # fp32 sum, one rounding
    t["rounded"] = int((q.double() != v + 0.0).sum()) if not c["gate"] else 0
    if c["big"]:
        assert dt == BF16 and t["rounded"] * 10 >= q.numel(), f"{name}: only {t['rounded']} of {q.numel()} outputs are rounded"
        if True:
            bits = v.float().view(torch.int32) & 0xFFFF
            t["ties"] = int((bits == 0x8000).sum())
            assert t["ties"] > 0, f"{name}: no exact tie"
    # ---- statistics of the stored values: integer (dyadic) totals per column
    qd = q.double()
    second = qd * (xh if xh is not None else qd)
    if c["stats"]:
        sum_exact(qd, (0, 2, 3), f"{name}: sum v")
        sum_exact(second, (0, 2, 3), f"{name}: sum v * xhat | v^2")
    t["stats"] = torch.stack([qd.sum((0, 2, 3)), second.sum((0, 2, 3))]) + 0.0
    t["sq_max"] = float(second.abs().sum((0, 2, 3)).max())
    # ---- the destination(s)
    if c["pack"] == "deconv":
        co = N // 4
        o = out.view(B, 2, 2, co, Ho, Wo).permute(0, 4, 1, 5, 2, 3).reshape(B, 2 * Ho, 2 * Wo, co)     # [b, y, dy, x, dx, n]
        t["outs"] = [o.contiguous()]
    elif c["phase"] is not None:
        py, px = c["phase"]
        o = torch.full((B, 2 * Ho, 2 * Wo, N), NAN, dtype=dt)
        o[:, py::2, px::2] = nhwc(out)
        t["outs"] = [o]
    elif c["ostride"]:
        o = torch.zeros((B, Ho, Wo, c["ostride"]), dtype=dt)             # the pad channels of the last 8-channel group come back zero
        o[..., :N] = nhwc(out)
        t["outs"] = [o]
    else:
        per = N // c["ndst"]
        t["outs"] = [nhwc(out[:, i * per:(i + 1) * per]) for i in range(c["ndst"])]
    return t


def _make_forward_gauss(c):
    s, dt = _seed(c), c["dtype"]
    B, H, W, cs, N, k = c["B"], c["H"], c["W"], c["cs"], c["N"], c["k"]
    K = sum(cs)
    xs = [E.gauss((B, ci, H, W), s + i).float().to(dt).double() for i, ci in enumerate(cs)]
    w = (E.gauss((N, K, k, k), s + 20) * (2.0 / (K * k * k)) ** 0.5).float().to(dt).double()       # (the packer stores the weights in dt)
    b = (E.gauss((N,), s + 30) * 0.1).float().double()
    y = F.conv2d(torch.cat(xs, 1), w, b, stride=c["stride"], padding=c["pad"])
    q = y.float().to(dt)
    return {"xs": [nhwc(x).float().to(dt) for x in xs], "w": w.float(), "bias": b.float(), "ref": nhwc(y), "outs": [nhwc(q)],
            "stats": torch.stack([q.double().sum((0, 2, 3)), (q.double() ** 2).sum((0, 2, 3))]),
            "stats_mag": torch.stack([q.double().abs().sum((0, 2, 3)), (q.double() ** 2).sum((0, 2, 3))])}


def forward_prefill(c, t):
    """what each destination holds before the launch: NaN, or the old integers where the call accumulates"""
    if c["acc"]:
        return [t["old"]]
    return [torch.full(o.shape, NAN, dtype=o.dtype) for o in t["outs"]]


def forward_desc(c, dev_t, outs, stats_buf=None):
    """the descriptor of a forward case over tensors on any device (dev_t: the dict of make_forward with its tensors moved; outs: the
    destinations) -> (descriptor, chunk table, statistics rows).  The packed weights are left to the caller (a device kernel)."""
    from kurosiwo_amd.runtime import SrcSpec, conv_stats_rows, make_conv
    B, H, W, N, k, dt = c["B"], c["H"], c["W"], c["N"], c["k"], c["dtype"]
    Ho, Wo = out_hw(c)
    srcs = [SrcSpec(x, ci) for x, ci in zip(dev_t["xs"], c["cs"])]
    if c["aff"]:
        srcs[0].scale, srcs[0].shift, srcs[0].relu = dev_t["scale"], dev_t["shift"], 1
    per = N // c["ndst"]
    dsts = [(o, o.shape[-1], 0, i * per, per, 1 if c["acc"] else 0) for i, o in enumerate(outs)]
    kw = {}
    if c["phase"] is not None:
        py, px = c["phase"]
        kw.update(pad_x=px, out_map=(2, 2, py, px, 2 * Ho, 2 * Wo))
    if c["extras"]:
        kw.update(alpha=c["extras"], relu_out=1, resid=(dev_t["resid"], N))
    pad = c["phase"][0] if c["phase"] is not None else c["pad"]
    d, table = make_conv(srcs, dsts, outs[0], dev_t.get("bias"), None, B, H, W, Ho, Wo, k, k, c["stride"], pad, N, dt,
                         mask=dev_t.get("mask"), ps_cout=N // 4 if c["pack"] == "deconv" else 0, max_pix=c["max_pix"], **kw)
    if c["gate"]:
        d.gate_src, d.xhat_src, d.g_mean, d.g_rstd = (x.data_ptr() for x in dev_t["gate"])
    rows = 0
    if c["stats"]:
        if stats_buf is None:
            stats_buf = torch.empty((16,), dtype=F32)
        d.stats = stats_buf.data_ptr()
        rows = conv_stats_rows(d, dt)
    d._keep = (srcs, dsts, dev_t, outs, stats_buf)
    return d, table, rows


def forward_pack_args(c, table):
    """arguments of functional._pack after the weight: (table, taps, N, n_mod, sK, sN, sD, sT, flip)"""
    K, N, k = sum(c["cs"]), c["N"], c["k"]
    if c["pack"] == "deconv":
        return table, 1, N, N // 4, N, 4, 1, 0, 0
    if c["pack"] == "dgrad":
        return table, 9, N, N, N * 9, 9, 0, 1, 1
    return table, k * k, N, N, k * k, K * k * k, 0, 1, 0


def ig4_patch512(H, W, pmax=512, hmax=640):
    """the 512-pixel patch of igemm4's <8, x> variants: ig4_patch of csrc/igemm4.hip restated (hmax = IG4_NHMAX * 128 halo pixels); the
    <4, x> variants and igemm3 use the descriptor's TH x TW"""
    best, pick_ = 1e30, (1, 1)
    for tw in range(1, min(W, pmax) + 1):
        for th in range(1, min(H, pmax // tw) + 1):
            hp = (th + 2) * (tw + 2)
            if hp > hmax:
                continue
            cost = (-(-H // th) * -(-W // tw)) * pmax * (1.0 + 0.15 * hp / pmax)
            if cost < best:
                best, pick_ = cost, (th, tw)
    return pick_


def persistent_grid(c, d, info):
    """(tiles, gx, rounds, patch, last tile row partial, last tile column partial) of a case on igemm3 / igemm4"""
    Ho, Wo = out_hw(c)
    th, tw = ig4_patch512(Ho, Wo) if (info[0] == 4 and info[2] == 8) else (d.TH, d.TW)
    tiles, gx = c["B"] * -(-Ho // th) * -(-Wo // tw), info[6]
    return tiles, gx, -(-tiles // gx), (th, tw), Ho % th != 0, Wo % tw != 0


def forward_info(d, dtype):
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import DT
    info = (C.c_int32 * 8)()
    _lib.check(_lib.load().ksmi_conv_dispatch_info(C.byref(d), DT[dtype], info), "conv_dispatch_info")
    return list(info)


def assert_forward_route(c, d):
    info = forward_info(d, c["dtype"])
    want = c["route"]
    got = [info[0]] + ([info[2], info[3]] if len(want) == 3 else [])
    assert got == want and info[1] == 1, (c["name"], want, info)
    return info


FWD_KERNEL = {1: "igemm_fwd_kernel<", 2: "igemm2_fwd_kernel<", 3: "igemm3_kernel<", 4: "igemm4_kernel<"}


def forward_kernel_prefix(c, info):
    """what the launched kernel's name must start with: the generation, for igemm4 WM and NF, and the instance arguments a row promises"""
    if c["kernel"]:
        return c["kernel"]
    if info[0] == 4:
        return f"igemm4_kernel<{info[2]}, {info[3]}, "
    return FWD_KERNEL[info[0]]


# ------------------------------------------------------------------------------------------------------------------------------
# weight-gradient cases
# ------------------------------------------------------------------------------------------------------------------------------
PATCH, TOKEN1, GEMM2, WGRAD3 = 1, 2, 3, 4
RED_NONE, RED_WGRAD3, RED_TREE, RED_TN_TR, RED_TN = 0, 1, 2, 3, 4


def wg(name, route, B, H, W, cs, N, k=3, stride=1, pad=None, dtype=BF16, knobs=None, aff=False, dyC=None, k_real=None, phase=None,
       bias=False, seed=0, kernel="", nt=None):
    """One weight gradient: dW[N, K, k, k] of out = conv(cat(sources), W) given d out (`dy`, N of its dyC channels).  k = 1 with W = 1:
    a token matrix (H rows).  k_real: rows of the weight (the source's remaining channels are pad).  phase = (py, px): the 2 x 2 phase
    gradient over the parity sub-image of a [B, 2H, 2W] source, written through use_tap_off into 4 of 16 taps.
    route = [core, reducer, nsplit > 1, bias mode]"""
    pad = (1 if k == 3 else 0) if pad is None else pad
    return dict(name=name, route=list(route), B=B, H=H, W=W, cs=list(cs), N=N, k=k, stride=stride, pad=pad, dtype=dtype, knobs=dict(knobs or {}),
                aff=aff, dyC=dyC or N, k_real=k_real, phase=phase, bias=bias, seed=seed, kernel=kernel, nt=nt)


W3 = lambda wgs, nst: {"KSMI_WGRAD3_WGS": str(wgs), "KSMI_WGRAD3_NST": str(nst)}      # noqa: E731
R3 = [WGRAD3, RED_WGRAD3]

WG_CASES = (
    # ---- wgrad3
    [wg("wg3 32->16 one chunk", R3, 2, 9, 7, [32], 16, kernel="wgrad3_kernel<2, "),
     wg("wg3 32->32", R3, 1, 33, 19, [32], 32, kernel="wgrad3_kernel<2, "),
     wg("wg3 64->48 WC4 NTL64", R3, 1, 33, 19, [64], 48, kernel="wgrad3_kernel<4, 1, 4, "),
     wg("wg3 96->64", R3, 2, 9, 7, [96], 64),
     wg("wg3 32->2 of 8", R3, 1, 33, 19, [32], 2, dyC=8),
     wg("wg3 64->3 of 8", R3, 2, 9, 7, [64], 3, dyC=8),
     wg("wg3 32+16->32", R3, 1, 33, 19, [32, 16], 32),
     wg("wg3 16+16+16->16", R3, 2, 9, 7, [16, 16, 16], 16),
     wg("wg3 32->32 affine", R3, 1, 33, 19, [32], 32, aff=True),
     wg("wg3 64->64 narrow map", R3, 2, 21, 5, [64], 64),
     wg("wg3 phase (0,0) 64->64", R3, 1, 9, 11, [64], 64, k=2, phase=(0, 0)),
     wg("wg3 phase (1,0) 64->64", R3, 2, 5, 6, [64], 64, k=2, phase=(1, 0)),
     wg("wg3 phase (1,1) 64->64", R3, 1, 9, 11, [64], 64, k=2, phase=(1, 1))]
    + [wg(f"wg3 {c}->32 partial chunk", R3, 1, 33, 19, [c], 32) for c in (8, 16, 24)]
    + [wg(f"wg3 64->32 wgs{w_} nst{n_}", R3, 2, 33, 19, [64], 32, knobs=W3(w_, n_)) for w_, n_ in ((1, 2), (2, 3), (3, 4))]
    # ---- the token core of gemm2.hip, with its fused bias gradient
    + [wg("tok direct 128x64->64", [GEMM2, RED_NONE, False, 1], 1, 128, 1, [64], 64, k=1, bias=True),
       wg("tok direct 128x192->320", [GEMM2, RED_NONE, False, 1], 1, 128, 1, [192], 320, k=1, bias=True),
       wg("tok direct ragged 100x64->64", [GEMM2, RED_NONE, False, 1], 1, 100, 1, [64], 64, k=1, bias=True),
       wg("tok slabs transposing 512x64->64", [GEMM2, RED_TN_TR, True, 2], 1, 512, 1, [64], 64, k=1, bias=True),
       wg("tok slabs ragged 471x64->64", [GEMM2, RED_TN_TR, True, 2], 1, 471, 1, [64], 64, k=1, bias=True),
       wg("tok slabs tree 3152x64->64", [GEMM2, RED_TREE, True, 2], 1, 3152, 1, [64], 64, k=1, bias=True),
       wg("tok element-wise 128x56of64->64", [GEMM2, RED_TN, True, 0], 1, 128, 1, [64], 64, k=1, k_real=56)]
    # ---- the first-generation patch kernel and the tree reducer
    + [wg("patch fp32 3x3 16->16", [PATCH, RED_TREE], 2, 9, 7, [16], 16, dtype=F32),
       wg("patch 2x2s2 32->16 NT1", [PATCH, RED_TREE], 2, 16, 16, [32], 16, k=2, stride=2, nt=1, kernel="igemm_wgrad_kernel<bf16, 1, 2, 2, "),
       wg("patch 2x2s2 32->64 NT4", [PATCH, RED_TREE], 2, 16, 16, [32], 64, k=2, stride=2, nt=4, kernel="igemm_wgrad_kernel<bf16, 4, 2, 2, "),
       wg("patch 1x1 32->64", [PATCH, RED_TREE], 1, 33, 19, [32], 64, k=1),
       wg("patch 3x3 stride 2 32->32", [PATCH, RED_TREE], 2, 17, 13, [32], 32, stride=2)]
)
WG_BY_NAME = {c["name"]: c for c in WG_CASES}
assert len(WG_BY_NAME) == len(WG_CASES)


@functools.lru_cache(maxsize=None)
def make_wgrad(name):
    c = WG_BY_NAME[name]
    s, dt = _seed(c), c["dtype"]
    B, H, W, cs, N, k = c["B"], c["H"], c["W"], c["cs"], c["N"], c["k"]
    K = sum(cs)
    Ho, Wo = out_hw(c)
    t = {}
    if c["phase"] is not None:
        py, px = c["phase"]
        full = ints((B, K, 2 * H, 2 * W), -2, 2, s)                       # the [B, 2H, 2W] tensor whose parity sub-image is the source
        t["xs"] = [stored(nhwc(full), dt)]
        src = F.pad(full[:, :, py::2, px::2], (px, 1 - px, py, 1 - py))
        conv = lambda a, ww: F.conv2d(a, ww)                              # noqa: E731
    else:
        xs = [ints((B, ci, H, W), -2, 2, s + i) for i, ci in enumerate(cs)]
        t["xs"] = [stored(nhwc(x), dt) for x in xs]
        src = torch.cat(xs, 1)
        conv = lambda a, ww: F.conv2d(a, ww, stride=c["stride"], padding=c["pad"])      # noqa: E731
    if c["aff"]:
        sc, sh = pick(SPOW2, (K,), s + 10), ints((K,), -2, 2, s + 11)
        t["scale"], t["shift"] = sc.float(), sh.float()
        src = torch.relu(exact_f32(src * sc.view(1, -1, 1, 1), "x * scale") + sh.view(1, -1, 1, 1))
        assert torch.equal(src.float().to(dt).double(), src)
    kr = K if c["k_real"] is None else c["k_real"]
    dyf = ints((B, c["dyC"], Ho, Wo), -2, 2, s + 20)                      # (the pad channels of a wide d out row hold integers too)
    t["dy"] = stored(nhwc(dyf), dt)
    dy = dyf[:, :N]

    def grad_of(a, g):
        wz = torch.zeros((N, kr, k, k), dtype=F64, requires_grad=True)
        return torch.autograd.grad(conv(a[:, :kr], wz), wz, g)[0]
    dw = grad_of(src, dy)
    t["dw_max"] = below_limit(grad_of(src.abs(), dy.abs()), "|dW|")
    if c["phase"] is not None:
        from kurosiwo_amd.runtime import phase_taps_k4s2
        t["tap_off"] = phase_taps_k4s2(py, px, False)
        shape = (N, kr, 16)
        nanfill = torch.full(shape, NAN, dtype=F64)
        place = lambda g, base: _place_taps(g, nanfill if base is None else base, base is not None, t["tap_off"])      # noqa: E731
    else:
        shape = (N, kr, k * k)
        place = lambda g, base: g.reshape(shape) if base is None else g.reshape(shape) + base      # noqa: E731
    t["shape"] = shape
    t["prior"] = ints(shape, -16, 16, s + 30).float()
    t["grad"] = {0: (place(dw, None) + 0.0).float(),
                 1: exact_f32(place(dw, t["prior"].double()) + 0.0, "dW + prior").float()}
    if c["bias"]:
        db = dy.sum((0, 2, 3))
        below_limit(dy.abs().sum((0, 2, 3)), "bias sums")
        t["bias_prior"] = ints((N,), -16, 16, s + 31).float()
        t["db"] = {0: (db + 0.0).float(), 1: (db + t["bias_prior"].double() + 0.0).float()}
    return t


def _place_taps(g, base, add, tap_off):
    """g [N, K, 2, 2] into the four tap_off entries of base [N, K, 16] (added to them where the call accumulates)"""
    out = base.clone()
    for i, o in enumerate(tap_off):
        out[..., o] = g[..., i // 2, i % 2] + (out[..., o] if add else 0.0)
    return out


def wgrad_desc(c, dev_t, grad, accumulate):
    """the weight-gradient descriptor over tensors on any device -> (descriptor, workspace bytes)"""
    from kurosiwo_amd.runtime import SrcSpec, make_wgrad as mk
    B, H, W, N, k, dt = c["B"], c["H"], c["W"], c["N"], c["k"], c["dtype"]
    K = sum(c["cs"])
    kr = K if c["k_real"] is None else c["k_real"]
    Ho, Wo = out_hw(c)
    srcs = [SrcSpec(x, ci, k_real=(kr if c["k_real"] is not None else None)) for x, ci in zip(dev_t["xs"], c["cs"])]
    if c["aff"]:
        srcs[0].scale, srcs[0].shift, srcs[0].relu = dev_t["scale"], dev_t["shift"], 1
    if c["phase"] is not None:
        py, px = c["phase"]
        d, ws = mk(srcs, dev_t["dy"], c["dyC"], 0, N, grad, 16, kr * 16, 0, accumulate, B, H, W, Ho, Wo, 2, 2, 1, py, dt, pad_x=px,
                   in_map=(2, 2, py, px, 2 * H, 2 * W), tap_off=dev_t["tap_off"])
    else:
        d, ws = mk(srcs, dev_t["dy"], c["dyC"], 0, N, grad, k * k, kr * k * k, 1 if k > 1 else 0, accumulate, B, H, W, Ho, Wo, k, k,
                   c["stride"], c["pad"], dt)
    d._keep = (srcs, dev_t, grad)
    return d, ws


def assert_wgrad_route(c, d):
    from kurosiwo_amd.runtime import wgrad_dispatch_info
    info = wgrad_dispatch_info(d, c["dtype"])
    want = c["route"]
    got = [info[0], info[1]] + ([info[2] > 1, info[3]] if len(want) == 4 else [])
    assert got == want and d.nsplit == info[2], (c["name"], want, info)
    assert c["nt"] is None or info[4] == c["nt"], (c["name"], info)          # (the patch kernel's column fragments per workgroup)
    return info


WG_CORE = {PATCH: "igemm_wgrad_kernel<", GEMM2: "gemm2_tn_kernel<", WGRAD3: "wgrad3_kernel<"}
WG_REDUCER = {RED_WGRAD3: "wgrad3_reduce_kernel", RED_TREE: "wgrad_reduce_kernel", RED_TN_TR: "tn_reduce_tr_kernel", RED_TN: "tn_reduce_kernel"}


# ------------------------------------------------------------------------------------------------------------------------------
# composition: forward -> input gradient -> weight gradient of ONE 3 x 3 layer on one set of tensors, through kurosiwo_amd.functional
# ------------------------------------------------------------------------------------------------------------------------------
# (name, B, H, W, K, N, knobs, forward kernel, input-gradient kernel)
COMPOSE_CASES = [("igemm3", 2, 9, 7, 32, 32, G3(1), "igemm3_kernel<", "igemm3_kernel<"),
                 ("igemm4", 1, 35, 53, 128, 128, G4("4,4", 5), "igemm4_kernel<4, 4, ", "igemm4_kernel<4, 4, "),
                 ("igemm2", 1, 14, 14, 128, 128, {}, "igemm2_fwd_kernel<", "igemm2_fwd_kernel<")]


@functools.lru_cache(maxsize=None)
def make_compose(name):
    _, B, H, W, K, N, _, _, _ = [c for c in COMPOSE_CASES if c[0] == name][0]
    s = 5000 + sum(map(ord, name))
    x = ints((B, K, H, W), -2, 2, s).requires_grad_(True)
    w = ints((N, K, 3, 3), -1, 1, s + 1).requires_grad_(True)
    b, dy = ints((N,), -4, 4, s + 2), ints((B, N, H, W), -2, 2, s + 3)
    y = F.conv2d(x, w, b, padding=1)
    y.backward(dy)
    xa, wa, da = x.detach().abs(), w.detach().abs(), dy.abs()
    below_limit(F.conv2d(xa, wa, b.abs(), padding=1), "forward accumulator")
    below_limit(F.conv_transpose2d(da, wa, padding=1), "input-gradient accumulator")
    wz = torch.zeros_like(wa).requires_grad_(True)
    below_limit(torch.autograd.grad(F.conv2d(xa, wz, padding=1), wz, da)[0], "|dW|")
    return {"x": stored(nhwc(x.detach()), BF16), "w": w.detach().float(), "bias": b.float(), "dy": stored(nhwc(dy), BF16),
            "y": stored(nhwc(y.detach()), BF16), "dx": stored(nhwc(x.grad), BF16), "dw": (w.grad + 0.0).float()}
