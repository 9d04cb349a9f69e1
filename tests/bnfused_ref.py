"""Float64 oracles of the four fused BatchNorm passes of csrc/bnfused.hip and the case tables that tests/test_gpu_bnfused.py and
tests/test_bnfused_ref_cpu.py share.

A fused pass finishes the statistics rows itself and then streams, so its oracle is a composition of the oracles of
tests/elementwise_ref.py (imported, never copied): bn_finalize + bn_add_relu + maxpool_forward for ksmi_bn_fin_add_relu, the column
totals of the rows + bn_bwd_apply / bn_bwd_apply_add + bias_partial for the three backward passes.  What is new here is the data
that keeps the FINISH exact in fp32 as well, so that the whole fused call can be compared bit for bit:

  forward   eps = 1, momentum = 0.25, count = 64 (or 1); per channel an integer mean in [-2, 2] and a variance from {0, 3, 15, 63}:
            var + eps is a power of 4, rstd is exactly 1, 1/2, 1/4 or 1/8, and with gamma in {+-0.5, 1, +-2} and integer beta the
            published mean, rstd, scale, shift and running mean are exact.  The running variance is exact where var is 0 or 63 (the
            unbiased 63 * 64 / 63 = 64) or count = 1, and is held to the bound R.bn_finalize derives elsewhere.
            Channel 0 is the clamp case: q = 0, s != 0, the variance comes out below zero and is clamped to 0.
  backward  integer rows whose column totals are the `sums` of R.make_bn_bwd, so R.bn_bwd_apply / R.bn_bwd_apply_add give the expected
            dz, g and di unchanged.

State of `partial` after a fused call: more than 512 rows are folded in place first (rows 0..31 then hold the sums of rows r, r + 32,
...; the padding columns and the other rows stay), up to 512 rows nothing is written.  The standalone reducers differ: they fold above
256 rows.  Both thresholds assume the default of the KSMI_FOLD_MIN knob, as R.folded does."""
import torch

import elementwise_ref as R

BF16, F32, F64 = R.BF16, R.F32, R.F64
EPS, MOMENTUM, COUNT = 1.0, 0.25, 64.0
VARS = [0.0, 3.0, 15.0, 63.0]
GAMMAS = [-2, -0.5, 0.5, 1, 2]
NBT = 41
FUSED_FOLD_MIN = 512                    # rows a fused workgroup sums itself; longer lists go through the in-place fold
MAX_ROWS = 256                          # ksmi_bn_fused_max_rows(): up to here the fused pass equals the launches it replaces


def dtypes_of(C):
    """bf16 needs C % 8 == 0"""
    return [d for d in R.DTYPES if C % R.vec_of(d) == 0]


def dtype_id(dtype):
    return R.DTYPE_IDS[R.DTYPES.index(dtype)]


# ------------------------------------------------------------------------------------------------------------------------------
# statistics rows
# ------------------------------------------------------------------------------------------------------------------------------
def rows_with_totals(rows, totals, C, Cstride, seed):
    """partial [rows, K, Cstride] fp32: random integer rows, row 0 corrected so that the column totals are `totals` [K, C] (float64
    integers); the padding columns hold R.SENTINEL"""
    K = totals.shape[0]
    body = R.ints((rows, K, C), -64, 64, seed)
    body[0] += totals - body.sum(0)
    partial = torch.full((rows, K, Cstride), R.SENTINEL, dtype=F64)
    partial[:, :, :C] = body
    assert torch.equal(partial[:, :, :C].sum(0), totals)
    return R.exact_f32(partial, "partial").float()


def partial_after(partial, C):
    """`partial` as a FUSED call leaves it: folded above 512 rows (there R.folded applies: 512 > its own threshold of 256), else untouched"""
    return R.folded(partial, C) if partial.shape[0] > FUSED_FOLD_MIN else partial.clone()


def make_fin_stats(rows, C, pad, count=COUNT, seed=20):
    """what ksmi_bn_fin_add_relu reads besides the activations.  Channel 0: the clamp (q = 0 in every row, s != 0); channel 1: mean 0,
    gamma 1, beta -0.0, so shift = -0.0; channel 2: mean 0, gamma -2, beta +0.0, so mean * scale = -0.0 and shift = +0.0"""
    assert C >= 4
    mean, var = R.ints((C,), -2, 2, seed), R.pick(VARS, (C,), seed + 1)
    mean[0] = [-2.0, -1.0, 1.0, 2.0][seed % 4]
    mean[1] = mean[2] = 0.0
    totals = torch.stack([count * mean, count * (var + mean * mean)])
    totals[1, 0] = 0.0
    partial = rows_with_totals(rows, totals, C, C + pad, seed + 2)
    partial[:, 1, 0] = 0.0
    gamma, beta = R.pick(GAMMAS, (C,), seed + 3), R.ints((C,), -2, 2, seed + 4)
    gamma[1], beta[1] = 1.0, -0.0
    gamma[2], beta[2] = -2.0, 0.0
    var[0] = 0.0                                                        # what the clamp leaves
    return {"partial": partial, "Cstride": C + pad, "gamma": gamma.float(), "beta": beta.float(), "rmean": R.ints((C,), -2, 2, seed + 5).float(),
            "rvar": R.pick([0.5, 1, 2, 4], (C,), seed + 6).float(), "nbt": NBT, "mean_want": mean, "var_want": var, "count": count}


def fin_expect(st, C):
    """-> mean, rstd, scale, shift, rmean as fp32 tensors (bit-exact), rvar as (ref, bound, mask of the channels that are bit-exact)"""
    ref = R.bn_finalize(st["partial"], C, st["count"], st["gamma"], st["beta"], st["rmean"], st["rvar"], MOMENTUM, EPS, True)
    want = {k: R.exact_f32(ref[k][0], k).float() for k in ("mean", "rstd", "scale", "shift", "rmean")}
    assert torch.equal(ref["mean"][0], st["mean_want"]) and torch.equal(ref["rstd"][0], 1.0 / torch.sqrt(st["var_want"] + EPS))
    exact = (st["var_want"] == 0) | ((st["var_want"] == 63) & torch.tensor(st["count"] == 64.0)) | torch.tensor(st["count"] == 1.0)
    R.exact_f32(ref["rvar"][0][exact], "running variance")
    want["rvar"] = (ref["rvar"][0], ref["rvar"][1], exact)
    return want


# ------------------------------------------------------------------------------------------------------------------------------
# ksmi_bn_fin_add_relu
# ------------------------------------------------------------------------------------------------------------------------------
def add_relu_real(z, idn, scale, shift):
    """max(z * scale + shift + identity, 0) on any data -> (float64 value, sum of the absolute values of its three terms)"""
    v = z * scale + shift + idn
    return v.clamp_min(0.0) + 0.0, (z * scale).abs() + shift.abs() + idn.abs()


N_ADD_RELU = 3                          # the product, + shift, + identity: three fp32 roundings before the store's


def pool_of(out, B, H, W):
    """out [B * H * W, C] -> [B, H / 2, W / 2, C]: the first-maximum 2x2 pool of R.maxpool_forward"""
    return R.maxpool_forward(out.double().view(B, H, W, -1))[0]


def fin_add_relu(st, C, z, idn, B, H, W, dtype, pooled):
    """the whole forward pass on dyadic data: the finish, then R.bn_add_relu with the exact scale and shift, then the pool of the
    STORED out (what the standalone pool would read) -> the dict of fin_expect + out (+ pooled), in dtype"""
    want = fin_expect(st, C)
    want["out"] = R.bn_add_relu(z, idn, want["scale"].double(), want["shift"].double(), dtype)
    if pooled:
        want["pooled"] = R.stored(pool_of(want["out"], B, H, W), dtype, "pooled")
    return want


def make_fin_add_relu(B, H, W, C, dtype, pooled, rows=5, pad=4, count=COUNT, seed=30):
    """integer z and identity with R.make_bn_add_relu's negative-zero row: pixel 0, channels 0..3 are zeros, the identity -0.0; in channel
    1 z is -0.0 as well, so with scale > 0 and shift = -0.0 the sum before the ReLU is -0.0 (R.bn_add_relu documents the choice of
    max(-0.0, +0.0)); in channel 2 (scale < 0) the product is -0.0 and the sum +0.0"""
    npix = B * H * W
    st = make_fin_stats(rows, C, pad, count, seed)
    z = R.ints((npix, C), -8, 8, seed + 10)
    idn = R.with_negative_zeros(R.ints((npix, C), -8, 8, seed + 11), seed + 12)
    z[0, :4], idn[0, :4] = 0.0, -0.0
    z[0, 1] = -0.0
    d = dict(st)
    d.update(z=R.stored(z, dtype), idn=R.stored(idn, dtype), want=fin_add_relu(st, C, z, idn, B, H, W, dtype, pooled))
    return d


# (B, H, W): one pixel; one row of odd length; two images of several windows.  Only the last is poolable
FIN_SHAPES = [(1, 1, 1), (1, 1, 37), (2, 6, 10)]
FIN_C = [8, 24, 64, 512]
FIN_CASES = [(s, C, p) for s in FIN_SHAPES for C in FIN_C for p in ((0, 1) if s == (2, 6, 10) else (0,))] + [((1, 2, 2), 8, 1)]
# the second grid-stride trip, by shape: more than 2 * 256 * 1024 vectors unpooled, more than 256 * 1024 windows pooled (fp32, C = 8)
FIN_BIG = [((1, 500, 540), 8, 0), ((1, 728, 728), 8, 1)]


# ------------------------------------------------------------------------------------------------------------------------------
# the three backward passes
# ------------------------------------------------------------------------------------------------------------------------------
# (C, rows) of the row-sum cases: 4 / 8 -> 512 / 256 row lanes, a single row, a fold; 24 -> 85 row lanes of 12 threads + 4 idle, rows
# around the lane count; 512 -> 4 row lanes and full LDS tables, rows around the lane count, the launch limit 256, the fold limit 512
ROWSUM_CASES = [(4, 1), (4, 513), (8, 1), (8, 2000), (24, 84), (24, 85), (24, 86), (512, 3), (512, 4), (512, 5), (512, 256), (512, 257),
                (512, 512), (512, 513)]
ROWSUM_SPOT = [(24, 85), (512, 513)]                                    # through each of the other three launchers
# (padding columns, (sums, dgamma, dbeta) given?, accumulate)
ROWSUM_VARIANTS = [(0, (1, 1, 1), 0), (4, (0, 1, 1), 1), (0, (1, 0, 1), 1), (4, (1, 1, 0), 0), (4, (1, 1, 1), 1)]
ROWSUM_NPIX = 7
BWD_MODES = ["gated", "relu"]                                           # ksmi_bn_bwd_fin_apply_gated / ksmi_bnrelu_bwd_fin_apply
BWD_NPIX, BWD_C = R.BWD_NPIX, R.BWD_C
ADD_C = BWD_C + [512]
BIAS_ROWS = [1, 3, 8, 256]
BWD_BIG = (270000, 8)                                                   # fp32: 540000 vectors > 2 * 256 * 1024


def make_bwd(npix, C, dtype, rows, pad, count=R.BWD_COUNT, seed=40, whole=False):
    """R.make_bn_bwd + the rows that total its `sums`, prior dgamma / dbeta, and -0.0 among the zeros of `out`.
    whole: `sums` rounded to multiples of `count`, so that sums / count is an integer"""
    d = R.make_bn_bwd(npix, C, dtype, seed=seed, count=count)
    if whole:
        d["sums"] = (torch.round(d["sums"].double() / count) * count).float()
    out = R.with_negative_zeros(d["out"].double(), seed + 20)
    out[0, 0], out[0, 1] = -0.0, 0.0                                    # (both zeros even in a one-pixel tensor)
    d["out"] = R.stored(out, dtype)
    d["partial"] = rows_with_totals(rows, d["sums"].double(), C, C + pad, seed + 21)
    d["Cstride"] = C + pad
    d["prior_dgamma"], d["prior_dbeta"] = R.ints((C,), -32, 32, seed + 22).float(), R.ints((C,), -32, 32, seed + 23).float()
    return d


def bwd_finish(d, C, accumulate):
    """what workgroup 0 publishes: sums [2, C] = the column totals as floats, dbeta (+)= sums[0], dgamma (+)= sums[1]; and `partial` after"""
    s = R.exact_f32(d["partial"].double()[:, :, :C].sum(0), "row totals")
    assert torch.equal(s, d["sums"].double())

    def into(prior, k):
        return R.exact_f32(prior.double() + s[k] if accumulate else s[k] + 0.0, "parameter gradient").float()
    return {"sums": s.float(), "dgamma": into(d["prior_dgamma"], 1), "dbeta": into(d["prior_dbeta"], 0),
            "partial_after": partial_after(d["partial"], C)}


def case_bwd_fin_apply(mode, npix, C, dtype, rows, pad, seed=40):
    """-> inputs, the gradient as the call leaves it (mode "relu": gated by out > 0 and written over dout; "gated": read only), dz"""
    d = make_bwd(npix, C, dtype, rows, pad, seed=seed)
    g, dz, _ = R.bn_bwd_apply(d, dtype, gate=mode == "relu")
    return d, g, R.stored(dz, dtype, "dz")


def case_bwd_fin_apply_add(npix, C, dtype, rows, pad, bias_rows=BIAS_ROWS, seed=40):
    """-> inputs, di as stored over r, {bias_rows: bias_partial [bias_rows, C]}: the slab sums of the values stored, per = ceil(npix /
    bias_rows) as in the standalone kernel; a workgroup whose slab is empty writes a row of +0.0"""
    # count 16 as in R.case_bwd_apply_add, and sums that are multiples of it: the stored values have quantum 2^-3 (gamma * rstd >= 1 / 4,
    # xhat in halves), so that all 1073 of a channel still sum exactly in ONE slab, whichever of 512 channels is the largest
    d = make_bwd(npix, C, dtype, rows, pad, count=16.0, seed=seed, whole=True)
    di, _ = R.bn_bwd_apply_add(d, 1, dtype)
    st = R.stored(di, dtype, "di")
    return d, st, {b: R.exact_f32(R.bias_partial(st, b)[0], "bias partial").float() for b in bias_rows}


# ------------------------------------------------------------------------------------------------------------------------------
# gaussian data: nothing is dyadic but the two quantities R.bn_finalize needs exact (the mean and the fp64 variance)
# ------------------------------------------------------------------------------------------------------------------------------
REAL_NPIX, REAL_C, REAL_ROWS = R.REAL_NPIX, R.REAL_C, R.REAL_ROWS
REAL_SHAPE = (1, 29, 37)                                                # 1073 pixels: odd in both directions, so not poolable
REAL_POOL_SHAPE = (2, 18, 30)                                           # the nearest poolable size (1080 pixels) for the pooled sequence
REAL_COUNT = 1024.0


def make_real_forward(B, H, W, C, dtype, rows=REAL_ROWS, pad=4, seed=500):
    """gaussian z and identity, and statistics rows of a gaussian sample of 1024 values per channel.  R.bn_finalize asserts that the mean
    is an fp32 number and that the variance is exact in fp64, so the count is a power of two and each row sum is rounded to a multiple
    of 2^-8; with eps = 1e-5 rstd, scale, shift, the running statistics and every output are not dyadic"""
    npix = B * H * W
    sample = R.gauss((int(REAL_COUNT), C), seed, 2.0) + R.gauss((C,), seed + 1, 0.5)
    body = torch.stack([R.slab_sums(sample, rows), R.slab_sums(sample * sample, rows)], 1)
    partial = torch.full((rows, 2, C + pad), R.SENTINEL, dtype=F64)
    partial[:, :, :C] = torch.round(body * 256.0) / 256.0
    return {"partial": R.exact_f32(partial, "partial").float(), "Cstride": C + pad, "count": REAL_COUNT, "gamma": R.gauss((C,), seed + 2).float(),
            "beta": R.gauss((C,), seed + 3).float(), "rmean": R.gauss((C,), seed + 4).float(), "rvar": (R.gauss((C,), seed + 5).abs() + 0.5).float(),
            "nbt": NBT, "z": (R.gauss((npix, C), seed + 6, 2.0) + 0.5).to(dtype), "idn": R.gauss((npix, C), seed + 7, 2.0).to(dtype)}


def make_real_bwd(npix, C, dtype, rows=REAL_ROWS, pad=4, seed=600):
    """R.make_bn_bwd(real=True) + gaussian rows; `sums` becomes their fp64 column total, (row 0 + row 1) + row 2 ..., rounded to fp32 once"""
    d = R.make_bn_bwd(npix, C, dtype, seed=seed, real=True)
    partial = torch.full((rows, 2, C + pad), R.SENTINEL, dtype=F64)
    partial[:, :, :C] = R.gauss((rows, 2, C), seed + 20, (npix / rows) ** 0.5)
    d["partial"], d["Cstride"] = partial.float(), C + pad
    s = torch.zeros((2, C), dtype=F64)
    for r in range(rows):
        s = s + d["partial"].double()[r, :, :C]
    d["sums64"], d["sums_mag"] = s, d["partial"].double()[:, :, :C].abs().sum(0)
    d["sums"] = s.float()
    return d


def real_sums_bound(d):
    """the kernel sums the rows in fp64 and converts once: half an ulp of fp32 (+ 2^-20 of it for a double rounding) + the fp64 chain"""
    rows = d["partial"].shape[0]
    return R.half_ulp(d["sums64"], F32) * (1 + 2.0 ** -20) + rows * 2.0 ** -53 * d["sums_mag"]
