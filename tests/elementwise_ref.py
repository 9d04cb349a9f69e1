"""Float64 oracles of the kernels of csrc/elementwise.hip, one per kernel, and the input builders that tests/test_gpu_elementwise.py
and tests/test_elementwise_ref_cpu.py share.

Every oracle takes what its kernel reads (the stored bf16 / fp32 values upcast to float64 and the fp32 parameter vectors) and
evaluates the kernel's expression in float64.  On the dyadic inputs built here (small integers, powers of two) every intermediate
of the kernel's fp32 evaluation is exactly representable, so the fp32 result IS the float64 one whatever the summation order and
whether or not the compiler contracts a multiply-add: the GPU tests compare bit for bit.  An oracle that claims exactness asserts
its own precondition (exact_f32 / sum_exact below), so a badly chosen input fails here, on the CPU.

Inexact results (gaussian inputs, BatchNorm finalize) come with an elementwise bound instead:
    bound = half an ulp of the output type at |ref|  +  n * 2^-24 * (sum of the absolute values of the terms of the expression)
with n the number of fp32 roundings on the longest path of the kernel, stated next to each use."""
import torch

BF16, F32 = torch.bfloat16, torch.float32
DTYPES = [BF16, F32]
DTYPE_IDS = ["bf16", "fp32"]
F64 = torch.float64
U = 2.0 ** -24                     # unit roundoff of fp32


def vec_of(dtype):
    return 8 if dtype == BF16 else 4


# ------------------------------------------------------------------------------------------------------------------------------
# data and exactness helpers
# ------------------------------------------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(shape, lo, hi, seed):
    """float64 integers in [lo, hi]"""
    return torch.randint(lo, hi + 1, tuple(shape), generator=_gen(seed)).to(F64)


def pick(values, shape, seed):
    v = torch.tensor(values, dtype=F64)
    return v[torch.randint(0, len(values), tuple(shape), generator=_gen(seed))]


def gauss(shape, seed, scale=1.0):
    return torch.randn(tuple(shape), generator=_gen(seed), dtype=F64) * scale


def with_negative_zeros(x, seed):
    """half of the zeros of x become -0.0"""
    m = torch.rand(x.shape, generator=_gen(seed)) < 0.5
    return torch.where(m & (x == 0), torch.tensor(-0.0, dtype=F64), x)


def exact_f32(x, what):
    assert torch.equal(x.float().double(), x), f"{what}: not exactly representable in fp32"
    return x


def quantum(x):
    """the largest power of two that divides every element of x"""
    nz = x[x != 0]
    if nz.numel() == 0:
        return 1.0
    m, e = torch.frexp(nz)
    m53 = (m.abs() * 2.0 ** 53).to(torch.int64)
    low = (m53 & -m53).to(F64) * torch.pow(torch.tensor(2.0, dtype=F64), (e - 53).to(F64))
    return float(low.min())


def sum_exact(terms, dims, what):
    """precondition of an fp32 accumulation: every partial sum, in any order, is a multiple of the data's quantum below 2^24 quanta"""
    exact_f32(terms, what)
    q = quantum(terms)
    top = float(terms.abs().sum(dims).max()) if terms.numel() else 0.0
    assert top < 2.0 ** 24 * q, f"{what}: partial sums up to {top} at quantum {q} are not exact in fp32"


def stored(x, dtype, what="value"):
    """an exact float64 value as the kernel stores it: rounded once, to nearest even"""
    return exact_f32(x, what).float().to(dtype)


def half_ulp(ref, dtype):
    """half an ulp of `dtype` at |ref| (elementwise, float64)"""
    bits = 7 if dtype == BF16 else 23
    _, e = torch.frexp(ref.abs().clamp_min(2.0 ** -126))
    return 0.5 * torch.pow(torch.tensor(2.0, dtype=F64), (e - 1 - bits).to(F64))


def ratio(got, ref, bound):
    """largest error / bound; an error where the bound is zero counts as infinite"""
    err = (got.double() - ref).abs()
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.tensor(float("inf"), dtype=F64), torch.zeros((), dtype=F64)))
    return float(r.max()) if r.numel() else 0.0


def slab_bounds(npix, rows):
    """pixel slab [p0, p1) of each of the `rows` workgroups: per = ceil(npix / rows)"""
    per = (npix + rows - 1) // rows
    r = torch.arange(rows, dtype=torch.int64)
    return torch.clamp(per * r, max=npix), torch.clamp(per * (r + 1), max=npix)


def slab_sums(x, rows):
    """x [npix, C] -> [rows, C]: the sum of each workgroup's slab (float64 prefix sums: exact on dyadic data)"""
    p0, p1 = slab_bounds(x.shape[0], rows)
    cs = torch.cat([torch.zeros(1, x.shape[1], dtype=F64), torch.cumsum(x, 0)])
    return (cs[p1] - cs[p0]) + 0.0                                      # (an accumulator starts at +0.0: a lone -0.0 term sums to +0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# layout helpers
# ------------------------------------------------------------------------------------------------------------------------------
LAYOUT_CASES = [(1, 1, 1), (2, 3, 35), (3, 24, 77)]                    # (B, C, HW)


def nchw_to_nhwc(x, dtype):
    """x [B, C, HW] fp32 -> [B, HW, C] in dtype (one rounding)"""
    return x.permute(0, 2, 1).contiguous().to(dtype)


def nhwc_to_nchw(x):
    """x [B, HW, C] stored -> [B, C, HW] fp32"""
    return x.float().permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# channel_sum / colsum
# ------------------------------------------------------------------------------------------------------------------------------
# (npix, rows): one pixel; odd sizes against 1 / 3 / 8 slabs; more slabs than pixels
CHANNEL_SUM_SHAPES = [(n, r) for n in (1, 37, 1073) for r in (1, 3, 8)] + [(5, 9)]
CHANNEL_SUM_C = [8, 24, 40, 64]
CHANNEL_SUM_WIDE = {BF16: 2056, F32: 1032}                               # C / VEC = 257 / 258 > 128: the wide kernel, ragged last group


def make_channel_sum(npix, rows, C, dtype, seed=1):
    x = ints((npix, C), -8, 8, seed)
    return {"x": stored(x, dtype), "partial": channel_sum(x, rows)}


def channel_sum(x, rows):
    """x [npix, C] -> partial [rows, C] fp32"""
    sum_exact(x, (0,), "channel_sum")
    return slab_sums(x, rows).float()


COLSUM_ROWS = [1, 255, 256, 257, 1023, 1025, 2100]
COLSUM_C = [8, 24, 136]


def make_colsum(rows, C, dtype, accumulate, seed=2):
    x = ints((rows, C), -8, 8, seed)
    prior = ints((C,), -64, 64, seed + 1)
    return {"x": stored(x, dtype), "prior": prior.float(), "out": colsum(x, prior if accumulate else None)}


def colsum(x, prior):
    sum_exact(x, (0,), "colsum")
    s = x.sum(0)
    return exact_f32(s + prior if prior is not None else s, "colsum").float()


# ------------------------------------------------------------------------------------------------------------------------------
# row reducers
# ------------------------------------------------------------------------------------------------------------------------------
REDUCE_ROWS = [1, 63, 64, 65, 256, 257, 1000]                           # 257 and 1000 fold in place first
REDUCE_KC = [(K, C) for K in (1, 2, 3) for C in (3, 16, 40)]
FOLD_MIN, FOLD_R = 256, 32
# (sums, dgamma, dbeta given?, accumulate, alpha)
REDUCE_VARIANTS = [((1, 1, 1), 0, 1.0), ((0, 1, 1), 1, 0.5), ((1, 0, 1), 1, 1.0), ((1, 1, 0), 0, 0.5)]
SENTINEL = 1234.0


def make_reduce_rows(rows, K, C, seed=3):
    Cstride = C + 5
    partial = torch.full((rows, K, Cstride), SENTINEL, dtype=F64)
    partial[:, :, :C] = ints((rows, K, C), -64, 64, seed)
    return {"partial": partial.float(), "Cstride": Cstride, "prior_dgamma": ints((C,), -32, 32, seed + 1).float(),
            "prior_dbeta": ints((C,), -32, 32, seed + 2).float()}


def folded(partial, C):
    """`partial` [rows, K, Cstride] as a reducer leaves it: more than 256 rows (the default of the KSMI_FOLD_MIN knob, which these tests
    assume) are folded in place first, rows 0..31 then hold the sums of rows r, r + 32, ...; the rest and the padding columns stay"""
    p = partial.double()
    after = p.clone()
    if p.shape[0] > FOLD_MIN:
        for r0 in range(FOLD_R):
            after[r0, :, :C] = exact_f32(p[r0::FOLD_R, :, :C].sum(0), "fold")
    return after.float()


def reduce_rows(partial, C, prior_dgamma, prior_dbeta, accumulate, alpha):
    """partial [rows, K, Cstride] -> sums [K, C] (unscaled), dgamma (k = 1; None when K == 1: never written), dbeta (k = 0), and
    `partial` as the call leaves it (more than 256 rows: rows 0..31 hold the fold of rows r, r + 32, ...)"""
    p = partial.double()
    rows, K, _ = p.shape
    s = exact_f32(p[:, :, :C].sum(0), "reduce_rows sums")

    def into(prior, k):
        if k >= K:
            return None
        scaled = exact_f32(alpha * s[k], "alpha * sum")
        return exact_f32(prior.double() + scaled if accumulate else scaled, "reduce_rows target").float()
    return {"sums": s.float(), "dgamma": into(prior_dgamma, 1), "dbeta": into(prior_dbeta, 0), "partial_after": folded(partial, C)}


BATCHED_SINGLE_ROWS = [1, 15, 16, 17, 33, 100]
BATCHED_C = [5, 512, 520]                                               # 520: only through _wide (max_c = 520)


def make_reduce_rows_batched(C, accumulate, seed=4):
    """a descriptor table as a list of dicts (partial [rows, K, Cstride] fp32 or None, k, dst index, head, next) + the prior dst rows:
    six single entries, a three-entry chain with different rows / K / k / Cstride, and a chain through a rows = 0, partial = NULL entry"""
    ents, ndst = [], 0

    def entry(rows, K, k, pad, dst, head, nxt, s):
        part = None
        if rows:
            part = torch.full((rows, K, C + pad), SENTINEL, dtype=F64)
            part[:, :, :C] = ints((rows, K, C), -64, 64, s)
            part = part.float()
        ents.append({"partial": part, "rows": rows, "K": K, "k": k, "Cstride": C + pad, "C": C, "accumulate": accumulate, "dst": dst,
                     "head": head, "next": nxt})
    for i, rows in enumerate(BATCHED_SINGLE_ROWS):
        entry(rows, 1 + i % 3, i % (1 + i % 3), i % 2 * 3, ndst, 1, -1, seed + i)
        ndst += 1
    n = len(ents)                                                        # chain n -> n+1 -> n+2; only the head writes
    entry(40, 2, 1, 0, ndst, 1, n + 1, seed + 10)
    entry(17, 3, 2, 7, ndst + 1, 0, n + 2, seed + 11)                  # (a non-head entry names a row of its own, which must stay as it was)
    entry(1, 1, 0, 1, ndst + 2, 0, -1, seed + 12)
    ndst += 3
    n = len(ents)                                                        # chain through an empty entry (the plan's "no partial here": zeros)
    entry(33, 1, 0, 0, ndst, 1, n + 1, seed + 20)
    entry(0, 2, 1, 0, ndst + 1, 0, n + 2, seed + 21)
    entry(16, 2, 0, 3, ndst + 2, 0, -1, seed + 22)
    ndst += 3
    init = ints((ndst, C), -32, 32, seed + 30).float() if accumulate else torch.full((ndst, C), float("nan"))
    for e in ents:
        if not e["head"]:
            init[e["dst"]] = float("nan")                                # only a head writes: these rows come back as NaN
    return {"entries": ents, "init": init, "dst": reduce_rows_batched(ents, init)}


def reduce_rows_batched(ents, prior):
    """dst [ndst, C] from its state before the call: each head's chain summed in float64, rounded to fp32 once, added to the row when
    the head accumulates; a row that no head names stays as it was"""
    out = prior.double().clone()
    for e in ents:
        if not e["head"]:
            continue
        s, d = torch.zeros(e["C"], dtype=F64), e
        while True:
            if d["rows"]:
                s[:d["C"]] += d["partial"].double()[:, d["k"], :d["C"]].sum(0)
            if d["next"] < 0:
                break
            d = ents[d["next"]]
        exact_f32(s, "batched chain sum")
        out[e["dst"]] = exact_f32(prior[e["dst"]].double() + s if e["accumulate"] else s, "batched dst")
    return out.float()


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm finalize
# ------------------------------------------------------------------------------------------------------------------------------
# (rows, C, count): 300 rows fold; count = 1 takes the biased variance for the running update
FINALIZE_CASES = [(1, 5, 64.0), (70, 16, 4096.0), (300, 33, 16384.0), (1, 16, 1.0)]
MOMENTUM, EPS = 0.1, 1e-5


def make_bn_finalize(rows, C, count, seed=5):
    """integer partial sums with q >= s^2 / count + (a positive integer), except channel 0: q = 0, s != 0 (the clamp var = 0)"""
    Cpad = C + 3
    s = ints((rows, C), -6, 6, seed)
    S = s.sum(0)
    need = torch.ceil(S * S / count) + ints((C,), 1, 9, seed + 1) * count       # total of q per channel: var = need / count - mean^2 > 0
    q = torch.zeros((rows, C), dtype=F64)
    q[:] = torch.floor(need / rows)
    q[0] += need - q.sum(0)
    if S[0] == 0:
        s[0, 0] += 3
    q[:, 0] = 0
    partial = torch.full((rows, 2, Cpad), SENTINEL, dtype=F64)
    partial[:, 0, :C], partial[:, 1, :C] = s, q
    return {"partial": exact_f32(partial, "partial").float(), "Cpad": Cpad, "gamma": pick([-2, -0.5, 0.5, 1, 2], (C,), seed + 2).float(),
            "beta": ints((C,), -2, 2, seed + 3).float(), "rmean": ints((C,), -2, 2, seed + 4).float(),
            "rvar": pick([0.5, 1, 2, 4], (C,), seed + 5).float(), "nbt": 41}


def bn_finalize(partial, C, count, gamma, beta, rmean, rvar, momentum, eps, training):
    """-> {name: (ref, bound)} for mean, rstd, scale, shift, rmean, rvar (float64); bound None = bit-exact.
    momentum and eps are the fp32 values the kernel receives."""
    g, b, rm, rv = gamma.double(), beta.double(), rmean.double(), rvar.double()
    m, e = float(torch.tensor(momentum, dtype=F32)), float(torch.tensor(eps, dtype=F32))
    fp64_slack = 8 * 2.0 ** -53                                         # the handful of fp64 operations before the one conversion
    if not training:
        rs = 1.0 / torch.sqrt(rv + e)
        sc = g * rs
        # rstd: n = 2 (rvar + eps, sqrtf) before the division, which is the output rounding; scale: + the division = 3;
        # shift = beta - rmean * sc: 3 + the product = 4 on the longest path
        return {"mean": (rm, None), "rstd": (rs, half_ulp(rs, F32) + 2 * U * rs), "scale": (sc, half_ulp(sc, F32) + 3 * U * sc.abs()),
                "shift": (b - rm * sc, half_ulp(b - rm * sc, F32) + 4 * U * (b.abs() + (rm * sc).abs())),
                "rmean": (rm, None), "rvar": (rv, None)}
    p = partial.double()
    s, q = p[:, 0, :C].sum(0), p[:, 1, :C].sum(0)
    mean = exact_f32(s / count, "mean")
    var = q / count - mean * mean
    assert torch.equal(var, (q * count - s * s) / (count * count)), "variance not exact in fp64"
    var = var.clamp_min(0.0)
    rs = 1.0 / torch.sqrt(var + e)
    sc = g * rs
    unb = var * count / (count - 1.0) if count > 1.0 else var
    sh = b - mean * sc
    nrm, nrv = (1.0 - m) * rm + m * mean, (1.0 - m) * rv + m * unb
    return {
        "mean": (mean, None),
        # rstd: fp64 throughout, one conversion: n = 0
        "rstd": (rs, half_ulp(rs, F32) * (1 + 2.0 ** -20) + fp64_slack * rs),
        # scale = gamma * rs: n = 1 (the conversion of rs) before the product
        "scale": (sc, half_ulp(sc, F32) + 1 * U * sc.abs()),
        # shift = beta - (float)mean * sc: conversion of rs, product sc, product mean * sc: n = 3 before the subtraction
        "shift": (sh, half_ulp(sh, F32) + 3 * U * (b.abs() + (mean * sc).abs())),
        # running = (1 - m) * old + m * new: 1 - m and its product / the conversion of `unb` and its product: n = 2 before the sum
        "rmean": (nrm, half_ulp(nrm, F32) + 2 * U * (((1.0 - m) * rm).abs() + (m * mean).abs())),
        "rvar": (nrv, half_ulp(nrv, F32) + 2 * U * (((1.0 - m) * rv).abs() + (m * unb).abs())),
    }


# ------------------------------------------------------------------------------------------------------------------------------
# bn_add_relu
# ------------------------------------------------------------------------------------------------------------------------------
ADD_RELU_CASES = [(n, C) for n in (1, 37) for C in (8, 24, 64)]


def make_bn_add_relu(npix, C, dtype, seed=6):
    z, idn = ints((npix, C), -8, 8, seed), with_negative_zeros(ints((npix, C), -8, 8, seed + 1), seed + 2)
    scale, shift = pick([-2, -0.5, 0.5, 1, 2], (C,), seed + 3), ints((C,), -4, 4, seed + 4)
    shift[1] = -0.0
    z[0, :4], idn[0, :4] = 0.0, -0.0        # -0.0 before the ReLU where scale < 0 (channel 1: also with shift = -0.0), +0.0 elsewhere
    scale[1], scale[2] = -2.0, 1.0
    return {"z": stored(z, dtype), "idn": stored(idn, dtype), "scale": scale.float(), "shift": shift.float(),
            "out": bn_add_relu(z, idn, scale, shift, dtype)}


def bn_add_relu(z, idn, scale, shift, dtype):
    """max(z * scale + shift + identity, 0); a sum of -0.0 or less gives +0.0.
    For a sum of exactly -0.0 that is a choice, not arithmetic: IEEE maxNum leaves max(-0.0, +0.0) open, and fmaxf(-0.0, 0.f) may
    return either zero.  The oracle takes what gfx950's v_max_f32 does (it orders -0 below +0).  A failure of test_bn_add_relu that
    shows only -0.0 where +0.0 is expected therefore means the compiler lowered the maximum differently, not that a value is wrong:
    every reader of `out` gates on out > 0, for which the two zeros are the same."""
    prod = exact_f32(z * scale, "z * scale")
    v = exact_f32(exact_f32(prod + shift, "+ shift") + idn, "+ identity")
    return stored(torch.where(v > 0, v, torch.zeros((), dtype=F64)), dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU backward
# ------------------------------------------------------------------------------------------------------------------------------
BWD_NPIX = [1, 7, 1073]
BWD_ROWS = [1, 3, 8, 2000]
BWD_C = [8, 24, 64]
BWD_COUNT = 64.0
REAL_NPIX, REAL_C, REAL_ROWS = 1073, 24, 3


def make_bn_bwd(npix, C, dtype, seed=7, real=False, count=BWD_COUNT):
    """what the backward kernels read: dout, out, z, r (activations in dtype) and mean, rstd, gamma, sums [2, C] (fp32)"""
    if real:
        act = {k: gauss((npix, C), seed + i, 2.0).to(dtype) for i, k in enumerate(("dout", "out", "z", "r"))}
        par = {"mean": gauss((C,), seed + 4, 0.5), "rstd": gauss((C,), seed + 5).abs() + 0.5, "gamma": gauss((C,), seed + 6),
               "sums": gauss((2, C), seed + 7, npix ** 0.5)}
        count = float(npix)
    else:
        act = {k: stored(ints((npix, C), -8, 8, seed + i), dtype) for i, k in enumerate(("dout", "out", "z", "r"))}
        par = {"mean": ints((C,), -2, 2, seed + 4), "rstd": pick([0.5, 1, 2], (C,), seed + 5),
               "gamma": pick([-2, -0.5, 0.5, 1, 2], (C,), seed + 6), "sums": ints((2, C), -64, 64, seed + 7)}
    d = dict(act)
    d.update({k: v.float() for k, v in par.items()})
    d["count"] = count
    return d


def reduce_chain(npix, rows, C, dtype):
    """the longest fp32 accumulation chain of a ChanWalk reduction: a lane's pixels, then the block's pixel lanes"""
    cv = C // vec_of(dtype)
    npl = max(1, 256 // cv)
    per = (npix + rows - 1) // rows
    return (per + npl - 1) // npl + npl


def bnrelu_bwd_reduce(d, rows, exact=True):
    """-> partial [rows, 2, C] float64 and the slab sums of |terms|: [.,0] = sum g, [.,1] = sum g * (z - mean) * rstd, g = dout * (out > 0)"""
    dout, out, z = d["dout"].double(), d["out"].double(), d["z"].double()
    mean, rstd = d["mean"].double(), d["rstd"].double()
    g = torch.where(out > 0, dout, torch.zeros((), dtype=F64))
    diff = z - mean
    t1 = g * diff
    term = t1 * rstd
    if exact:
        exact_f32(diff, "z - mean"), exact_f32(t1, "g * (z - mean)")
        sum_exact(g, (0,), "sum g"), sum_exact(term, (0,), "sum g * zhat")
    p = torch.stack([slab_sums(g, rows), slab_sums(term, rows)], 1)
    mag = torch.stack([slab_sums(g.abs(), rows), slab_sums(term.abs(), rows)], 1)
    return p, mag


def bn_bwd_apply(d, dtype, alpha=1.0, gate=True, exact=True, sums=None):
    """-> g (the gated gradient, stored), dz (float64), sum of |terms| of dz = alpha * gamma * rstd * (g - s0 / n - zhat * s1 / n)"""
    dout, out, z = d["dout"].double(), d["out"].double(), d["z"].double()
    mean, rstd, gamma = d["mean"].double(), d["rstd"].double(), d["gamma"].double()
    sums = (d["sums"] if sums is None else sums).double()
    inv_n = 1.0 / d["count"]
    g = torch.where(out > 0, dout, torch.zeros((), dtype=F64)) if gate else dout
    zh = (z - mean) * rstd
    a = sums[0] * inv_n
    b1 = zh * sums[1]
    b = b1 * inv_n
    inner = (g - a) - b
    ag = alpha * gamma
    pre = ag * rstd
    dz = pre * inner
    if exact:
        for name, v in (("1 / count", torch.tensor(inv_n, dtype=F64)), ("z - mean", z - mean), ("zhat", zh), ("s0 / n", a), ("zhat * s1", b1),
                        ("zhat * s1 / n", b), ("g - s0 / n", g - a), ("inner", inner), ("alpha * gamma", ag), ("prefactor", pre), ("dz", dz)):
            exact_f32(v, "bn_bwd_apply " + name)
    return g.to(dtype), dz, pre.abs() * (g.abs() + a.abs() + b.abs())


# The last operation is a product, so the roundings of both its factors count.  Bracket: 1 / count, z - mean, * rstd, * s1, * 1 / n, the
# subtraction = 6; prefactor: alpha * gamma, * rstd = 2, or 1 where alpha * gamma is exact (alpha = 1) or absent (the pre-gated kernel).
N_APPLY = {"scaled": 8, "apply": 7, "gated": 7}


def bn_bwd_apply_add(d, rows, dtype, exact=True):
    """di = g + gamma * rstd * (r - s0 / n - xhat * s1 / n) with xhat from `z` (the block's input); -> di (float64), sum of |terms|"""
    r, g, iv = d["r"].double(), d["dout"].double(), d["z"].double()
    mean, rstd, gamma, sums = d["mean"].double(), d["rstd"].double(), d["gamma"].double(), d["sums"].double()
    inv_n = 1.0 / d["count"]
    gr = gamma * rstd
    k0, k1 = sums[0] * inv_n, sums[1] * inv_n
    xh = (iv - mean) * rstd
    t = xh * k1
    inner = (r - k0) - t
    w = gr * inner
    di = g + w
    if exact:
        for name, v in (("gamma * rstd", gr), ("s0 / n", k0), ("s1 / n", k1), ("i - mean", iv - mean), ("xhat", xh), ("xhat * k1", t),
                        ("r - k0", r - k0), ("inner", inner), ("gr * inner", w), ("di", di)):
            exact_f32(v, "bn_bwd_apply_add " + name)
    return di, g.abs() + gr.abs() * (r.abs() + k0.abs() + t.abs())


# apply_add: the last operation is g (exact) + gr * inner.  inner: 1 / count, s1 / n, i - mean, * rstd, * k1, the subtraction = 6; gamma * rstd
# = 1; their product = 1: n = 8 before the last sum
N_APPLY_ADD = 8


def bias_partial(stored_di, rows, exact=True):
    """partial [rows, C] of bn_bwd_apply_add: the slab sums of the values it STORED -> (sums, sums of |values|), float64"""
    v = stored_di.double()
    if exact:
        sum_exact(v, (0,), "bias partial")
    return slab_sums(v, rows), slab_sums(v.abs(), rows)


# ------------------------------------------------------------------------------------------------------------------------------
# 2x2 max-pool
# ------------------------------------------------------------------------------------------------------------------------------
POOL_CASES = [(1, 2, 2, 8), (2, 6, 10, 24), (1, 4, 2, 64)]


def make_maxpool(B, H, W, C, dtype, seed=8, ties=True):
    if ties:
        x = with_negative_zeros(ints((B, H, W, C), -2, 2, seed), seed + 1)
    else:
        x = torch.randperm(B * H * W * C, generator=_gen(seed)).to(F64).sub(B * H * W * C // 2).view(B, H, W, C)
    dy = with_negative_zeros(ints((B, H // 2, W // 2, C), -8, 8, seed + 2), seed + 3)
    prior = ints((B, H, W, C), -8, 8, seed + 4)
    return {"x": x.float().to(dtype) if ties else x, "dy": stored(dy, dtype), "prior": stored(prior, dtype)}


def _taps(t):
    """the four window taps in the kernel's scan order (0,0), (0,1), (1,0), (1,1)"""
    return [t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]]


def maxpool_forward(x):
    """x [B, H, W, C] float64 -> (y, argmax tap): the first maximum wins (a later tap replaces the maximum only if it is greater)"""
    taps = _taps(x)
    m, am = taps[0].clone(), torch.zeros(taps[0].shape, dtype=torch.int64)
    for k in range(1, 4):
        up = taps[k] > m
        m, am = torch.where(up, taps[k], m), torch.where(up, torch.tensor(k), am)
    return m, am


def maxpool_backward(x, dy, prior=None):
    """the gradient goes to the argmax tap only; every other tap gets +0.0 (or keeps its prior value + 0.0)"""
    _, am = maxpool_forward(x)
    dx = torch.zeros_like(x)
    for k, view in enumerate(_taps(dx)):
        view.copy_(torch.where(am == k, dy, torch.zeros((), dtype=F64)))
    return dx if prior is None else exact_f32(prior + dx, "pool accumulate")


# ------------------------------------------------------------------------------------------------------------------------------
# first-layer conv, im2col, weight gradient
# ------------------------------------------------------------------------------------------------------------------------------
# (B, Cin, H, W, Cout); Cout = 20 only in fp32 (a pass of 4 channels)
CONV_FIRST_CASES = [(1, 1, 1, 1, 8), (2, 3, 20, 35, 24), (1, 8, 16, 16, 32), (2, 2, 17, 16, 40)]
CONV_FIRST_F32_ONLY = (2, 3, 20, 35, 20)
IMAGES = [c[:4] for c in CONV_FIRST_CASES]
WGRAD_CASES = [img + (co,) for img in IMAGES for co in (8, 32)] + [(9, 2, 128, 128, 8)]     # the last: 576 patches > 512 workgroups


def make_conv_first(B, Cin, H, W, Cout, dtype, seed=9, big=False):
    x = ints((B, Cin, H, W), -8, 8, seed) if big else ints((B, Cin, H, W), -2, 2, seed)
    w = ints((Cout, Cin, 3, 3), -4, 4, seed + 1) if big else ints((Cout, Cin, 3, 3), -1, 1, seed + 1)
    bias = ints((Cout,), -2, 2, seed + 2)
    return {"x": x.float(), "w": w.float(), "bias": bias.float()}


def _padded(x):
    return torch.nn.functional.pad(x, (1, 1, 1, 1))


def conv_first(x, w, bias):
    """x [B, Cin, H, W], w [Cout, Cin, 3, 3], bias [Cout] (float64) -> out [B, H, W, Cout] float64, before the store"""
    B, Cin, H, W = x.shape
    xp = _padded(x)
    out = bias.view(1, 1, 1, -1).expand(B, H, W, -1).clone()
    mag = out.abs()
    for t in range(9):
        win = xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W]
        out += torch.einsum("bchw,nc->bhwn", win, w[:, :, t // 3, t % 3])
        mag += torch.einsum("bchw,nc->bhwn", win.abs(), w[:, :, t // 3, t % 3].abs())
    assert float(mag.max()) < 2.0 ** 24, "conv_first: the tap chain is not exact in fp32"
    return out


def conv_first_stats(out_stored, exact=True):
    """stats [tiles, 2, Cout] of the STORED outputs [B, H, W, Cout], tile rows in (b, ty, tx) order -> (sums, sums of |terms|)"""
    v = out_stored.double()
    B, H, W, _ = v.shape
    rows, mags = [], []
    for b in range(B):
        for ty in range((H + 15) // 16):
            for tx in range((W + 15) // 16):
                t = v[b, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16]
                rows.append(torch.stack([t.sum((0, 1)), (t * t).sum((0, 1))]))
                mags.append(torch.stack([t.abs().sum((0, 1)), (t * t).sum((0, 1))]))
                if exact:
                    sum_exact(t, (0, 1), "conv_first tile sum"), sum_exact(t * t, (0, 1), "conv_first tile squares")
    return torch.stack(rows), torch.stack(mags)


# squares row of the rounding case: v * v is exact (8-bit significands); 16 adds down a column of the tile, 16 across the groups
N_STATS_SQ = 32


def im2col3x3(x, Kpad):
    """x [B, Cin, H, W] -> [B, H, W, Kpad]: column c * 9 + t holds x[b, c, y + t / 3 - 1, x + t % 3 - 1] (zero outside), the rest zero"""
    B, Cin, H, W = x.shape
    xp = _padded(x)
    cols = torch.stack([xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W] for t in range(9)], 2)          # [B, Cin, 9, H, W]
    out = torch.zeros(B, H, W, Kpad, dtype=F64)
    out[..., :Cin * 9] = cols.permute(0, 3, 4, 1, 2).reshape(B, H, W, Cin * 9)
    return out


def conv_first_wgrad(x, dy, prior=None, exact=True):
    """x [B, Cin, H, W], dy [B, H, W, Cout] (float64) -> dw [Cout, Cin, 3, 3] (+ prior)"""
    B, Cin, H, W = x.shape
    xp = _padded(x)
    dw = torch.zeros(dy.shape[-1], Cin, 3, 3, dtype=F64)
    mag = torch.zeros_like(dw)
    for t in range(9):
        win = xp[:, :, t // 3:t // 3 + H, t % 3:t % 3 + W]
        dw[:, :, t // 3, t % 3] = torch.einsum("bhwn,bchw->nc", dy, win)
        mag[:, :, t // 3, t % 3] = torch.einsum("bhwn,bchw->nc", dy.abs(), win.abs())
    if not exact:
        return dw if prior is None else dw + prior
    assert float(mag.max()) < 2.0 ** 24 and quantum(x) >= 1 and quantum(dy) >= 1, "conv_first_wgrad: sums are not exact in fp32"
    return exact_f32(dw + 0.0 if prior is None else dw + prior, "wgrad")        # (the accumulators start at +0.0)


def make_wgrad(B, Cin, H, W, Cout, dtype, seed=10):
    x, dy = ints((B, Cin, H, W), -2, 2, seed), ints((B, H, W, Cout), -4, 4, seed + 1)
    return {"x": x.float(), "dy": stored(dy, dtype), "prior": ints((Cout, Cin, 3, 3), -16, 16, seed + 2).float()}


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_elementwise.py: inputs and expected outputs (tests/test_elementwise_ref_cpu.py builds every one of
# them, so the exactness preconditions are checked without a GPU)
# ------------------------------------------------------------------------------------------------------------------------------
def case_layout(B, C, HW, dtype):
    x = gauss((B, C, HW), 11).float()
    y = nchw_to_nhwc(x, dtype)
    return {"x": x, "nhwc": y, "back": nhwc_to_nchw(y)}


def case_bwd_reduce(npix, rows, C, dtype):
    d = make_bn_bwd(npix, C, dtype)
    p, _ = bnrelu_bwd_reduce(d, rows)
    return d, exact_f32(p, "partial").float()


BWD_APPLY_KINDS = ["apply", "scaled", "gated"]


def case_bwd_apply(kind, npix, C, dtype):
    d = make_bn_bwd(npix, C, dtype)
    g, dz, _ = bn_bwd_apply(d, dtype, alpha=0.5 if kind == "scaled" else 1.0, gate=kind != "gated")
    return d, g, stored(dz, dtype, "dz")


def case_bwd_apply_add(npix, rows, C, dtype):
    d = make_bn_bwd(npix, C, dtype, count=16.0)                         # (quantum 2^-7: a slab's 1073 stored values still sum exactly)
    di, _ = bn_bwd_apply_add(d, rows, dtype)
    st = stored(di, dtype, "di")
    p, _ = bias_partial(st, rows)
    return d, st, exact_f32(p, "bias partial").float()


CHAIN_NPIX, CHAIN_C, CHAIN_ROWS = 1024, 32, 8


def case_chain(dtype):
    """bnrelu_bwd_reduce -> reduce_rows -> bnrelu_bwd_apply with count = npix: each stage's exact output feeds the next"""
    d = make_bn_bwd(CHAIN_NPIX, CHAIN_C, dtype, seed=70, count=float(CHAIN_NPIX))
    p, _ = bnrelu_bwd_reduce(d, CHAIN_ROWS)
    sums = exact_f32(p.sum(0), "chain sums")
    g, dz, _ = bn_bwd_apply(d, dtype, sums=sums)
    return d, exact_f32(p, "partial").float(), sums.float(), g, stored(dz, dtype, "dz")


def case_maxpool(B, H, W, C, dtype, accumulate):
    d = make_maxpool(B, H, W, C, dtype)
    x, dy, prior = d["x"].double(), d["dy"].double(), d["prior"].double()
    y, _ = maxpool_forward(x)
    d["y"] = stored(y, dtype)
    d["dx"] = stored(maxpool_backward(x, dy, prior if accumulate else None), dtype)
    return d


def case_conv_first(case, dtype, big=False):
    d = make_conv_first(*case, dtype, big=big)
    out = conv_first(d["x"].double(), d["w"].double(), d["bias"].double())
    assert big == bool(float(out.abs().max()) > 256), "the plain cases store exactly, the rounding case rounds"
    d["out"] = stored(out, dtype, "conv_first")
    d["stats"], d["stats_mag"] = conv_first_stats(d["out"], exact=not big)
    if big:
        sum_exact(d["out"].double(), (0, 1, 2), "conv_first sum row")
    return d


def case_im2col(image, extra, dtype):
    B, Cin, H, W = image
    v = vec_of(dtype)
    Kpad = (Cin * 9 + v - 1) // v * v + extra * 2 * v
    x = ints(image, -2, 2, 12)
    return {"x": x.float(), "Kpad": Kpad, "out": stored(im2col3x3(x, Kpad), dtype)}


def case_wgrad(case, dtype, accumulate):
    d = make_wgrad(*case, dtype)
    d["dw"] = conv_first_wgrad(d["x"].double(), d["dy"].double(), d["prior"].double() if accumulate else None).float()
    return d
