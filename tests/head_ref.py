"""Float64 oracles of the six entry points of csrc/head.hip (the ECAM head of SNUNet), one per entry point, the float64 chain of the
whole head that they are checked against, and the input builders that tests/test_gpu_head.py and tests/test_head_ref_cpu.py share.

As in tests/elementwise_ref.py every oracle evaluates the expression include/ksmi.h documents, in float64, on the values the kernel
reads.  The inputs are dyadic (small integers, multiples of 1/8, powers of two), so every intermediate of the kernel's fp32 evaluation
is exactly representable and the result does not depend on the summation order, on the number of pixel splits or on whether the
compiler contracts a multiply-add: the GPU tests compare bit for bit.  An oracle that claims exactness asserts its own precondition
(exact_f32 / sum_exact of elementwise_ref, dot_exact here).  The two results that are not dyadic come with the bound of elementwise_ref,
    bound = half an ulp of the output type at |ref|  +  n * 2^-24 * (sum of the absolute values of the terms)
with n stated next to its use: the sigmoid of the MLP (N_SIGMOID) and dx where 1 / HW is not a power of two (N_DX)."""
import functools

import torch

from elementwise_ref import (BF16, DTYPE_IDS, DTYPES, F32, F64, U, exact_f32, gauss, half_ulp, ints, pick, quantum, ratio, stored,  # noqa: F401
                             sum_exact, vec_of)

NCLS = 3
POOL_SPLIT = 16                     # default of the KSMI_ECAM_POOL_SPLIT knob, which the tie coverage below assumes (the oracles do not)
THREADS = 256


def dtype_id(dtype):
    return DTYPE_IDS[DTYPES.index(dtype)]


# ------------------------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------------------------
def dot_exact(eq, a, b, what, plus=None):
    """einsum(eq, a, b) (+ plus): the precondition of an fp32 multiply-accumulate chain in any order, fused or not: every product and
    every partial sum is a multiple of the products' quantum below 2^24 quanta"""
    exact_f32(a, what), exact_f32(b, what)
    q = quantum(a) * quantum(b)
    top = torch.einsum(eq, a.abs(), b.abs())
    out = torch.einsum(eq, a, b)
    if plus is not None:
        exact_f32(plus, what)
        q = min(q, quantum(plus))
        top = top + plus.abs()
        out = out + plus
    assert float(top.max()) < 2.0 ** 24 * q, f"{what}: partial sums up to {float(top.max())} at quantum {q} are not exact in fp32"
    return exact_f32(out, what) + 0.0                                    # (an accumulator starts at +0.0: a sum of -0.0 products is +0.0)


def _dot(eq, a, b, what, exact, plus=None):
    if exact:
        return dot_exact(eq, a, b, what, plus)
    out = torch.einsum(eq, a, b)
    return out if plus is None else out + plus


def _store(x, dtype, exact, what):
    """x as a kernel stores it in `dtype` and reads it back (float64); F64: the unrounded chain"""
    if dtype == F64:
        return x
    return (stored(x, dtype, what) if exact else x.float().to(dtype)).double()


def _ex(x, what, exact):
    return exact_f32(x, what) if exact else x


def is_pow2(n):
    return n & (n - 1) == 0


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_head.py
# ------------------------------------------------------------------------------------------------------------------------------
# every C that ecam_c_ok admits and that reaches another path: the pool's register reduction (C <= 128) and its LDS fallback, the
# backward's (4C / VEC <= 32) and its fallback, in both dtypes, and every (pixel lane, channel vector) thread map between
HEAD_C = {F32: [16, 32, 64, 256], BF16: [16, 64, 128, 512]}
# fewer pixels than splits (16 / 64), a ragged last split, splits that own no pixel (65: 13 of 16 and 33 of 64 used), exact multiples
HEAD_HW = [1, 5, 16, 63, 64, 65, 1000, 1024]
# (C, dtype, B, HW): every (C, dtype) meets every HW once; B alternates between 1 and 3
CASES = [(Cc, dt, 3 if (i + j) % 2 else 1, HW) for dt in DTYPES for i, Cc in enumerate(HEAD_C[dt]) for j, HW in enumerate(HEAD_HW)]
GRID_STRIDE_CASE = (16, F32, 1, 65536 + 257)        # final_forward: 256 workgroups x 256 threads walk 65536 pixels per trip
MLP_CASES = [(Cc, B) for Cc in (16, 32, 48, 64, 128, 256, 512) for B in (1, 3)]      # the MLP kernels take any multiple of 16
CHAIN_CASE = (32, 2, 1000)                           # (C, B, HW)


def case_id(c):
    return f"{dtype_id(c[1])}-C{c[0]}-B{c[2]}-HW{c[3]}"


def make_x(B, HW, Cc, dtype, lo, hi, seed):
    """the four sources x0_1..x0_4 [B, HW, C]: integers, exact in `dtype` -> (float64 list, stored list)"""
    xs = [ints((B, HW, Cc), lo, hi, seed + s) for s in range(4)]
    return xs, [stored(x, dtype, "x") for x in xs]


def eighths(shape, seed):
    """channel attention values as inputs: multiples of 1/8 in [0, 1]"""
    return ints(shape, 0, 8, seed) / 8.0


# ------------------------------------------------------------------------------------------------------------------------------
# pool
# ------------------------------------------------------------------------------------------------------------------------------
def pool(xs, dtype, exact=True):
    """xs: four [B, HW, C] float64 -> avg, mx [B, 5C] float64, argmax [B, 5C] int32 (the lowest pixel index that attains the maximum),
    all5 [B, HW, 5C] (the concatenation, then intra = ((x1 + x2) + x3) + x4 rounded once to the activation dtype)"""
    t = _ex(xs[0] + xs[1], "x1 + x2", exact)
    t = _ex(t + xs[2], "+ x3", exact)
    t = _ex(t + xs[3], "+ x4", exact)
    intra = _store(t, dtype, False, "intra")                            # (a rounding, not a claim: bf16 sums above 256 do round)
    all5 = torch.cat(list(xs) + [intra], -1)
    if exact:
        sum_exact(all5, (1,), "pool sums")
    HW = all5.shape[1]
    avg = all5.sum(1) / HW                                              # the kernel: fp64 sum of exact fp32 partial sums, / HW in fp64
    mx = all5.max(1).values
    pix = torch.arange(HW).view(1, HW, 1)
    am = torch.where(all5 == mx.unsqueeze(1), pix, torch.tensor(HW)).min(1).values
    assert int(am.max()) < HW
    return {"avg": avg, "mx": mx, "argmax": am.to(torch.int32), "all5": all5, "intra_unrounded": t}


def pool_thread_map(HW, Cc, dtype):
    """pixel -> (split, pixel lane, wave) of ecam_pool_kernel at the default split count; the wave does not depend on the channel
    vector, because C / VEC divides 64"""
    cv = Cc // vec_of(dtype)
    npl = THREADS // cv
    per = (HW + POOL_SPLIT - 1) // POOL_SPLIT
    p = torch.arange(HW)
    sp = p // per
    pl = (p - sp * per) % npl
    return sp, pl, (pl * cv) // 64


RELATIONS = ["thread", "lanes", "lower_lane", "waves", "splits"]


@functools.lru_cache(maxsize=4)
def pair_relations(HW, Cc, dtype):
    """[HW, HW] int8: how the pool meets a tie between pixels p < q (row p, column q); -1 below and on the diagonal.
    0 both in one thread; 1 two lanes of a wave, the later pixel in the higher lane; 2 the later pixel in the LOWER lane; 3 two waves of
    a workgroup; 4 two splits"""
    sp, pl, wave = pool_thread_map(HW, Cc, dtype)
    same_sp = sp[:, None] == sp[None, :]
    same_w = wave[:, None] == wave[None, :]
    r = torch.full((HW, HW), 4, dtype=torch.int8)
    r[same_sp & ~same_w] = 3
    r[same_sp & same_w & (pl[None, :] > pl[:, None])] = 1
    r[same_sp & same_w & (pl[None, :] < pl[:, None])] = 2
    r[same_sp & (pl[None, :] == pl[:, None])] = 0
    r[torch.tril(torch.ones(HW, HW, dtype=torch.bool))] = -1
    return r


def tie_coverage(all5, Cc, dtype):
    """number of tied pairs of maxima per relation, over every channel of all5 [B, HW, 5C]"""
    B, HW, C5 = all5.shape
    rel = pair_relations(HW, Cc, dtype)
    top = (all5 == all5.max(1, keepdim=True).values).permute(0, 2, 1).reshape(B * C5, HW)
    counts = [0] * len(RELATIONS)
    for row in top[top.sum(1) > 1]:
        p = row.nonzero().flatten()
        for v in rel[p][:, p].flatten().tolist():
            if v >= 0:
                counts[v] += 1
    return dict(zip(RELATIONS, counts))


def feasible_relations(HW, Cc, dtype):
    rel = pair_relations(HW, Cc, dtype)
    return [name for i, name in enumerate(RELATIONS) if bool((rel == i).any())]


def make_pool_rounding(B, HW, Cc, dtype, seed=21):
    """random integers; bf16: up to 256 in size, so that intra (sums up to 1024) is rounded to bf16, which the builder asserts: a
    kernel that pools the unrounded fp32 sum would otherwise pass"""
    r = 256 if dtype == BF16 else 1000
    xs, st = make_x(B, HW, Cc, dtype, -r, r, seed)
    ref = pool(xs, dtype)
    if dtype == BF16:
        assert bool((ref["all5"][..., 4 * Cc:] != ref["intra_unrounded"]).any()), "the bf16 rounding of intra changes no value"
        assert not torch.equal(pool_unrounded(xs)["avg"].float(), ref["avg"].float()), "the rounding of intra does not show in avg"
    return st, ref


def pool_unrounded(xs):
    """what a kernel that skips the conversion of intra would compute"""
    return pool(xs, F64, exact=False)


def make_pool_ties(B, HW, Cc, dtype, seed=22):
    """every one of the 5C channels of every sample has its top value at 1, 2 or 3 pixels drawn from [0, HW) and strictly lower values
    elsewhere.  Source s of channel cc holds its top value T at its own pixels P_s and at the pixels P_4 drawn for intra; so intra
    attains its top, 4 T, on P_4 (and wherever all four P_s meet), and a source's first maximum and intra's are the same pixel in
    some channels and different pixels in others.  The first channels take their pairs from each relation that the thread map of
    (C, dtype, HW) allows (pair_relations), so that each of them occurs whatever the seed; the builder asserts that."""
    g = torch.Generator().manual_seed(seed * 1000003 + HW * 131 + Cc)
    base, T = (60, 100) if dtype == BF16 else (8, 16)                   # bf16: 4 T = 400 > 256, where bf16 keeps even integers only
    xs = [ints((B, HW, Cc), -base, base, seed + 10 + s) for s in range(4)]
    rel = pair_relations(HW, Cc, dtype)
    feas = feasible_relations(HW, Cc, dtype)
    pairs = {name: (rel == RELATIONS.index(name)).nonzero() for name in feas}
    n = 0
    tops = torch.randint(0, 4, (B, Cc), generator=g).to(F64) + T         # the top value varies by channel, not by source
    for b in range(B):
        for grp in range(5):
            for cc in range(Cc):
                if feas and n < 4 * len(feas):
                    cand = pairs[feas[n % len(feas)]]
                    pos = cand[int(torch.randint(0, cand.shape[0], (1,), generator=g))].tolist()
                    if n % 3 == 0 and HW > 6:
                        pos.append(int(torch.randint(0, HW, (1,), generator=g)))
                else:                                                   # (few pixels: fewer tops, so that a lower value remains)
                    pos = torch.randint(0, HW, (min(1 + n % 3, max(1, (HW - 1) // 2)),), generator=g).tolist()
                n += 1
                for s in (range(4) if grp == 4 else (grp,)):
                    xs[s][b, pos, cc] = tops[b, cc]
    st = [stored(x, dtype, "x") for x in xs]
    ref = pool(xs, dtype)
    cov = tie_coverage(ref["all5"], Cc, dtype)
    missing = [name for name in feas if cov[name] == 0]
    assert not missing, f"tie relations never met: {missing}"
    src_am, intra_am = ref["argmax"][:, :4 * Cc].view(B, 4, Cc), ref["argmax"][:, 4 * Cc:].view(B, 1, Cc)
    assert bool((src_am == intra_am).any()) and (HW == 1 or bool((src_am != intra_am).any()))
    ref["coverage"], ref["feasible"] = cov, feas
    return st, ref


def make_pool_nan(B, HW, Cc, dtype, seed=23):
    """the rounding inputs with channel 1 of source 2 all NaN in the last sample (so intra's channel 1 is NaN there too)"""
    st, ref = make_pool_rounding(B, HW, Cc, dtype, seed)
    st[2][B - 1, :, 1] = float("nan")
    nan = torch.zeros(B, 5 * Cc, dtype=torch.bool)
    nan[B - 1, 2 * Cc + 1] = nan[B - 1, 4 * Cc + 1] = True
    return st, ref, nan


# ------------------------------------------------------------------------------------------------------------------------------
# the two MLPs
# ------------------------------------------------------------------------------------------------------------------------------
# ca = 1.f / (1.f + expf(-z)) on an exact z: expf within 1 ulp = 2 * 2^-24 (the figure of the HIP math accuracy table, which is not at
# hand here: taken from memory of the public ROCm documentation), the sum 1 + e rounds once = 1, and the division is the correctly
# rounded one (hipcc's default, no fast-math flag in csrc/Makefile): it is the output rounding, the half ulp of the bound.  A relative
# error of the denominator is at most the same relative error of the quotient: n = 3 on |ref|.
N_SIGMOID = 3


def _fc_scale(n):
    """a power of two near 1 / sqrt(n): keeps a dot product of n terms of order one"""
    return 2.0 ** -round(0.5 * torch.log2(torch.tensor(float(n))).item())


def make_mlp(Cc, B, seed=31):
    """avg, mx [B, 5C] halves of integers; fc weights [-1, -1/2, 0, 1/2, 1] times a power of two, so the sigmoid arguments stay of
    order one"""
    C4, H = 4 * Cc, Cc // 4
    d = {"avg": ints((B, 5 * Cc), -4, 4, seed) / 2.0, "mx": ints((B, 5 * Cc), -4, 4, seed + 1) / 2.0}
    vals = [-1, -0.5, 0, 0.5, 1]
    d["w1"] = pick(vals, (H, C4), seed + 2) * _fc_scale(C4)
    d["w2"] = pick(vals, (C4, H), seed + 3) * _fc_scale(H)
    d["v1"] = pick(vals, (H, Cc), seed + 4) * _fc_scale(Cc)
    d["v2"] = pick(vals, (Cc, H), seed + 5) * _fc_scale(H)
    return d


def mlp(avg, mx, w1, w2, v1, v2, exact=True):
    """-> hidden [B, 2, H1 + H2] (rows: from avg, from max; columns: the H1 units of ca, then the H2 of ca1), the sigmoid arguments
    z, z1 and ca [B, 4C], ca1 [B, C] with their bounds"""
    C4 = w1.shape[1]

    def hid(v):
        return torch.relu(torch.cat([_dot("bc,jc->bj", v[:, :C4], w1, "fc1", exact), _dot("bc,jc->bj", v[:, C4:], v1, "ca1 fc1", exact)], 1))
    H1 = w1.shape[0]
    ha, hm = hid(avg), hid(mx)
    za, zm = _dot("bj,cj->bc", ha[:, :H1], w2, "fc2 avg", exact), _dot("bj,cj->bc", hm[:, :H1], w2, "fc2 max", exact)
    ya, ym = _dot("bj,cj->bc", ha[:, H1:], v2, "ca1 fc2 avg", exact), _dot("bj,cj->bc", hm[:, H1:], v2, "ca1 fc2 max", exact)
    z, z1 = _ex(za + zm, "z", exact), _ex(ya + ym, "z1", exact)
    ca, ca1 = torch.sigmoid(z), torch.sigmoid(z1)
    return {"hidden": torch.stack([ha, hm], 1), "z": z, "z1": z1, "ca": ca, "ca1": ca1,
            "ca_bound": half_ulp(ca, F32) + N_SIGMOID * U * ca.abs(), "ca1_bound": half_ulp(ca1, F32) + N_SIGMOID * U * ca1.abs()}


# ------------------------------------------------------------------------------------------------------------------------------
# fusion + conv_final, forward
# ------------------------------------------------------------------------------------------------------------------------------
def make_final(B, HW, Cc, dtype, seed=41):
    xs, st = make_x(B, HW, Cc, dtype, -4, 4, seed)
    d = {"xs": xs, "x": st, "ca": eighths((B, 4 * Cc), seed + 4), "ca1": eighths((B, Cc), seed + 5),
         "wf": ints((NCLS, 4 * Cc), -2, 2, seed + 6), "bias": ints((NCLS,), -3, 3, seed + 7), "dl": ints((B, NCLS, HW), -4, 4, seed + 8)}
    d["ca"][:, 0], d["ca"][:, 1], d["ca1"][:, 0] = 0.0, 1.0, 0.0       # (the ends of the range in every sample)
    return d


def final_forward(xs, ca, ca1, wf, bias, exact=True):
    """logits[b, k, p] = beff[b, k] + sum_c weff[b, k, c] * cat[b, p, c]; weff = Wf * ca, beff = bias + sum_c weff * ca1[c % C]"""
    cat = torch.cat(list(xs), -1)
    weff = _ex(wf[None] * ca[:, None, :], "weff", exact)
    beff = _dot("bkc,bc->bk", weff, ca1.repeat(1, 4), "beff", exact, plus=bias[None].expand(ca.shape[0], -1))
    return _dot("bpc,bkc->bkp", cat, weff, "logits", exact, plus=beff[:, :, None].expand(-1, -1, cat.shape[1]))


# ------------------------------------------------------------------------------------------------------------------------------
# backward, phase A: the reductions over the pixels
# ------------------------------------------------------------------------------------------------------------------------------
def backward_reduce(xs, dl, ca, ca1, wf, exact=True):
    """G[b, k, c] = sum_p dl * cat, DL[b, k] = sum_p dl; t = G + ca1[c % C] * DL; dca = sum_k Wf * t; dca1[cc] = sum_j ca[cc + jC] *
    sum_k Wf[k, cc + jC] * DL; dWf = sum_b ca * t; dbias = sum_b DL"""
    cat = torch.cat(list(xs), -1)
    B, Cc = ca1.shape
    G = _dot("bkp,bpc->bkc", dl, cat, "G", exact)
    if exact:
        sum_exact(dl, (2,), "DL")
    DL = dl.sum(2)
    r = ca1.repeat(1, 4)
    t = _ex(G + _ex(r[:, None, :] * DL[:, :, None], "ca1 * DL", exact), "G + ca1 * DL", exact)
    dca = _dot("kc,bkc->bc", wf, t, "dca", exact)
    s1 = _dot("kc,bk->bc", wf, DL, "Wf * DL", exact)
    prod = _ex(ca * s1, "ca * sum_k Wf DL", exact).view(B, 4, Cc)
    dwf = _dot("bc,bkc->kc", ca, t, "dWf", exact)
    if exact:
        sum_exact(prod, (1,), "dca1"), sum_exact(DL, (0,), "dbias")
    return {"G": G, "DL": DL, "dca": dca, "dca1": prod.sum(1) + 0.0, "dwf": dwf, "dbias": DL.sum(0) + 0.0}


# ------------------------------------------------------------------------------------------------------------------------------
# MLP backward
# ------------------------------------------------------------------------------------------------------------------------------
def make_mlp_backward(Cc, B, seed=51):
    """what ksmi_ecam_mlp_backward reads, all dyadic: ca / ca1 multiples of 1/8, hidden non-negative halves with a third of zeros
    (the ReLU gate), integer fc weights"""
    C4, H = 4 * Cc, Cc // 4
    d = {"avg": ints((B, 5 * Cc), -4, 4, seed) / 2.0, "mx": ints((B, 5 * Cc), -4, 4, seed + 1) / 2.0,
         "hidden": ints((B, 2, 2 * H), -2, 4, seed + 2).clamp_min(0.0) / 2.0,
         "ca": eighths((B, C4), seed + 3), "ca1": eighths((B, Cc), seed + 4),
         "dca": ints((B, C4), -4, 4, seed + 5), "dca1": ints((B, Cc), -4, 4, seed + 6),
         "w1": ints((H, C4), -2, 2, seed + 7), "w2": ints((C4, H), -2, 2, seed + 8),
         "v1": ints((H, Cc), -2, 2, seed + 9), "v2": ints((Cc, H), -2, 2, seed + 10)}
    assert bool((d["hidden"] == 0).any()) and bool((d["hidden"] > 0).any())
    return d


def _dot2(eq, a0, b0, a1, b1, what, exact):
    """einsum(a0, b0) + einsum(a1, b1) accumulated in one chain"""
    out = torch.einsum(eq, a0, b0) + torch.einsum(eq, a1, b1)
    if exact:
        for v in (a0, b0, a1, b1):
            exact_f32(v, what)
        q = min(quantum(a0) * quantum(b0), quantum(a1) * quantum(b1))
        top = torch.einsum(eq, a0.abs(), b0.abs()) + torch.einsum(eq, a1.abs(), b1.abs())
        assert float(top.max()) < 2.0 ** 24 * q, f"{what}: partial sums up to {float(top.max())} at quantum {q} are not exact in fp32"
        exact_f32(out, what)
    return out + 0.0


def mlp_backward(avg, mx, hidden, ca, ca1, dca, dca1, w1, w2, v1, v2, exact=True):
    """ds = d * s * (1 - s) over [ca | ca1]; dh = (hidden > 0) * fc2^T ds (the same ds for the avg and the max row); davg / dmax =
    fc1^T dh of the row; weight gradients summed over the samples: fc2[c, j] = sum_b ds[c] * (h_avg + h_max)[j],
    fc1[j, c] = sum_b dh_avg[j] * avg[c] + dh_max[j] * max[c]"""
    C4, H1 = w1.shape[1], w1.shape[0]
    s, d = torch.cat([ca, ca1], 1), torch.cat([dca, dca1], 1)
    ds = _ex(_ex(d * s, "d * s", exact) * _ex(1.0 - s, "1 - s", exact), "ds", exact)
    a = torch.cat([_dot("bc,cj->bj", ds[:, :C4], w2, "dh", exact), _dot("bc,cj->bj", ds[:, C4:], v2, "dh ca1", exact)], 1)
    dh = torch.where(hidden > 0, a[:, None, :].expand_as(hidden), torch.zeros((), dtype=F64))

    def back(row):
        return torch.cat([_dot("bj,jc->bc", row[:, :H1], w1, "davg", exact), _dot("bj,jc->bc", row[:, H1:], v1, "davg ca1", exact)], 1)
    hs = _ex(hidden[:, 0] + hidden[:, 1], "h_avg + h_max", exact)
    return {"ds": ds, "dh": dh, "davg": back(dh[:, 0]), "dmax": back(dh[:, 1]),
            "gw2": _dot("bc,bj->cj", ds[:, :C4], hs[:, :H1], "g fc2", exact), "gv2": _dot("bc,bj->cj", ds[:, C4:], hs[:, H1:], "g ca1 fc2", exact),
            "gw1": _dot2("bj,bc->jc", dh[:, 0, :H1], avg[:, :C4], dh[:, 1, :H1], mx[:, :C4], "g fc1", exact),
            "gv1": _dot2("bj,bc->jc", dh[:, 0, H1:], avg[:, C4:], dh[:, 1, H1:], mx[:, C4:], "g ca1 fc1", exact)}


# ------------------------------------------------------------------------------------------------------------------------------
# backward, phase B: dx and the max-pool scatter
# ------------------------------------------------------------------------------------------------------------------------------
# a = cst + w0 d0 + w1 d1 + w2 d2 with cst = (davg[c] + davg[4C + c % C]) * (1.f / HW).  The products w * d and the sum of the two davg
# are exact on these inputs.  Roundings: 1.f / HW, its product, and the three accumulations.  fp32: the last accumulation is the output
# rounding (the half ulp of the bound), n = 4; bf16: the conversion is the output rounding, n = 5.
N_DX = {F32: 4, BF16: 5}


def make_dx(B, HW, Cc, dtype, seed=61):
    d = {"dl": ints((B, NCLS, HW), -4, 4, seed), "ca": eighths((B, 4 * Cc), seed + 1), "wf": ints((NCLS, 4 * Cc), -2, 2, seed + 2),
         "davg": ints((B, 5 * Cc), -8, 8, seed + 3) * 4.0, "dmax": ints((B, 5 * Cc), -8, 8, seed + 4) / 2.0}
    am = torch.randint(0, HW, (B, 5 * Cc), generator=torch.Generator().manual_seed(seed + 5))
    am[:, 4 * Cc] = am[:, 0]                                            # channel 0: source 0 and intra scatter to the same pixel
    am[:, 1:4 * Cc:Cc] = am[:, 4 * Cc + 1:4 * Cc + 2]                   # channel 1: all four sources and intra do
    if HW > 1:
        am[:, 4 * Cc + 2] = (am[:, 2] + 1) % HW                         # channel 2: source 0 and intra differ
    d["argmax"] = am.to(torch.int32)
    src, intra = am[:, :4 * Cc].view(B, 4, Cc), am[:, 4 * Cc:].view(B, 1, Cc)
    assert bool((src == intra).all(1).any()) and (HW == 1 or bool((src != intra).any()))
    return d


def backward_dx(dl, ca, wf, davg, dmax, argmax, dtype, exact=True):
    """dx_s[b, p, cc] = (davg[sC + cc] + davg[4C + cc]) / HW + sum_k weff[k, sC + cc] * dl[b, k, p], rounded to the activation dtype; then,
    in the kernel's store order, the element at the first-maximum pixel of source s gets dmax[sC + cc] added in fp32 and is rounded again,
    and the four elements at the first-maximum pixel of intra get dmax[4C + cc] and are rounded again.
    -> {"dx": four [B, HW, C] float64, "bound": four tensors or None (None: compare the bits)}"""
    B, _, HW = dl.shape
    Cc = ca.shape[1] // 4
    C4 = 4 * Cc
    bits = exact and is_pow2(HW)
    weff = _ex(wf[None] * ca[:, None, :], "weff", exact)
    dsum = _ex(davg[:, :C4] + davg[:, C4:].repeat(1, 4), "davg + davg intra", exact)
    cst = _ex(dsum / HW, "cst", bits)
    a = _dot("bkp,bkc->bpc", dl, weff, "dx", bits, plus=cst[:, None, :].expand(-1, HW, -1))
    mag = torch.einsum("bkp,bkc->bpc", dl.abs(), weff.abs()) + cst.abs()[:, None, :]
    v = _store(a, dtype, bits, "dx") if bits else a.clone()             # bound mode: v stays the unrounded reference
    err = None if bits else half_ulp(a, dtype) + N_DX.get(dtype, 0) * U * mag
    bi, ci = torch.arange(B)[:, None], torch.arange(Cc)[None, :]
    am = argmax.long()

    def update(s, pix, g):
        col = s * Cc + ci
        new = _ex(v[bi, pix, col] + g, "scatter sum", bits)
        v[bi, pix, col] = _store(new, dtype, bits, "scatter") if bits else new
        if not bits:
            # one more rounding to the activation dtype; for bf16 the fp32 sum before it rounds too
            mag[bi, pix, col] += g.abs()
            err[bi, pix, col] += half_ulp(new, dtype) + (U * mag[bi, pix, col] if dtype == BF16 else 0.0)
    for s in range(4):
        update(s, am[:, s * Cc:(s + 1) * Cc], dmax[:, s * Cc:(s + 1) * Cc])
    for s in range(4):
        update(s, am[:, C4:], dmax[:, C4:])
    return {"dx": [v[..., s * Cc:(s + 1) * Cc].contiguous() for s in range(4)],
            "bound": None if bits else [err[..., s * Cc:(s + 1) * Cc].contiguous() for s in range(4)]}


# ------------------------------------------------------------------------------------------------------------------------------
# the whole head in one differentiable function
# ------------------------------------------------------------------------------------------------------------------------------
def chain(xs, p, intra_dtype=None):
    """models/snunet.py:49-62 and :146-151 on NHWC tensors, in the dtype of the arguments: ChannelAttention (avg pool and max pool over
    the pixels, fc1, ReLU, fc2, summed, sigmoid) of the concatenation and of intra = the sum of the four sources, then
    ca * (cat + repeat(ca1)) and the 1x1 conv.  The maximum is gathered at the first pixel that attains it, so autograd sends its
    gradient to that pixel alone.  intra_dtype = bfloat16 rounds intra as the bf16 reference does (straight through for the gradient).
    xs: four [B, HW, C]; p: w1 [C/4, 4C], w2 [4C, C/4], v1 [C/4, C], v2 [C, C/4], wf [3, 4C], bias [3] -> logits [B, 3, HW]"""
    cat = torch.cat(list(xs), -1)
    intra = ((xs[0] + xs[1]) + xs[2]) + xs[3]
    if intra_dtype == BF16:
        intra = intra + (intra.detach().float().to(BF16).to(intra.dtype) - intra.detach())

    def attention(t, fc1, fc2):
        HW = t.shape[1]
        d = t.detach()
        pix = torch.arange(HW).view(1, HW, 1)
        first = torch.where(d == d.max(1, keepdim=True).values, pix, torch.tensor(HW)).min(1, keepdim=True).values
        avg, mx = t.mean(1), t.gather(1, first).squeeze(1)
        return torch.sigmoid(torch.relu(avg @ fc1.T) @ fc2.T + torch.relu(mx @ fc1.T) @ fc2.T)
    ca, ca1 = attention(cat, p["w1"], p["w2"]), attention(intra, p["v1"], p["v2"])
    out = ca[:, None, :] * (cat + ca1.repeat(1, 4)[:, None, :])
    return (out @ p["wf"].T + p["bias"]).permute(0, 2, 1)


CHAIN_PARAMS = ["w1", "w2", "v1", "v2", "wf", "bias"]


@functools.lru_cache(maxsize=None)
def make_chain(dtype, Cc=CHAIN_CASE[0], B=CHAIN_CASE[1], HW=CHAIN_CASE[2], seed=71):
    """gaussian inputs as stored in `dtype`, with a unique maximum in every channel of every source and of intra (asserted: the pixel
    that receives the max-pool gradient must not depend on rounding)"""
    xs = [gauss((B, HW, Cc), seed + s).float().to(dtype).double() for s in range(4)]
    bi, ci = torch.arange(B)[:, None], torch.arange(Cc)[None, :]
    for x in xs:                                                        # lift every source's maximum by 1,
        x[bi, x.argmax(1), ci] += 1.0
    q = (((xs[0] + xs[1]) + xs[2]) + xs[3]).argmax(1)
    for x in xs:                                                        # then intra's by 4 * 1/2
        x[bi, q, ci] += 0.5
    xs = [x.float().to(dtype) for x in xs]
    H = Cc // 4
    p = {"w1": gauss((H, 4 * Cc), seed + 4, (4 * Cc) ** -0.5), "w2": gauss((4 * Cc, H), seed + 5, H ** -0.5), "v1": gauss((H, Cc), seed + 6, Cc ** -0.5),
         "v2": gauss((Cc, H), seed + 7, H ** -0.5), "wf": gauss((NCLS, 4 * Cc), seed + 8, (4 * Cc) ** -0.5), "bias": gauss((NCLS,), seed + 9)}
    p = {k: v.float() for k, v in p.items()}
    dl = gauss((B, NCLS, HW), seed + 10, 1.0 / HW).float()
    all5 = pool([x.double() for x in xs], dtype, exact=False)["all5"]
    top2 = all5.topk(2, dim=1).values
    gap = float((top2[:, 0] - top2[:, 1]).min())
    assert gap >= 0.25, f"a channel's maximum is not unique by a margin: {gap}"
    return {"x": xs, "p": p, "dl": dl, "gap": gap}


def chain_reference(d, dtype, compute):
    """logits and every gradient of the head by autograd in `compute` (float64: the reference; float32: the yardstick, with dx rounded to
    the activation dtype as a kernel stores it) -> {name: float64 tensor}"""
    xs = [x.to(compute).requires_grad_(True) for x in d["x"]]
    p = {k: v.to(compute).requires_grad_(True) for k, v in d["p"].items()}
    logits = chain(xs, p, dtype)
    logits.backward(d["dl"].to(compute))
    out = {"logits": logits.detach().double()}
    for s in range(4):
        g = xs[s].grad
        out[f"dx{s}"] = (g.to(dtype) if compute != F64 else g).double()
    for k in CHAIN_PARAMS:
        out["d" + k] = p[k].grad.double()
    return out


def chain_tolerance(ref64, cpu32, name, out_dtype):
    """4 * max(the largest error of the fp32 yardstick, half an ulp of the output dtype at the largest reference value)"""
    floor = float(half_ulp(ref64[name].abs().max().view(1), out_dtype))
    return 4.0 * max(float((cpu32[name] - ref64[name]).abs().max()), floor)


# ------------------------------------------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_head.py: inputs and expected outputs (tests/test_head_ref_cpu.py builds every one of them, so the
# exactness preconditions and the coverage conditions are checked without a GPU)
# ------------------------------------------------------------------------------------------------------------------------------
POOL_KINDS = ["rounding", "ties"]


def case_pool(kind, c):
    Cc, dtype, B, HW = c
    return (make_pool_rounding if kind == "rounding" else make_pool_ties)(B, HW, Cc, dtype)


def case_final(c, forward=True, backward=True):
    Cc, dtype, B, HW = c
    d = make_final(B, HW, Cc, dtype)
    if forward:
        d["logits"] = final_forward(d["xs"], d["ca"], d["ca1"], d["wf"], d["bias"])
    if backward:
        d["reduce"] = backward_reduce(d["xs"], d["dl"], d["ca"], d["ca1"], d["wf"])
    return d


def case_mlp(Cc, B):
    d = make_mlp(Cc, B)
    d["ref"] = mlp(d["avg"], d["mx"], d["w1"], d["w2"], d["v1"], d["v2"])
    return d


MLP_BWD_ARGS = ["avg", "mx", "hidden", "ca", "ca1", "dca", "dca1", "w1", "w2", "v1", "v2"]


def case_mlp_backward(Cc, B):
    d = make_mlp_backward(Cc, B)
    d["ref"] = mlp_backward(*[d[k] for k in MLP_BWD_ARGS])
    return d


def case_dx(c):
    Cc, dtype, B, HW = c
    d = make_dx(B, HW, Cc, dtype)
    d["ref"] = backward_dx(d["dl"], d["ca"], d["wf"], d["davg"], d["dmax"], d["argmax"], dtype)
    assert (d["ref"]["bound"] is None) == is_pow2(HW)
    return d
