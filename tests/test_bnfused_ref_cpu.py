"""The composed oracles of tests/bnfused_ref.py against torch (float64, tie-free gaussian data), and every case of
tests/test_gpu_bnfused.py built here: building a case runs its oracles, whose exactness assertions fail here, without a GPU, if an input
is not exactly computable in fp32."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnfused_ref as N  # noqa: E402
import elementwise_ref as R  # noqa: E402

F64 = torch.float64


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# the oracles against torch
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count,shape", [(64.0, (1, 8, 8)), (64.0, (2, 4, 8)), (64.0, (4, 2, 8))])
def test_forward_composition_matches_batch_norm_relu_max_pool(count, shape):
    """statistics rows -> finish -> scale / shift -> + identity -> ReLU -> 2x2 pool, against native_batch_norm(training) + relu +
    max_pool2d on data that has exactly the statistics the rows state (channel 0, the clamp: constant data, variance 0)"""
    B, H, W = shape
    C, npix = 12, B * H * W
    assert npix == count
    st = N.make_fin_stats(3, C, 4, count=count, seed=77)
    want = N.fin_expect(st, C)
    z = R.gauss((npix, C), 78)
    z = (z - z.mean(0)) / z.var(0, unbiased=False).sqrt() * st["var_want"].sqrt() + st["mean_want"]
    idn = R.gauss((npix, C), 79, 2.0)
    rm, rv = st["rmean"].double().clone(), st["rvar"].double().clone()
    y, save_mean, save_rstd = torch.native_batch_norm(z, st["gamma"].double(), st["beta"].double(), rm, rv, True, N.MOMENTUM, N.EPS)
    out = torch.relu(y + idn)
    pooled = F.max_pool2d(out.view(B, H, W, C).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    _close(want["mean"].double(), save_mean)
    _close(want["rstd"].double(), save_rstd)
    _close(want["rmean"].double(), rm)
    _close(want["rvar"][0], rv)
    got, _ = N.add_relu_real(z, idn, want["scale"].double(), want["shift"].double())
    _close(got, out)
    _close(N.pool_of(got, B, H, W), pooled)
    assert float(want["rstd"][0]) == 1.0 and float(save_rstd[0]) == 1.0                       # channel 0: the clamp var = 0


def test_exact_and_real_forward_expressions_agree_on_dyadic_data():
    """R.bn_add_relu (exact, asserted) and add_relu_real are the same expression: equal where both apply"""
    for dtype in R.DTYPES:
        d = N.make_fin_add_relu(2, 6, 10, 24, dtype, 1)
        w = d["want"]
        v, _ = N.add_relu_real(d["z"].double(), d["idn"].double(), w["scale"].double(), w["shift"].double())
        assert torch.equal(R.stored(v, dtype), w["out"])
        assert torch.equal(w["pooled"].double(), F.max_pool2d(w["out"].double().view(2, 6, 10, 24).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1))


def test_the_negative_zero_rows_reach_the_relu():
    d = N.make_fin_add_relu(1, 1, 37, 8, R.F32, 0)
    w = d["want"]
    z, idn, sc, sh = d["z"].double(), d["idn"].double(), w["scale"].double(), w["shift"].double()
    assert torch.signbit(sh[1]) and float(sh[1]) == 0.0 and float(sc[1]) > 0 and float(sc[2]) < 0
    pre = z[0] * sc + sh + idn[0]
    assert torch.signbit(pre[1]) and float(pre[1]) == 0.0                                        # -0.0 before the maximum
    assert not torch.signbit(pre[2]) and float(pre[2]) == 0.0 and torch.signbit((z[0] * sc)[2])  # a -0.0 product, a +0.0 sum
    assert not torch.signbit(w["out"].float()).any()
    assert float(w["rstd"][0]) == 1.0 and float(w["mean"][0]) != 0.0                            # channel 0: clamped


def test_statistics_rows_total_what_they_are_meant_to():
    for C, rows in N.ROWSUM_CASES:
        for pad in (0, 4):
            d = N.make_bwd(N.ROWSUM_NPIX, C, R.F32, rows, pad)
            p = d["partial"].double()
            assert p.shape == (rows, 2, C + pad)
            assert torch.equal(p[:, :, :C].sum(0), d["sums"].double())
            assert bool((p[:, :, C:] == R.SENTINEL).all())
            st = N.make_fin_stats(rows, C, pad)
            q = st["partial"].double()
            mean, var = st["mean_want"], st["var_want"].clone()
            assert torch.equal(q[:, 0, :C].sum(0), N.COUNT * mean)
            assert torch.equal(q[:, 1, 1:C].sum(0), (N.COUNT * (var + mean * mean))[1:])
            assert not q[:, 1, 0].any() and float(mean[0]) != 0.0                               # the clamp channel: q = 0, s != 0
            assert bool((q[:, :, C:] == R.SENTINEL).all())


def test_partial_after_a_fused_call():
    """folded above 512 rows (rows 0..31, data columns only), untouched up to 512: the standalone reducers fold above 256"""
    for rows in (256, 257, 512):
        p = N.make_bwd(1, 8, R.F32, rows, 4)["partial"]
        assert torch.equal(N.partial_after(p, 8), p)
    assert not torch.equal(R.folded(N.make_bwd(1, 8, R.F32, 257, 4)["partial"], 8), N.make_bwd(1, 8, R.F32, 257, 4)["partial"])
    p = N.make_bwd(1, 8, R.F32, 513, 4)["partial"]
    a = N.partial_after(p, 8)
    assert torch.equal(a[32:], p[32:]) and torch.equal(a[:, :, 8:], p[:, :, 8:]) and not torch.equal(a[:32], p[:32])
    assert torch.equal(a[:32, :, :8].double().sum(0), p[:, :, :8].double().sum(0))


def test_backward_oracle_on_fused_rows_matches_autograd():
    """the rows -> sums -> apply composition: rows that total the true (sum g, sum g * xhat) give autograd's dz"""
    npix, C = 203, 12
    z0, dout = R.gauss((npix, C), 90, 2.0), R.gauss((npix, C), 91, 2.0)
    gamma, beta = R.gauss((C,), 92), R.gauss((C,), 93)
    z = z0.clone().requires_grad_(True)
    out = torch.relu(F.batch_norm(z, None, None, gamma, beta, training=True, eps=1e-5))
    out.backward(dout)
    mean, rstd = z0.mean(0), 1.0 / (z0.var(0, unbiased=False) + 1e-5).sqrt()
    k = {"dout": dout, "out": out.detach(), "z": z0, "mean": mean, "rstd": rstd, "gamma": gamma, "count": float(npix)}
    rows, _ = R.bnrelu_bwd_reduce(k, 5, exact=False)                                             # [5, 2, C]: what the convolution epilogue hands over
    _, dz, _ = R.bn_bwd_apply(k, F64, exact=False, sums=rows.sum(0))
    _close(dz, z.grad)


# ------------------------------------------------------------------------------------------------------------------------------
# every case of the GPU file builds, i.e. passes its oracles' exactness assertions
# ------------------------------------------------------------------------------------------------------------------------------
def test_gpu_forward_cases_are_exactly_computable():
    for (B, H, W), C, pooled in N.FIN_CASES:
        for dtype in N.dtypes_of(C):
            d = N.make_fin_add_relu(B, H, W, C, dtype, pooled)
            w = d["want"]
            assert set(w["rstd"].tolist()) <= {1.0, 0.5, 0.25, 0.125}
            assert not bool(w["rvar"][2].all()) or C < 16                                       # some channels take the bound, the rest are exact
            assert (w["out"].float() == 0).any() or B * H * W == 1
    for rows in (1, 85, 513):                                                                    # the row-sum spot checks of the forward pass
        N.make_fin_add_relu(1, 1, 37, 24, R.BF16, 0, rows=rows)
    w = N.make_fin_add_relu(2, 6, 10, 24, R.F32, 1, count=1.0)["want"]
    assert bool(w["rvar"][2].all())                                                              # count = 1: the biased variance, exact everywhere


def test_gpu_big_cases_are_exactly_computable():
    for (B, H, W), C, pooled in N.FIN_BIG:
        n = B * H * W * C // 4 if not pooled else B * (H // 2) * (W // 2) * C // 4
        assert n > (2 - pooled) * 256 * 1024                                                     # a second grid-stride trip at the default grid cap
        N.make_fin_add_relu(B, H, W, C, R.F32, pooled)
    npix, C = N.BWD_BIG
    assert npix * C // 4 > 2 * 256 * 1024
    N.case_bwd_fin_apply("relu", npix, C, R.F32, 3, 4)


def test_gpu_backward_cases_are_exactly_computable():
    for C, rows in N.ROWSUM_CASES:
        for dtype in N.dtypes_of(C):
            for pad, _, acc in N.ROWSUM_VARIANTS:
                d, _, _ = N.case_bwd_fin_apply("gated", N.ROWSUM_NPIX, C, dtype, rows, pad)
                N.bwd_finish(d, C, acc)
    for C, rows in N.ROWSUM_SPOT:
        d, _, _ = N.case_bwd_fin_apply("relu", N.ROWSUM_NPIX, C, R.BF16, rows, 4)
        N.bwd_finish(d, C, 1)
        N.case_bwd_fin_apply_add(N.ROWSUM_NPIX, C, R.BF16, rows, 4)
    odd = 0
    for npix in N.BWD_NPIX:
        for C in N.BWD_C:
            for dtype in R.DTYPES:
                odd += (npix * C // R.vec_of(dtype)) % 2
                for mode in N.BWD_MODES:
                    d, g, _ = N.case_bwd_fin_apply(mode, npix, C, dtype, 3, 4)
                    if mode == "relu":
                        o = d["out"].float()
                        assert torch.signbit(o[o == 0]).any() and not torch.signbit(g.float()[o <= 0]).any()   # -0.0 in `out` gates to +0.0
    assert odd > 0                                                                               # an odd total vector count: the lone last vector
    for npix in N.BWD_NPIX:
        for C in N.ADD_C:
            for dtype in R.DTYPES:
                _, _, parts = N.case_bwd_fin_apply_add(npix, C, dtype, 3, 4)
                for b, p in parts.items():
                    assert p.shape == (b, C)
                    if b > npix:
                        assert not p[npix:].any() and not torch.signbit(p[npix:]).any()          # empty slabs: rows of +0.0


def test_real_data_cases_build():
    for dtype in R.DTYPES:
        for shape in (N.REAL_SHAPE, N.REAL_POOL_SHAPE):
            d = N.make_real_forward(*shape, N.REAL_C, dtype)
            ref = R.bn_finalize(d["partial"], N.REAL_C, d["count"], d["gamma"], d["beta"], d["rmean"], d["rvar"], R.MOMENTUM, R.EPS, True)
            rs = ref["rstd"][0]
            assert bool((rs > 0.3).all()) and bool((rs < 1.0).all())                            # a sample of standard deviation 2
            assert not torch.equal(rs.float().double(), rs)                                      # and nothing dyadic about it
        d = N.make_real_bwd(N.REAL_NPIX, N.REAL_C, dtype)
        _close(d["sums64"], d["partial"].double()[:, :, :N.REAL_C].sum(0))
        assert bool((N.real_sums_bound(d) > 0).all())
