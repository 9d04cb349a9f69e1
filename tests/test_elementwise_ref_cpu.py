"""The float64 oracles of tests/elementwise_ref.py against torch (float64, tie-free random data), and the exactness preconditions of
every parametrised case of tests/test_gpu_elementwise.py: building a case runs its oracle, whose assertions fail here, without a GPU,
if an input is not exactly computable in fp32."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_ref as R  # noqa: E402

F64 = torch.float64
IDS = R.DTYPE_IDS


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# the oracles against torch
# ------------------------------------------------------------------------------------------------------------------------------
def _bn_data(npix=203, C=12, seed=100):
    d = {k: R.gauss((npix, C), seed + i, 2.0) for i, k in enumerate(("dout", "z", "r"))}
    d["gamma"], d["beta"] = R.gauss((C,), seed + 5), R.gauss((C,), seed + 6)
    return d


def test_bnrelu_backward_oracle_matches_autograd():
    d = _bn_data()
    z = d["z"].clone().requires_grad_(True)
    out = torch.relu(F.batch_norm(z, None, None, d["gamma"], d["beta"], training=True, eps=1e-5))
    out.backward(d["dout"])
    mean, rstd = d["z"].mean(0), 1.0 / (d["z"].var(0, unbiased=False) + 1e-5).sqrt()
    k = {"dout": d["dout"], "out": out.detach(), "z": d["z"], "mean": mean, "rstd": rstd, "gamma": d["gamma"], "count": float(z.shape[0])}
    for rows in (1, 5, 300):
        p, _ = R.bnrelu_bwd_reduce(k, rows, exact=False)
        sums = p.sum(0)
        _close(sums[0], (d["dout"] * (out > 0)).sum(0))
        g, dz, _ = R.bn_bwd_apply(k, F64, exact=False, sums=sums)
        _close(dz, z.grad)
        assert torch.equal(g, d["dout"] * (out.detach() > 0))
    # alpha scales the result; the pre-gated variant takes g as it comes
    k2 = dict(k, dout=g, sums=sums)
    _, dz2, _ = R.bn_bwd_apply(k2, F64, alpha=0.5, gate=False, exact=False)
    _close(dz2, 0.5 * z.grad)


def test_bn_bwd_apply_add_oracle_matches_autograd():
    """out = relu(bn(x) + 2 x): the gradient of x is 2 g (the identity branch) + the BatchNorm backward of g, g = dout * (out > 0);
    the kernel's operands are r = the gradient entering the BatchNorm, g = the identity branch's, i = x"""
    d = _bn_data(seed=200)
    x = d["z"].clone().requires_grad_(True)
    out = torch.relu(F.batch_norm(x, None, None, d["gamma"], d["beta"], training=True, eps=1e-5) + 2.0 * x)
    out.backward(d["dout"])
    g = d["dout"] * (out.detach() > 0)
    mean, rstd = d["z"].mean(0), 1.0 / (d["z"].var(0, unbiased=False) + 1e-5).sqrt()
    xh = (d["z"] - mean) * rstd
    sums = torch.stack([g.sum(0), (g * xh).sum(0)])
    k = {"r": g, "dout": 2.0 * g, "z": d["z"], "mean": mean, "rstd": rstd, "gamma": d["gamma"], "sums": sums, "count": float(x.shape[0])}
    di, _ = R.bn_bwd_apply_add(k, 4, F64, exact=False)
    _close(di, x.grad)
    p, _ = R.bias_partial(di, 4, exact=False)
    _close(p.sum(0), di.sum(0))


def test_slab_sums_cover_every_pixel_once():
    x = R.gauss((1073, 3), 5)
    for rows in (1, 3, 8, 1073, 2000):
        p0, p1 = R.slab_bounds(1073, rows)
        assert int(p0[0]) == 0 and int(p1.max()) == 1073 and bool((p1[:-1] == p0[1:]).all())
        _close(R.slab_sums(x, rows).sum(0), x.sum(0))


def test_maxpool_oracle_matches_torch_on_tie_free_data():
    for B, H, W, C in R.POOL_CASES:
        d = R.make_maxpool(B, H, W, C, F64, ties=False)
        x = d["x"].clone().requires_grad_(True)
        y = F.max_pool2d(x.permute(0, 3, 1, 2), 2)
        dy = d["dy"].double()
        y.backward(dy.permute(0, 3, 1, 2))
        got, _ = R.maxpool_forward(d["x"])
        assert torch.equal(got, y.detach().permute(0, 2, 3, 1))
        assert torch.equal(R.maxpool_backward(d["x"], dy), x.grad)
        assert torch.equal(R.maxpool_backward(d["x"], dy, d["prior"].double()), x.grad + d["prior"].double())


def test_maxpool_oracle_tie_rule():
    """the first maximum in scan order (0,0), (0,1), (1,0), (1,1) wins, -0.0 and +0.0 compare equal"""
    x = torch.tensor([[1.0, 1.0], [1.0, 0.0]], dtype=F64).view(1, 2, 2, 1)
    assert R.maxpool_backward(x, torch.full((1, 1, 1, 1), 5.0, dtype=F64)).flatten().tolist() == [5.0, 0.0, 0.0, 0.0]
    x = torch.tensor([[0.0, 2.0], [2.0, 2.0]], dtype=F64).view(1, 2, 2, 1)
    assert R.maxpool_backward(x, torch.full((1, 1, 1, 1), 5.0, dtype=F64)).flatten().tolist() == [0.0, 5.0, 0.0, 0.0]
    x = torch.tensor([[-0.0, 0.0], [0.0, -1.0]], dtype=F64).view(1, 2, 2, 1)
    y, am = R.maxpool_forward(x)
    assert int(am) == 0 and torch.signbit(y).all()


def test_conv_first_oracles_match_torch():
    B, Cin, H, W, Cout = 2, 3, 20, 35, 24
    x, w, b = R.gauss((B, Cin, H, W), 1), R.gauss((Cout, Cin, 3, 3), 2), R.gauss((Cout,), 3)
    _close(R.conv_first(x, w, b), F.conv2d(x, w, b, padding=1).permute(0, 2, 3, 1))
    cols = F.unfold(x, 3, padding=1).view(B, Cin * 9, H, W).permute(0, 2, 3, 1)
    got = R.im2col3x3(x, Cin * 9 + 5)
    assert torch.equal(got[..., :Cin * 9], cols) and not got[..., Cin * 9:].any()
    w2 = w.clone().requires_grad_(True)
    dy = R.gauss((B, H, W, Cout), 4)
    F.conv2d(x, w2, None, padding=1).backward(dy.permute(0, 3, 1, 2))
    _close(R.conv_first_wgrad(x, dy, exact=False), w2.grad)
    xi, dyi = R.ints((B, Cin, H, W), -2, 2, 5), R.ints((B, H, W, Cout), -4, 4, 6)
    w3 = w.clone().requires_grad_(True)
    F.conv2d(xi, w3, None, padding=1).backward(dyi.permute(0, 3, 1, 2))
    assert torch.equal(R.conv_first_wgrad(xi, dyi), w3.grad)
    st, _ = R.conv_first_stats(R.ints((B, H, W, Cout), -9, 9, 7))
    assert st.shape == (B * 2 * 3, 2, Cout)
    v = R.ints((B, H, W, Cout), -9, 9, 7)
    assert torch.equal(st[:, 0].sum(0), v.sum((0, 1, 2))) and torch.equal(st[:, 1].sum(0), (v * v).sum((0, 1, 2)))
    assert torch.equal(st[4, 0], v[0, 16:20, 16:32].sum((0, 1)))        # row order (b, ty, tx): b = 0, ty = 1, tx = 1


def test_bn_finalize_oracle_matches_batch_norm_running_update():
    m, e = float(torch.tensor(R.MOMENTUM, dtype=torch.float32)), float(torch.tensor(R.EPS, dtype=torch.float32))
    d = R.make_bn_finalize(70, 16, 4096.0)
    ref = R.bn_finalize(d["partial"], 16, 4096.0, d["gamma"], d["beta"], d["rmean"], d["rvar"], R.MOMENTUM, R.EPS, True)
    # the same numbers through F.batch_norm: 4096 samples per channel with the case's mean and (biased) variance
    p = d["partial"].double()
    s, q = p[:, 0, :16].sum(0), p[:, 1, :16].sum(0)
    mean, var = s / 4096.0, (q / 4096.0 - (s / 4096.0) ** 2).clamp_min(0)
    z = R.gauss((4096, 16), 14)
    z = (z - z.mean(0)) / z.var(0, unbiased=False).sqrt() * var.sqrt() + mean
    trm, trv = d["rmean"].double(), d["rvar"].double()
    y = F.batch_norm(z, trm, trv, d["gamma"].double(), d["beta"].double(), training=True, momentum=m, eps=e)
    _close(ref["mean"][0], mean)
    _close(ref["rmean"][0], trm, 1e-9)
    _close(ref["rvar"][0], trv, 1e-9)
    _close(z * ref["scale"][0] + ref["shift"][0], y, 1e-8)
    assert abs(float(ref["rstd"][0][0]) - e ** -0.5) < 1e-9                                    # channel 0: the clamp var = 0
    ev = R.bn_finalize(None, 16, 4096.0, d["gamma"], d["beta"], d["rmean"], d["rvar"], R.MOMENTUM, R.EPS, False)
    ye = F.batch_norm(z, d["rmean"].double(), d["rvar"].double(), d["gamma"].double(), d["beta"].double(), training=False, eps=e)
    _close(z * ev["scale"][0] + ev["shift"][0], ye, 1e-9)


def test_helpers():
    assert R.quantum(torch.tensor([1.5, -4.0, 0.0], dtype=F64)) == 0.5
    assert R.quantum(torch.tensor([3.0 * 2 ** -11], dtype=F64)) == 2.0 ** -11
    with pytest.raises(AssertionError):
        R.sum_exact(torch.full((2 ** 12, 1), 2.0 ** 12 + 1, dtype=F64), (0,), "too long")
    with pytest.raises(AssertionError):
        R.exact_f32(torch.tensor([1.0 + 2.0 ** -30], dtype=F64), "x")
    assert float(R.half_ulp(torch.tensor([1.0, 3.0, 0.75], dtype=F64), R.F32)[0]) == 2.0 ** -24
    assert R.half_ulp(torch.tensor([1.0, 3.0, 0.75], dtype=F64), R.BF16).tolist() == [2.0 ** -8, 2.0 ** -7, 2.0 ** -9]


# ------------------------------------------------------------------------------------------------------------------------------
# every case of the GPU file builds, i.e. passes its oracle's exactness assertions
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_gpu_cases_are_exactly_computable(dtype):
    for c in R.LAYOUT_CASES:
        R.case_layout(*c, dtype)
    for npix, rows in R.CHANNEL_SUM_SHAPES:
        for C in R.CHANNEL_SUM_C + [R.CHANNEL_SUM_WIDE[dtype]]:
            d = R.make_channel_sum(npix, rows, C, dtype)
            assert torch.equal(d["partial"].double().sum(0), d["x"].double().sum(0))
    for rows in R.COLSUM_ROWS:
        for C in R.COLSUM_C:
            for acc in (0, 1):
                R.make_colsum(rows, C, dtype, acc)
    for npix, C in R.ADD_RELU_CASES:
        d = R.make_bn_add_relu(npix, C, dtype)
        assert not torch.signbit(d["out"].float()).any() and (d["out"].float() == 0).any()
    for npix in R.BWD_NPIX:
        for C in R.BWD_C:
            for rows in R.BWD_ROWS:
                R.case_bwd_reduce(npix, rows, C, dtype)
                R.case_bwd_apply_add(npix, rows, C, dtype)
            for kind in R.BWD_APPLY_KINDS:
                R.case_bwd_apply(kind, npix, C, dtype)
    R.case_chain(dtype)
    for c in R.POOL_CASES:
        for acc in (0, 1):
            d = R.case_maxpool(*c, dtype, acc)
            assert torch.signbit(d["y"].float()[d["y"].float() == 0]).any() or c[1] * c[2] == 4
    for c in R.CONV_FIRST_CASES + ([R.CONV_FIRST_F32_ONLY] if dtype == R.F32 else []):
        R.case_conv_first(c, dtype)
    if dtype == R.BF16:
        R.case_conv_first(R.CONV_FIRST_CASES[1], dtype, big=True)
    for img in R.IMAGES:
        for extra in (0, 1):
            R.case_im2col(img, extra, dtype)
    for c in R.WGRAD_CASES:
        for acc in (0, 1):
            R.case_wgrad(c, dtype, acc)


def test_gpu_reducer_cases_are_exactly_computable():
    for rows in R.REDUCE_ROWS:
        for K, C in R.REDUCE_KC:
            d = R.make_reduce_rows(rows, K, C)
            for _, acc, alpha in R.REDUCE_VARIANTS:
                R.reduce_rows(d["partial"], C, d["prior_dgamma"], d["prior_dbeta"], acc, alpha)
    for C in R.BATCHED_C:
        for acc in (0, 1):
            R.make_reduce_rows_batched(C, acc)
    for rows, C, count in R.FINALIZE_CASES:
        d = R.make_bn_finalize(rows, C, count)
        ref = R.bn_finalize(d["partial"], C, count, d["gamma"], d["beta"], d["rmean"], d["rvar"], R.MOMENTUM, R.EPS, True)
        assert float(ref["rstd"][0][0]) == pytest.approx(float(torch.tensor(R.EPS, dtype=torch.float32)) ** -0.5)     # channel 0: the clamp
        assert bool((ref["rstd"][0][1:] < 10).all())                                                              # the others: var > 0


def test_ties_are_exercised():
    """the share of bf16 results that are exact rounding ties, and of pool windows with tied maxima"""
    d, _, dz = R.case_bwd_apply("apply", 1073, 24, R.BF16)
    _, ref, _ = R.bn_bwd_apply(d, R.BF16)
    lo = ref.float().to(R.BF16).double()
    tie = (ref - lo).abs() == R.half_ulp(ref, R.BF16)
    assert float(tie.double().mean()) > 0.02, float(tie.double().mean())
    p = R.make_maxpool(2, 6, 10, 24, R.BF16)
    taps = torch.stack(R._taps(p["x"].double()))
    assert float(((taps == taps.max(0).values).sum(0) > 1).double().mean()) > 0.25
