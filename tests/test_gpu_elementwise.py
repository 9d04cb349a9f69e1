"""Every exported kernel of csrc/elementwise.hip against the float64 oracles of tests/elementwise_ref.py, bit for bit: the inputs are
small integers and powers of two on which the kernels' fp32 evaluation is exact whatever the summation order (the oracles assert
that precondition; tests/test_elementwise_ref_cpu.py runs them for every case here without a GPU).  Every output lives between guard
words and starts as NaN (or, where the call accumulates, as integers); read-only inputs are compared with their host copies after
the call; inputs go up as host tensors, bf16 as raw bits, so the layout helpers are used only by their own test.  The few results
that are not dyadic (BatchNorm finalize, gaussian "real data" cases, the squares row of a rounding conv) are held to the bound the
oracle derives from the kernel's operation count; the test prints error / bound."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import elementwise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
IDS = R.DTYPE_IDS
GUARD = 64
NAN = float("nan")


def _env():
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import DT, stream_ptr
    return _lib.load(), _lib, DT, stream_ptr()


def _run(name, *args):
    """lib.<name>(*args, stream), checked and synchronised"""
    lib, _lib, _, st = _env()
    _lib.check(getattr(lib, name)(*args, st), name)
    torch.cuda.synchronize()


def _bits(t):
    t = t.contiguous()
    return t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _up(t):
    """a host tensor on the device, bit for bit"""
    t = t.contiguous()
    return _bits(t).cuda().view(t.dtype)


def _guarded(shape, dtype, init=NAN):
    """a device tensor of `shape` between GUARD sentinel elements on either side, filled with `init` (a number or a host tensor,
    copied bit for bit) -> (view, check)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device="cuda")
    view = flat[GUARD:GUARD + n].view(shape)
    if isinstance(init, torch.Tensor):
        view.copy_(_up(init.to(dtype)).view(shape))
    else:
        view.fill_(init)

    def check():
        assert (flat[:GUARD] == 77).all() and (flat[GUARD + n:] == 77).all(), "write outside the tensor"
    return view, check


def _same(got, want):
    """bit equality of a device tensor with the host expectation (-0.0 and +0.0 differ, NaN equals the same NaN)"""
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{bad.shape[0]} of {got.numel()} elements differ; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def _within(name, got, ref, bound):
    r = R.ratio(got.cpu(), ref, bound)
    print(f"RATIO {name} {r:.4f}")
    assert r <= 1.0, f"{name}: error / bound = {r}"


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------------------------------------
# layout helpers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.LAYOUT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_layout_helpers(case, dtype):
    _, _, DT, _ = _env()
    B, Cc, HW = case
    d = R.case_layout(B, Cc, HW, dtype)
    x = _up(d["x"])
    y, c0 = _guarded((B, HW, Cc), dtype)
    _run("ksmi_nchw_to_nhwc", x.data_ptr(), y.data_ptr(), B, Cc, HW, DT[dtype])
    c0()
    _same(y, d["nhwc"])
    _same(x, d["x"])
    src = _up(d["nhwc"])
    back, c1 = _guarded((B, Cc, HW), F32)
    _run("ksmi_nhwc_to_nchw", src.data_ptr(), back.data_ptr(), B, Cc, HW, DT[dtype])
    c1()
    _same(back, d["back"])
    _same(src, d["nhwc"])


# ------------------------------------------------------------------------------------------------------------------------------
# channel_sum / colsum
# ------------------------------------------------------------------------------------------------------------------------------
def _channel_sum(npix, rows, Cc, dtype):
    _, _, DT, _ = _env()
    d = R.make_channel_sum(npix, rows, Cc, dtype)
    x = _up(d["x"])
    partial, chk = _guarded((rows, Cc), F32)
    _run("ksmi_channel_sum", x.data_ptr(), partial.data_ptr(), rows, npix, Cc, DT[dtype])
    chk()
    _same(partial, d["partial"])
    _same(x, d["x"])
    assert torch.equal(partial.cpu().double().sum(0), d["x"].double().sum(0))      # the rows total the column sum


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc", R.CHANNEL_SUM_C)
@pytest.mark.parametrize("shape", R.CHANNEL_SUM_SHAPES, ids=lambda s: f"{s[0]}px{s[1]}rows")
def test_channel_sum(shape, Cc, dtype):
    _channel_sum(shape[0], shape[1], Cc, dtype)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", R.CHANNEL_SUM_SHAPES, ids=lambda s: f"{s[0]}px{s[1]}rows")
def test_channel_sum_wide(shape, dtype):
    _channel_sum(shape[0], shape[1], R.CHANNEL_SUM_WIDE[dtype], dtype)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("Cc", R.COLSUM_C)
@pytest.mark.parametrize("rows", R.COLSUM_ROWS)
def test_colsum(rows, Cc, accumulate, dtype):
    _, _, DT, _ = _env()
    d = R.make_colsum(rows, Cc, dtype, accumulate)
    x = _up(d["x"])
    out, chk = _guarded((Cc,), F32, d["prior"] if accumulate else NAN)
    _run("ksmi_colsum", x.data_ptr(), rows, Cc, out.data_ptr(), accumulate, DT[dtype])
    chk()
    _same(out, d["out"])
    _same(x, d["x"])


# ------------------------------------------------------------------------------------------------------------------------------
# row reducers
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("KC", R.REDUCE_KC, ids=lambda kc: f"K{kc[0]}C{kc[1]}")
@pytest.mark.parametrize("rows", R.REDUCE_ROWS)
def test_reduce_rows(rows, KC):
    K, Cc = KC
    d = R.make_reduce_rows(rows, K, Cc)
    for given, accumulate, alpha in R.REDUCE_VARIANTS:
        want = R.reduce_rows(d["partial"], Cc, d["prior_dgamma"], d["prior_dbeta"], accumulate, alpha)
        partial, c0 = _guarded(d["partial"].shape, F32, d["partial"])            # a scratch copy: a fold writes rows 0..31 in place
        sums, c1 = _guarded((K, Cc), F32)
        dgamma, c2 = _guarded((Cc,), F32, d["prior_dgamma"] if accumulate else NAN)
        dbeta, c3 = _guarded((Cc,), F32, d["prior_dbeta"] if accumulate else NAN)
        before = [t.cpu().clone() for t in (sums, dgamma, dbeta)]
        ptrs = [_ptr(t) if g else None for t, g in zip((sums, dgamma, dbeta), given)]
        if alpha == 1.0:
            _run("ksmi_reduce_rows", partial.data_ptr(), rows, K, d["Cstride"], Cc, *ptrs, accumulate)
        else:
            _run("ksmi_reduce_rows_scaled", partial.data_ptr(), rows, K, d["Cstride"], Cc, *ptrs, accumulate, alpha)
        for c in (c0, c1, c2, c3):
            c()
        _same(sums, want["sums"] if given[0] else before[0])                    # unscaled whatever alpha is
        _same(dgamma, want["dgamma"] if given[1] and K > 1 else before[1])
        _same(dbeta, want["dbeta"] if given[2] else before[2])
        _same(partial, want["partial_after"])                                   # rows >= 32 and the padding columns untouched


def _desc_table(ents, parts, dst):
    _, _lib, _, _ = _env()
    arr = (_lib.RowsumDesc * len(ents))()
    for r, e, p in zip(arr, ents, parts):
        r.partial = _ptr(p)
        r.dst = dst[e["dst"]].data_ptr()
        r.rows, r.K, r.k, r.Cstride, r.C = e["rows"], e["K"], e["k"], e["Cstride"], e["C"]
        r.accumulate, r.head, r.next = e["accumulate"], e["head"], e["next"]
    raw = bytes(C.string_at(C.addressof(arr), C.sizeof(arr)))
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("Cc", R.BATCHED_C)
def test_reduce_rows_batched(Cc, accumulate):
    d = R.make_reduce_rows_batched(Cc, accumulate)
    ents = d["entries"]
    parts = [None if e["partial"] is None else _up(e["partial"]) for e in ents]
    dst, chk = _guarded(d["init"].shape, F32, d["init"])                       # rows of non-head entries: NaN, and they must stay NaN
    table = _desc_table(ents, parts, dst)
    if Cc > 512:
        _run("ksmi_reduce_rows_batched_wide", table.data_ptr(), len(ents), Cc)
    else:
        _run("ksmi_reduce_rows_batched", table.data_ptr(), len(ents))
    chk()
    _same(dst, d["dst"])
    for p, e in zip(parts, ents):
        if p is not None:
            _same(p, e["partial"])


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm finalize
# ------------------------------------------------------------------------------------------------------------------------------
def _finalize(rows, Cc, count, training, with_nbt=True):
    d = R.make_bn_finalize(rows, Cc, count)
    ref = R.bn_finalize(d["partial"], Cc, count, d["gamma"], d["beta"], d["rmean"], d["rvar"], R.MOMENTUM, R.EPS, training)
    partial, c0 = _guarded(d["partial"].shape, F32, d["partial"])
    gamma, beta = _up(d["gamma"]), _up(d["beta"])
    rmean, c1 = _guarded((Cc,), F32, d["rmean"])
    rvar, c2 = _guarded((Cc,), F32, d["rvar"])
    nbt, c3 = _guarded((1,), torch.int64, d["nbt"])
    outs = {k: _guarded((Cc,), F32) for k in ("mean", "rstd", "scale", "shift")}
    _run("ksmi_bn_finalize", partial.data_ptr() if training else None, rows if training else 0, d["Cpad"], Cc, count, gamma.data_ptr(),
         beta.data_ptr(), rmean.data_ptr(), rvar.data_ptr(), nbt.data_ptr() if with_nbt else None, R.MOMENTUM, R.EPS, int(training),
         *[outs[k][0].data_ptr() for k in ("mean", "rstd", "scale", "shift")])
    for c in (c0, c1, c2, c3) + tuple(v[1] for v in outs.values()):
        c()
    assert int(nbt) == d["nbt"] + (1 if training and with_nbt else 0)
    _same(gamma, d["gamma"])
    _same(beta, d["beta"])
    got = {k: v[0] for k, v in outs.items()}
    got.update(rmean=rmean, rvar=rvar)
    worst = 0.0
    for k, (want, bound) in ref.items():
        if bound is None:
            _same(got[k], R.exact_f32(want, k).float())
        else:
            assert torch.isfinite(got[k]).all()
            worst = max(worst, R.ratio(got[k].cpu(), want, bound))
    print(f"RATIO bn_finalize training={int(training)} rows={rows} {worst:.4f}")
    assert worst <= 1.0, worst
    if training:                                                                # more than 256 rows fold into rows 0..31; nothing else is written
        _same(partial, R.folded(d["partial"], Cc))
    return got


@pytest.mark.parametrize("case", R.FINALIZE_CASES, ids=lambda c: f"{c[0]}rows{c[1]}ch_n{int(c[2])}")
def test_bn_finalize_training(case):
    rows, Cc, count = case
    got = _finalize(rows, Cc, count, True)
    assert abs(float(got["rstd"][0]) - R.EPS ** -0.5) < 1e-3                    # channel 0: q = 0, s != 0 -> the variance is clamped to 0


def test_bn_finalize_without_step_counter():
    _finalize(70, 16, 4096.0, True, with_nbt=False)


def test_bn_finalize_eval_reads_the_running_statistics():
    _finalize(1, 33, 64.0, False)


# ------------------------------------------------------------------------------------------------------------------------------
# bn_add_relu
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("case", R.ADD_RELU_CASES, ids=lambda c: f"{c[0]}px{c[1]}ch")
def test_bn_add_relu(case, dtype):
    _, _, DT, _ = _env()
    npix, Cc = case
    d = R.make_bn_add_relu(npix, Cc, dtype)
    z, idn, scale, shift = (_up(d[k]) for k in ("z", "idn", "scale", "shift"))
    out, chk = _guarded((npix, Cc), dtype)
    _run("ksmi_bn_add_relu", z.data_ptr(), idn.data_ptr(), scale.data_ptr(), shift.data_ptr(), out.data_ptr(), npix, Cc, DT[dtype])
    chk()
    _same(out, d["out"])
    for t, k in ((z, "z"), (idn, "idn"), (scale, "scale"), (shift, "shift")):
        _same(t, d[k])


# ------------------------------------------------------------------------------------------------------------------------------
# BatchNorm + ReLU backward
# ------------------------------------------------------------------------------------------------------------------------------
PARAMS = ("mean", "rstd", "gamma", "sums")


def _bwd_upload(d):
    return {k: _up(v) for k, v in d.items() if isinstance(v, torch.Tensor)}


def _bwd_unchanged(dev, d, keys):
    for k in keys:
        _same(dev[k], d[k])


def _call_reduce(dev, partial, rows, npix, Cc, dtype):
    _, _, DT, _ = _env()
    _run("ksmi_bnrelu_bwd_reduce", dev["dout"].data_ptr(), dev["out"].data_ptr(), dev["z"].data_ptr(), dev["mean"].data_ptr(),
         dev["rstd"].data_ptr(), partial.data_ptr(), rows, npix, Cc, DT[dtype])


def _call_apply(kind, dev, dz, count, npix, Cc, dtype, sums=None):
    _, _, DT, _ = _env()
    sums = dev["sums"] if sums is None else sums
    head = (dev["dout"].data_ptr(), dev["out"].data_ptr(), dev["z"].data_ptr(), dev["mean"].data_ptr(), dev["rstd"].data_ptr(),
            dev["gamma"].data_ptr(), sums.data_ptr(), dz.data_ptr(), count, npix, Cc)
    if kind == "apply":
        _run("ksmi_bnrelu_bwd_apply", *head, DT[dtype])
    elif kind == "scaled":
        _run("ksmi_bnrelu_bwd_apply_scaled", *head, 0.5, DT[dtype])
    else:
        _run("ksmi_bn_bwd_apply_gated", dev["dout"].data_ptr(), *head[2:], DT[dtype])


def _call_apply_add(dev, partial, rows, count, npix, Cc, dtype):
    _, _, DT, _ = _env()
    _run("ksmi_bn_bwd_apply_add", dev["r"].data_ptr(), dev["dout"].data_ptr(), dev["z"].data_ptr(), dev["mean"].data_ptr(),
         dev["rstd"].data_ptr(), dev["gamma"].data_ptr(), dev["sums"].data_ptr(), partial.data_ptr(), rows, count, npix, Cc, DT[dtype])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc", R.BWD_C)
@pytest.mark.parametrize("rows", R.BWD_ROWS)
@pytest.mark.parametrize("npix", R.BWD_NPIX)
def test_bnrelu_bwd_reduce(npix, rows, Cc, dtype):
    d, want = R.case_bwd_reduce(npix, rows, Cc, dtype)
    dev = _bwd_upload(d)
    partial, chk = _guarded((rows, 2, Cc), F32)
    _call_reduce(dev, partial, rows, npix, Cc, dtype)
    chk()
    _same(partial, want)
    _bwd_unchanged(dev, d, ("dout", "out", "z", "mean", "rstd"))


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc", R.BWD_C)
@pytest.mark.parametrize("npix", R.BWD_NPIX)
@pytest.mark.parametrize("kind", R.BWD_APPLY_KINDS)
def test_bn_bwd_apply(kind, npix, Cc, dtype):
    d, want_g, want_dz = R.case_bwd_apply(kind, npix, Cc, dtype)
    dev = _bwd_upload(d)
    dev["dout"], c0 = _guarded((npix, Cc), dtype, d["dout"])                    # rewritten in place to the gated gradient (not by _gated)
    dz, c1 = _guarded((npix, Cc), dtype)
    _call_apply(kind, dev, dz, d["count"], npix, Cc, dtype)
    c0(), c1()
    _same(dz, want_dz)
    _same(dev["dout"], want_g)
    if kind == "gated":
        _same(dev["dout"], d["dout"])
    _bwd_unchanged(dev, d, ("out", "z") + PARAMS)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("Cc", R.BWD_C)
@pytest.mark.parametrize("rows", R.BWD_ROWS)
@pytest.mark.parametrize("npix", R.BWD_NPIX)
def test_bn_bwd_apply_add(npix, rows, Cc, dtype):
    d, want_di, want_partial = R.case_bwd_apply_add(npix, rows, Cc, dtype)
    dev = _bwd_upload(d)
    dev["r"], c0 = _guarded((npix, Cc), dtype, d["r"])
    partial, c1 = _guarded((rows, Cc), F32)
    _call_apply_add(dev, partial, rows, d["count"], npix, Cc, dtype)
    c0(), c1()
    _same(dev["r"], want_di)
    _same(partial, want_partial)
    _bwd_unchanged(dev, d, ("dout", "z") + PARAMS)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_bn_bwd_chain(dtype):
    """reduce -> reduce_rows -> apply, each fed the previous kernel's own output"""
    npix, Cc, rows = R.CHAIN_NPIX, R.CHAIN_C, R.CHAIN_ROWS
    d, want_partial, want_sums, want_g, want_dz = R.case_chain(dtype)
    dev = _bwd_upload(d)
    dev["dout"], c0 = _guarded((npix, Cc), dtype, d["dout"])
    partial, c1 = _guarded((rows, 2, Cc), F32)
    sums, c2 = _guarded((2, Cc), F32)
    dz, c3 = _guarded((npix, Cc), dtype)
    _call_reduce(dev, partial, rows, npix, Cc, dtype)
    _run("ksmi_reduce_rows", partial.data_ptr(), rows, 2, Cc, Cc, sums.data_ptr(), None, None, 0)
    _call_apply("apply", dev, dz, d["count"], npix, Cc, dtype, sums=sums)
    for c in (c0, c1, c2, c3):
        c()
    _same(partial, want_partial)
    _same(sums, want_sums)
    _same(dev["dout"], want_g)
    _same(dz, want_dz)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_bn_bwd_real_data(dtype):
    """gaussian inputs at 1073 pixels x 24 channels: the exact cases are not special.  Bounds from the operation counts (see the oracle)"""
    npix, Cc, rows = R.REAL_NPIX, R.REAL_C, R.REAL_ROWS
    d = R.make_bn_bwd(npix, Cc, dtype, seed=300, real=True)
    name = IDS[R.DTYPES.index(dtype)]
    # reduce: z - mean, * g, * rstd = 3 roundings per term, then the accumulation chain
    dev = _bwd_upload(d)
    partial, chk = _guarded((rows, 2, Cc), F32)
    _call_reduce(dev, partial, rows, npix, Cc, dtype)
    chk()
    ref, mag = R.bnrelu_bwd_reduce(d, rows, exact=False)
    n = 3 + R.reduce_chain(npix, rows, Cc, dtype)
    _within(f"bnrelu_bwd_reduce {name}", partial, ref, R.half_ulp(ref, F32) + n * R.U * mag)
    for kind in R.BWD_APPLY_KINDS:
        dev = _bwd_upload(d)
        dev["dout"], c0 = _guarded((npix, Cc), dtype, d["dout"])
        dz, c1 = _guarded((npix, Cc), dtype)
        _call_apply(kind, dev, dz, d["count"], npix, Cc, dtype)
        c0(), c1()
        g, ref, mag = R.bn_bwd_apply(d, dtype, alpha=0.5 if kind == "scaled" else 1.0, gate=kind != "gated", exact=False)
        _same(dev["dout"], g)                                                   # the gate is exact on any data
        # (bf16: the last fp32 product is one more rounding before the store's)
        n = R.N_APPLY[kind] + (1 if dtype == BF16 else 0)
        _within(f"bn_bwd_apply[{kind}] {name}", dz, ref, R.half_ulp(ref, dtype) + n * R.U * mag)
    dev = _bwd_upload(d)
    dev["r"], c0 = _guarded((npix, Cc), dtype, d["r"])
    partial, c1 = _guarded((rows, Cc), F32)
    _call_apply_add(dev, partial, rows, d["count"], npix, Cc, dtype)
    c0(), c1()
    ref, mag = R.bn_bwd_apply_add(d, rows, dtype, exact=False)
    n = R.N_APPLY_ADD + (1 if dtype == BF16 else 0)
    _within(f"bn_bwd_apply_add {name}", dev["r"], ref, R.half_ulp(ref, dtype) + n * R.U * mag)
    # the bias partial sums what the kernel stored: the accumulation chain only
    ref, mag = R.bias_partial(dev["r"].cpu(), rows, exact=False)
    _within(f"bn_bwd_apply_add partial {name}", partial, ref, R.half_ulp(ref, F32) + R.reduce_chain(npix, rows, Cc, dtype) * R.U * mag)


# ------------------------------------------------------------------------------------------------------------------------------
# 2x2 max-pool
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", R.POOL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_maxpool2x2(case, accumulate, dtype):
    _, _, DT, _ = _env()
    B, H, W, Cc = case
    d = R.case_maxpool(B, H, W, Cc, dtype, accumulate)
    x, dy = _up(d["x"]), _up(d["dy"])
    y, c0 = _guarded((B, H // 2, W // 2, Cc), dtype)
    dx, c1 = _guarded((B, H, W, Cc), dtype, d["prior"] if accumulate else NAN)  # accumulate = 0 never reads the destination
    _run("ksmi_maxpool2x2_forward", x.data_ptr(), y.data_ptr(), B, H, W, Cc, DT[dtype])
    _run("ksmi_maxpool2x2_backward", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), accumulate, B, H, W, Cc, DT[dtype])
    c0(), c1()
    _same(y, d["y"])
    _same(dx, d["dx"])
    _same(x, d["x"])
    _same(dy, d["dy"])


# ------------------------------------------------------------------------------------------------------------------------------
# first-layer conv, im2col, weight gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _conv_first(case, dtype, with_stats, big=False, split=False):
    lib, _, DT, _ = _env()
    B, Cin, H, W, Cout = case
    d = R.case_conv_first(case, dtype, big=big)
    w, bias = _up(d["w"]), _up(d["bias"])
    out, c0 = _guarded((B, H, W, Cout), dtype)
    nrows = lib.ksmi_conv_first_stats_rows(B, H, W)
    assert nrows == d["stats"].shape[0]
    stats, c1 = _guarded((nrows, 2, Cout), F32)
    sp = stats.data_ptr() if with_stats else None
    if split:                                                                   # channels [0, 2) from x, the rest from the tail image
        head, tail = _up(d["x"][:, :2]), _up(d["x"][:, 2:])
        _run("ksmi_conv_first_forward_raw", head.data_ptr(), tail.data_ptr(), 2, w.data_ptr(), bias.data_ptr(), out.data_ptr(), sp, B, Cin, H, W,
             Cout, None, None, None, DT[dtype])
        _same(head, d["x"][:, :2].contiguous())
        _same(tail, d["x"][:, 2:].contiguous())
    else:
        x = _up(d["x"])
        _run("ksmi_conv_first_forward", x.data_ptr(), w.data_ptr(), bias.data_ptr(), out.data_ptr(), sp, B, Cin, H, W, Cout, DT[dtype])
        _same(x, d["x"])
    c0(), c1()
    _same(out, d["out"])
    _same(w, d["w"])
    _same(bias, d["bias"])
    if not with_stats:
        assert torch.isnan(stats).all()
    elif not big:
        _same(stats, R.exact_f32(d["stats"], "stats").float())
    else:
        _same(stats[:, 0], R.exact_f32(d["stats"][:, 0], "sum row").float())
        ref, mag = d["stats"][:, 1], d["stats_mag"][:, 1]
        _within("conv_first squares row", stats[:, 1], ref, R.half_ulp(ref, F32) + R.N_STATS_SQ * R.U * mag)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("with_stats", [0, 1])
@pytest.mark.parametrize("case", R.CONV_FIRST_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_first_forward(case, with_stats, dtype):
    _conv_first(case, dtype, with_stats)


def test_conv_first_forward_pass_of_four_channels():
    _conv_first(R.CONV_FIRST_F32_ONLY, F32, 1)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
def test_conv_first_forward_raw_channel_split(dtype):
    _conv_first(R.CONV_FIRST_CASES[1], dtype, 1, split=True)


def test_conv_first_forward_rounds_once():
    """outputs beyond 256 are rounded to bf16: the output bits and the sum row are exact, the squares row within its derived bound"""
    _conv_first(R.CONV_FIRST_CASES[1], BF16, 1, big=True)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("image", R.IMAGES, ids=lambda c: "x".join(map(str, c)))
def test_im2col3x3(image, extra, dtype):
    _, _, DT, _ = _env()
    B, Cin, H, W = image
    d = R.case_im2col(image, extra, dtype)
    x = _up(d["x"])
    out, chk = _guarded((B, H, W, d["Kpad"]), dtype)
    _run("ksmi_im2col3x3", x.data_ptr(), out.data_ptr(), B, Cin, H, W, d["Kpad"], DT[dtype])
    chk()
    _same(out, d["out"])
    assert not out[..., Cin * 9:].float().any()
    _same(x, d["x"])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=IDS)
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", R.WGRAD_CASES, ids=lambda c: "x".join(map(str, c)))
def test_conv_first_wgrad(case, accumulate, dtype):
    lib, _, DT, _ = _env()
    B, Cin, H, W, Cout = case
    d = R.case_wgrad(case, dtype, accumulate)
    x, dy = _up(d["x"]), _up(d["dy"])
    ws_bytes = lib.ksmi_conv_first_wgrad_workspace(B, Cin, H, W, Cout)
    patches = B * ((H + 15) // 16) * ((W + 15) // 16)
    assert ws_bytes == min(patches, 512) * Cout * Cin * 9 * 4
    ws, c0 = _guarded((ws_bytes // 4,), F32)
    dw, c1 = _guarded((Cout, Cin, 3, 3), F32, d["prior"] if accumulate else NAN)
    _run("ksmi_conv_first_wgrad", x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws.data_ptr(), ws_bytes, B, Cin, H, W, Cout, accumulate, DT[dtype])
    c0(), c1()
    _same(dw, d["dw"])
    _same(x, d["x"])
    _same(dy, d["dy"])


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: the launcher returns an error code before any launch
# ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib, _, DT, st = _env()
    t = torch.zeros(1 << 16, dtype=F32, device="cuda")
    p, bf, f32 = t.data_ptr(), DT[BF16], DT[F32]
    before = t.clone()
    refused = {
        # C not a multiple of the 16-byte vector
        "bn_add_relu C % 8": lib.ksmi_bn_add_relu(p, p, p, p, p, 4, 12, bf, st),
        "bn_add_relu C % 4": lib.ksmi_bn_add_relu(p, p, p, p, p, 4, 6, f32, st),
        "channel_sum C % 8": lib.ksmi_channel_sum(p, p, 1, 4, 12, bf, st),
        "colsum C % 4": lib.ksmi_colsum(p, 4, 6, p, 0, f32, st),
        "maxpool C % 8": lib.ksmi_maxpool2x2_forward(p, p, 1, 2, 2, 4, bf, st),
        "bnrelu_bwd_reduce C % 8": lib.ksmi_bnrelu_bwd_reduce(p, p, p, p, p, p, 1, 4, 12, bf, st),
        "conv_first Cout % 8": lib.ksmi_conv_first_forward(p, p, p, p, None, 1, 1, 4, 4, 12, bf, st),
        "im2col Kpad % 8": lib.ksmi_im2col3x3(p, p, 1, 1, 4, 4, 12, bf, st),
        # C / VEC > 128 for the kernels that walk channels with 256 threads
        "bn_add_relu wide": lib.ksmi_bn_add_relu(p, p, p, p, p, 1, 1032, bf, st),
        "bnrelu_bwd_reduce wide": lib.ksmi_bnrelu_bwd_reduce(p, p, p, p, p, p, 1, 1, 516, f32, st),
        "bnrelu_bwd_apply wide": lib.ksmi_bnrelu_bwd_apply(p, p, p, p, p, p, p, p, 1.0, 1, 516, f32, st),
        "bn_bwd_apply_gated wide": lib.ksmi_bn_bwd_apply_gated(p, p, p, p, p, p, p, 1.0, 1, 516, f32, st),
        "bn_bwd_apply_add wide": lib.ksmi_bn_bwd_apply_add(p, p, p, p, p, p, p, p, 1, 1.0, 1, 516, f32, st),
        "maxpool wide": lib.ksmi_maxpool2x2_backward(p, p, p, 0, 1, 2, 2, 1032, bf, st),
        # rows < 1
        "channel_sum rows": lib.ksmi_channel_sum(p, p, 0, 4, 8, bf, st),
        "colsum rows": lib.ksmi_colsum(p, 0, 8, p, 0, bf, st),
        "reduce_rows rows": lib.ksmi_reduce_rows(p, 0, 2, 8, 8, p, None, None, 0, st),
        "bnrelu_bwd_reduce rows": lib.ksmi_bnrelu_bwd_reduce(p, p, p, p, p, p, 0, 4, 8, bf, st),
        "bn_bwd_apply_add rows": lib.ksmi_bn_bwd_apply_add(p, p, p, p, p, p, p, p, 0, 1.0, 4, 8, bf, st),
        "bn_finalize rows": lib.ksmi_bn_finalize(p, 0, 8, 8, 4.0, p, p, p, p, None, 0.1, 1e-5, 1, p, p, p, p, st),
        "bn_finalize partial": lib.ksmi_bn_finalize(None, 1, 8, 8, 4.0, p, p, p, p, None, 0.1, 1e-5, 1, p, p, p, p, st),
        "reduce_rows_batched n": lib.ksmi_reduce_rows_batched(p, 0, st),
        "reduce_rows_batched_wide max_c": lib.ksmi_reduce_rows_batched_wide(p, 1, 0, st),
        # Cstride < C
        "reduce_rows Cstride": lib.ksmi_reduce_rows_scaled(p, 4, 2, 7, 8, p, None, None, 0, 1.0, st),
        # dtype
        "bn_add_relu dtype": lib.ksmi_bn_add_relu(p, p, p, p, p, 4, 8, 7, st),
        "nchw_to_nhwc dtype": lib.ksmi_nchw_to_nhwc(p, p, 1, 8, 4, 7, st),
        "nhwc_to_nchw dtype": lib.ksmi_nhwc_to_nchw(p, p, 1, 8, 4, 7, st),
        "conv_first dtype": lib.ksmi_conv_first_forward(p, p, p, p, None, 1, 1, 4, 4, 8, 7, st),
        # odd H or W
        "maxpool odd H": lib.ksmi_maxpool2x2_forward(p, p, 1, 3, 2, 8, bf, st),
        "maxpool odd W": lib.ksmi_maxpool2x2_backward(p, p, p, 0, 1, 2, 3, 8, bf, st),
        # first layer: Cin = 9, Cout = 48 for the weight gradient, a workspace one byte short, a tail image without a head
        "conv_first Cin": lib.ksmi_conv_first_forward(p, p, p, p, None, 1, 9, 4, 4, 8, bf, st),
        "conv_first_wgrad Cin": lib.ksmi_conv_first_wgrad(p, p, p, p, 1 << 18, 1, 9, 4, 4, 8, 0, bf, st),
        "conv_first_wgrad Cout": lib.ksmi_conv_first_wgrad(p, p, p, p, 1 << 18, 1, 2, 4, 4, 48, 0, bf, st),
        "conv_first_wgrad workspace": lib.ksmi_conv_first_wgrad(p, p, p, p, lib.ksmi_conv_first_wgrad_workspace(1, 2, 4, 4, 8) - 1, 1, 2, 4, 4, 8,
                                                                0, bf, st),
        "conv_first_raw c_head": lib.ksmi_conv_first_forward_raw(p, p, 3, p, p, p, None, 1, 3, 4, 4, 8, None, None, None, bf, st),
        "im2col Kpad < Cin * 9": lib.ksmi_im2col3x3(p, p, 1, 2, 4, 4, 16, bf, st),
    }
    torch.cuda.synchronize()
    accepted = [k for k, rc in refused.items() if rc == 0]
    assert not accepted, accepted
    assert torch.equal(t, before)                                               # nothing was launched
