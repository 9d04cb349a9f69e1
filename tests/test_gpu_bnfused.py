"""The four fused BatchNorm passes of csrc/bnfused.hip against the float64 oracles of tests/bnfused_ref.py (compositions of those of
tests/elementwise_ref.py), bit for bit: statistics rows, parameters and activations are small integers and powers of two on which the
finish (fp64 row sums, mean, variance, rstd with eps = 1, scale, shift, running mean) and the streaming arithmetic are exact whatever the
summation order and whether or not a multiply-add is contracted.  The oracles assert that precondition; tests/test_bnfused_ref_cpu.py
builds every case here without a GPU.  The conventions are those of tests/test_gpu_elementwise.py: every output lives between guard
words and starts as NaN (integers where the call accumulates), inputs go up bit for bit and read-only ones are compared with their host
copies after the call, comparisons go through _same and _within.  What is not dyadic (the running variance where var * 64 / 63 is not,
and the gaussian cases) is held to the bound the oracle derives from the kernel's operation count; the test prints error / bound.  On
the gaussian cases every fused call is also compared, bit for bit, with the launch sequence it replaces."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bnfused_ref as N  # noqa: E402
import elementwise_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
NAN = float("nan")
STATS = ("mean", "rstd", "scale", "shift")


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
# callers: one per launcher.  Each uploads the inputs of a case, runs the call on guarded outputs, checks the guards and the read-only
# inputs, and returns the device outputs
# ------------------------------------------------------------------------------------------------------------------------------
def _forward(d, B, H, W, Cc, dtype, pooled, momentum=N.MOMENTUM, eps=N.EPS, with_nbt=True):
    _, _, DT, _ = _env()
    npix, rows = B * H * W, d["partial"].shape[0]
    partial, c0 = _guarded(d["partial"].shape, F32, d["partial"])              # a scratch copy: a fold writes rows 0..31 in place
    ro = {k: _up(d[k]) for k in ("gamma", "beta", "z", "idn")}
    rmean, c1 = _guarded((Cc,), F32, d["rmean"])
    rvar, c2 = _guarded((Cc,), F32, d["rvar"])
    nbt, c3 = _guarded((1,), torch.int64, d["nbt"])
    outs = {k: _guarded((Cc,), F32) for k in STATS}
    out, c4 = _guarded((npix, Cc), dtype)
    y, c5 = _guarded((B, H // 2, W // 2, Cc), dtype)
    _run("ksmi_bn_fin_add_relu", partial.data_ptr(), rows, d["Cstride"], Cc, d["count"], ro["gamma"].data_ptr(), ro["beta"].data_ptr(),
         rmean.data_ptr(), rvar.data_ptr(), nbt.data_ptr() if with_nbt else None, momentum, eps, *[outs[k][0].data_ptr() for k in STATS],
         ro["z"].data_ptr(), ro["idn"].data_ptr(), out.data_ptr(), y.data_ptr() if pooled else None, B, H, W, DT[dtype])
    for c in (c0, c1, c2, c3, c4, c5) + tuple(v[1] for v in outs.values()):
        c()
    for k, t in ro.items():
        _same(t, d[k])
    assert int(nbt) == d["nbt"] + (1 if with_nbt else 0)
    if not pooled:
        assert torch.isnan(y.float()).all()
    got = {k: v[0] for k, v in outs.items()}
    got.update(rmean=rmean, rvar=rvar, out=out, pooled=y, partial=partial)
    return got


def _check_forward(got, d, Cc, pooled, name):
    """the dyadic expectation: everything bit for bit but the running variance of the channels where var * count / (count - 1) rounds"""
    want = d["want"]
    for k in STATS + ("rmean", "out"):
        _same(got[k], want[k])
    ref, bound, exact = want["rvar"]
    rv = got["rvar"].cpu()
    assert torch.isfinite(rv).all()
    _same(rv[exact], ref[exact].float())
    if not bool(exact.all()):
        _within(f"bn_fin_add_relu running_var {name}", rv[~exact], ref[~exact], bound[~exact])
    if pooled:
        _same(got["pooled"], want["pooled"])
    _same(got["partial"], N.partial_after(d["partial"], Cc))


def _finish_buffers(d, Cc, accumulate):
    """partial (a scratch copy), sums, dgamma, dbeta between guards -> (tensors, checks, their state before the call)"""
    partial, c0 = _guarded(d["partial"].shape, F32, d["partial"])
    sums, c1 = _guarded((2, Cc), F32)
    dgamma, c2 = _guarded((Cc,), F32, d["prior_dgamma"] if accumulate else NAN)
    dbeta, c3 = _guarded((Cc,), F32, d["prior_dbeta"] if accumulate else NAN)
    t = {"partial": partial, "sums": sums, "dgamma": dgamma, "dbeta": dbeta}
    return t, (c0, c1, c2, c3), {k: v.cpu().clone() for k, v in t.items()}


def _backward(kind, d, npix, Cc, dtype, given=(1, 1, 1), accumulate=0, bias_rows=0):
    """kind: "gated" | "relu" | "add" -> the device tensors the call wrote (or might have), the state of the optional ones before"""
    _, _, DT, _ = _env()
    rows = d["partial"].shape[0]
    fin, checks, before = _finish_buffers(d, Cc, accumulate)
    ro_keys = {"gated": ("dout", "z"), "relu": ("out", "z"), "add": ("dout", "z")}[kind] + ("mean", "rstd", "gamma")
    ro = {k: _up(d[k]) for k in ro_keys}
    head = (fin["partial"].data_ptr(), rows, d["Cstride"]) + tuple(_ptr(fin[k]) if g else None for k, g in zip(("sums", "dgamma", "dbeta"), given)) \
        + (accumulate,)
    par = (ro["mean"].data_ptr(), ro["rstd"].data_ptr(), ro["gamma"].data_ptr())
    tail = (d["count"], npix, Cc, DT[dtype])
    got = dict(fin)
    if kind == "add":
        got["r"], c4 = _guarded((npix, Cc), dtype, d["r"])
        got["bias"], c5 = _guarded((bias_rows, Cc), F32)
        _run("ksmi_bn_bwd_fin_apply_add", *head, got["r"].data_ptr(), ro["dout"].data_ptr(), ro["z"].data_ptr(), *par, got["bias"].data_ptr(),
             bias_rows, *tail)
    else:
        got["dz"], c4 = _guarded((npix, Cc), dtype)
        if kind == "relu":
            got["dout"], c5 = _guarded((npix, Cc), dtype, d["dout"])            # rewritten in place to the gated gradient
            _run("ksmi_bnrelu_bwd_fin_apply", *head, got["dout"].data_ptr(), ro["out"].data_ptr(), ro["z"].data_ptr(), *par, got["dz"].data_ptr(),
                 *tail)
        else:
            c5 = lambda: None                                                   # noqa: E731
            _run("ksmi_bn_bwd_fin_apply_gated", *head, ro["dout"].data_ptr(), ro["z"].data_ptr(), *par, got["dz"].data_ptr(), *tail)
    for c in checks + (c4, c5):
        c()
    for k, t in ro.items():
        _same(t, d[k])
    return got, before


def _check_finish(got, before, d, Cc, given, accumulate):
    want = N.bwd_finish(d, Cc, accumulate)
    for k, g in zip(("sums", "dgamma", "dbeta"), given):
        _same(got[k], want[k] if g else before[k])
    _same(got["partial"], want["partial_after"])


# ------------------------------------------------------------------------------------------------------------------------------
# the row sums every pass starts with
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c + (dt,) for c in N.ROWSUM_CASES for dt in N.dtypes_of(c[0])],
                         ids=lambda c: f"C{c[0]}rows{c[1]}-{N.dtype_id(c[2])}")
def test_row_sums(case):
    """through ksmi_bn_bwd_fin_apply_gated on a 7-pixel tensor: the published sums, dgamma and dbeta, the outputs that were not asked
    for, dz (which needs the right sums in every workgroup's LDS), and `partial` afterwards"""
    Cc, rows, dtype = case                                                      # (C = 4 runs in fp32 only: bf16 needs C % 8 == 0)
    npix = N.ROWSUM_NPIX
    for pad, given, accumulate in N.ROWSUM_VARIANTS:
        d, _, want_dz = N.case_bwd_fin_apply("gated", npix, Cc, dtype, rows, pad)
        got, before = _backward("gated", d, npix, Cc, dtype, given, accumulate)
        _check_finish(got, before, d, Cc, given, accumulate)
        _same(got["dz"], want_dz)


@pytest.mark.parametrize("kind", ["relu", "add", "forward"])
@pytest.mark.parametrize("case", N.ROWSUM_SPOT, ids=lambda c: f"C{c[0]}rows{c[1]}")
def test_row_sums_through_the_other_launchers(case, kind):
    Cc, rows = case
    npix = N.ROWSUM_NPIX
    for dtype in N.dtypes_of(Cc):
        if kind == "relu":
            d, want_g, want_dz = N.case_bwd_fin_apply("relu", npix, Cc, dtype, rows, 4)
            got, before = _backward("relu", d, npix, Cc, dtype, (1, 1, 1), 1)
            _check_finish(got, before, d, Cc, (1, 1, 1), 1)
            _same(got["dz"], want_dz)
            _same(got["dout"], want_g)
        elif kind == "add":
            d, want_di, want_bias = N.case_bwd_fin_apply_add(npix, Cc, dtype, rows, 4, bias_rows=(3,))
            got, before = _backward("add", d, npix, Cc, dtype, (1, 1, 1), 1, bias_rows=3)
            _check_finish(got, before, d, Cc, (1, 1, 1), 1)
            _same(got["r"], want_di)
            _same(got["bias"], want_bias[3])
        else:
            d = N.make_fin_add_relu(1, 1, npix, Cc, dtype, 0, rows=rows)
            _check_forward(_forward(d, 1, 1, npix, Cc, dtype, 0), d, Cc, 0, f"rows={rows}")


# ------------------------------------------------------------------------------------------------------------------------------
# the streaming part of ksmi_bn_bwd_fin_apply_gated / ksmi_bnrelu_bwd_fin_apply
# ------------------------------------------------------------------------------------------------------------------------------
def _bwd_fin_apply(mode, npix, Cc, dtype):
    d, want_g, want_dz = N.case_bwd_fin_apply(mode, npix, Cc, dtype, 3, 4)
    got, before = _backward(mode, d, npix, Cc, dtype, (1, 1, 1), 1)
    _check_finish(got, before, d, Cc, (1, 1, 1), 1)
    _same(got["dz"], want_dz)
    if mode == "relu":
        _same(got["dout"], want_g)                                              # gated by out > 0: -0.0 and +0.0 in `out` both give +0.0


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
@pytest.mark.parametrize("Cc", N.BWD_C)
@pytest.mark.parametrize("npix", N.BWD_NPIX)
@pytest.mark.parametrize("mode", N.BWD_MODES)
def test_bn_bwd_fin_apply(mode, npix, Cc, dtype):
    """one vector (1 pixel x 8 channels in bf16), odd vector counts (7 and 3219: a lone last vector), several workgroups (1073 pixels at C >= 24)"""
    _bwd_fin_apply(mode, npix, Cc, dtype)


# ------------------------------------------------------------------------------------------------------------------------------
# ksmi_bn_bwd_fin_apply_add
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
@pytest.mark.parametrize("Cc", N.ADD_C)
@pytest.mark.parametrize("npix", N.BWD_NPIX)
def test_bn_bwd_fin_apply_add(npix, Cc, dtype):
    """r is updated in place; bias_partial holds the slab sums of the values stored, rows of +0.0 for the workgroups whose slab is empty
    (bias_rows > npix, and 256 slabs of 5 pixels over 1073).  fp32, C = 24: 6 vectors per pixel leave 4 of the 1024 threads without a lane"""
    d, want_di, want_bias = N.case_bwd_fin_apply_add(npix, Cc, dtype, 3, 4)
    for bias_rows in N.BIAS_ROWS:
        got, before = _backward("add", d, npix, Cc, dtype, (1, 1, 1), 1, bias_rows=bias_rows)
        _check_finish(got, before, d, Cc, (1, 1, 1), 1)
        _same(got["r"], want_di)
        _same(got["bias"], want_bias[bias_rows])


# ------------------------------------------------------------------------------------------------------------------------------
# ksmi_bn_fin_add_relu
# ------------------------------------------------------------------------------------------------------------------------------
def _fin_id(c):
    (B, H, W), Cc, pooled = c
    return f"{B}x{H}x{W}x{Cc}" + ("pool" if pooled else "")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
@pytest.mark.parametrize("case", N.FIN_CASES, ids=_fin_id)
def test_bn_fin_add_relu(case, dtype):
    (B, H, W), Cc, pooled = case
    d = N.make_fin_add_relu(B, H, W, Cc, dtype, pooled)
    _check_forward(_forward(d, B, H, W, Cc, dtype, pooled), d, Cc, pooled, _fin_id(case))      # (the step counter: 41 becomes 42)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
def test_bn_fin_add_relu_without_step_counter(dtype):
    d = N.make_fin_add_relu(2, 6, 10, 24, dtype, 1)
    _check_forward(_forward(d, 2, 6, 10, 24, dtype, 1, with_nbt=False), d, 24, 1, "no counter")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
def test_bn_fin_add_relu_count_one_takes_the_biased_variance(dtype):
    d = N.make_fin_add_relu(2, 6, 10, 24, dtype, 1, count=1.0)
    assert bool(d["want"]["rvar"][2].all())                                     # every channel's running variance is bit-exact here
    _check_forward(_forward(d, 2, 6, 10, 24, dtype, 1), d, 24, 1, "count=1")


# ------------------------------------------------------------------------------------------------------------------------------
# the second grid-stride trip, reached by shape (the grid cap is a process-static knob; these assume its default of 256 workgroups)
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", N.FIN_BIG, ids=_fin_id)
def test_bn_fin_add_relu_second_grid_stride_trip(case):
    (B, H, W), Cc, pooled = case
    d = N.make_fin_add_relu(B, H, W, Cc, F32, pooled)
    _check_forward(_forward(d, B, H, W, Cc, F32, pooled), d, Cc, pooled, _fin_id(case))


def test_bn_bwd_fin_apply_second_grid_stride_trip():
    _bwd_fin_apply("relu", *N.BWD_BIG, F32)


# ------------------------------------------------------------------------------------------------------------------------------
# gaussian data: bounds from the operation counts, and the fused call against the launches it replaces
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
@pytest.mark.parametrize("shape", [N.REAL_SHAPE, N.REAL_POOL_SHAPE], ids=["1073px", "1080px_pool"])
def test_forward_real_data(shape, dtype):
    """1073 pixels (29 x 37, odd: not poolable) x 24 channels, 3 rows, eps = 1e-5; and 2 x 18 x 30 for the sequence that ends in the pool"""
    _, _, DT, _ = _env()
    B, H, W = shape
    Cc, npix, pooled = N.REAL_C, B * H * W, shape == N.REAL_POOL_SHAPE
    name = f"{N.dtype_id(dtype)} {npix}px"
    d = N.make_real_forward(B, H, W, Cc, dtype)
    rows = d["partial"].shape[0]
    got = _forward(d, B, H, W, Cc, dtype, pooled, momentum=R.MOMENTUM, eps=R.EPS)
    ref = R.bn_finalize(d["partial"], Cc, d["count"], d["gamma"], d["beta"], d["rmean"], d["rvar"], R.MOMENTUM, R.EPS, True)
    for k, (want, bound) in ref.items():
        if bound is None:
            _same(got[k], R.exact_f32(want, k).float())
        else:
            assert torch.isfinite(got[k]).all()
            _within(f"bn_fin_add_relu {k} {name}", got[k], want, bound)
    # out: the oracle evaluated with the scale and shift the kernel itself published
    want, mag = N.add_relu_real(d["z"].double(), d["idn"].double(), got["scale"].cpu().double(), got["shift"].cpu().double())
    _within(f"bn_fin_add_relu out {name}", got["out"], want, R.half_ulp(want, dtype) + N.N_ADD_RELU * R.U * mag)
    if pooled:                                                                  # a maximum is exact on any data
        _same(got["pooled"], N.pool_of(got["out"].cpu(), B, H, W).to(dtype))
    _same(got["partial"], d["partial"])
    # the launches it replaces: ksmi_bn_finalize + ksmi_bn_add_relu (+ ksmi_maxpool2x2_forward), bit for bit
    partial, gamma, beta, z, idn = (_up(d[k]) for k in ("partial", "gamma", "beta", "z", "idn"))
    rmean, rvar = _up(d["rmean"]), _up(d["rvar"])
    nbt = torch.full((1,), d["nbt"], dtype=torch.int64, device="cuda")
    seq = {k: torch.full((Cc,), NAN, dtype=F32, device="cuda") for k in STATS}
    out = torch.full((npix, Cc), NAN, dtype=dtype, device="cuda")
    _run("ksmi_bn_finalize", partial.data_ptr(), rows, d["Cstride"], Cc, d["count"], gamma.data_ptr(), beta.data_ptr(), rmean.data_ptr(),
         rvar.data_ptr(), nbt.data_ptr(), R.MOMENTUM, R.EPS, 1, *[seq[k].data_ptr() for k in STATS])
    _run("ksmi_bn_add_relu", z.data_ptr(), idn.data_ptr(), seq["scale"].data_ptr(), seq["shift"].data_ptr(), out.data_ptr(), npix, Cc, DT[dtype])
    seq.update(rmean=rmean, rvar=rvar, out=out)
    for k, t in seq.items():
        _same(got[k], t.cpu())
    if pooled:
        y = torch.full((B, H // 2, W // 2, Cc), NAN, dtype=dtype, device="cuda")
        _run("ksmi_maxpool2x2_forward", out.data_ptr(), y.data_ptr(), B, H, W, Cc, DT[dtype])
        _same(got["pooled"], y.cpu())


def _sequence_sums(d, Cc, accumulate):
    """ksmi_reduce_rows on a fresh copy of the rows -> sums, dgamma, dbeta"""
    rows = d["partial"].shape[0]
    partial = _up(d["partial"])
    sums = torch.full((2, Cc), NAN, dtype=F32, device="cuda")
    dgamma, dbeta = (_up(d[k]) if accumulate else torch.full((Cc,), NAN, dtype=F32, device="cuda") for k in ("prior_dgamma", "prior_dbeta"))
    _run("ksmi_reduce_rows", partial.data_ptr(), rows, 2, d["Cstride"], Cc, sums.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), accumulate)
    return {"sums": sums, "dgamma": dgamma, "dbeta": dbeta}


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
def test_backward_real_data(dtype):
    """gaussian inputs and rows at 1073 pixels x 24 channels, 3 rows; the bounds of test_bn_bwd_real_data (tests/test_gpu_elementwise.py)"""
    _, _, DT, _ = _env()
    npix, Cc, rows = N.REAL_NPIX, N.REAL_C, N.REAL_ROWS
    name = N.dtype_id(dtype)
    d = N.make_real_bwd(npix, Cc, dtype)
    d["prior_dgamma"], d["prior_dbeta"] = R.gauss((Cc,), 700).float(), R.gauss((Cc,), 701).float()
    extra = 1 if dtype == BF16 else 0                                           # (bf16: the last fp32 product is one more rounding before the store's)
    dev = {k: _up(d[k]) for k in ("dout", "out", "z", "r", "mean", "rstd", "gamma")}
    par = (dev["mean"].data_ptr(), dev["rstd"].data_ptr(), dev["gamma"].data_ptr())

    def finish(got, kind):
        """the published sums against the fp64 total, the parameter gradients against the published sums -> the oracle's inputs"""
        _within(f"{kind} sums {name}", got["sums"], d["sums64"], N.real_sums_bound(d))
        s = got["sums"].cpu()
        _same(got["dbeta"], s[0])
        _same(got["dgamma"], s[1])
        _same(got["partial"], d["partial"])
        return dict(d, sums=s)

    for mode in N.BWD_MODES:
        got, _ = _backward(mode, d, npix, Cc, dtype)
        g, ref, mag = R.bn_bwd_apply(finish(got, mode), dtype, gate=mode == "relu", exact=False)
        n = R.N_APPLY["apply" if mode == "relu" else "gated"] + extra
        _within(f"bn_bwd_fin_apply[{mode}] {name}", got["dz"], ref, R.half_ulp(ref, dtype) + n * R.U * mag)
        if mode == "relu":
            _same(got["dout"], g)                                               # the gate is exact on any data
        # the launches it replaces, with prior parameter gradients: ksmi_reduce_rows + the matching apply, bit for bit
        got, _ = _backward(mode, d, npix, Cc, dtype, accumulate=1)
        seq = _sequence_sums(d, Cc, 1)
        dout, dz = _up(d["dout"]), torch.full((npix, Cc), NAN, dtype=dtype, device="cuda")
        if mode == "relu":
            _run("ksmi_bnrelu_bwd_apply", dout.data_ptr(), dev["out"].data_ptr(), dev["z"].data_ptr(), *par, seq["sums"].data_ptr(),
                 dz.data_ptr(), d["count"], npix, Cc, DT[dtype])
            _same(got["dout"], dout.cpu())
        else:
            _run("ksmi_bn_bwd_apply_gated", dout.data_ptr(), dev["z"].data_ptr(), *par, seq["sums"].data_ptr(), dz.data_ptr(), d["count"], npix, Cc,
                 DT[dtype])
        for k, t in seq.items():
            _same(got[k], t.cpu())
        _same(got["dz"], dz.cpu())

    def bias_total(name_, bias, stored_di):
        """the bias partial through its column total: each row is within its chain bound, so the total is within their sum"""
        ref, mag = R.bias_partial(stored_di, rows, exact=False)
        bound = (R.half_ulp(ref, F32) + R.reduce_chain(npix, rows, Cc, dtype) * R.U * mag).sum(0)
        _within(name_, bias.cpu().double().sum(0), ref.sum(0), bound)

    got, _ = _backward("add", d, npix, Cc, dtype, bias_rows=rows)
    ref, mag = R.bn_bwd_apply_add(finish(got, "add"), rows, dtype, exact=False)
    _within(f"bn_bwd_fin_apply_add {name}", got["r"], ref, R.half_ulp(ref, dtype) + (R.N_APPLY_ADD + extra) * R.U * mag)
    bias_total(f"bn_bwd_fin_apply_add partial total {name}", got["bias"], got["r"].cpu())
    got, _ = _backward("add", d, npix, Cc, dtype, accumulate=1, bias_rows=rows)
    seq = _sequence_sums(d, Cc, 1)
    r, bias = _up(d["r"]), torch.full((rows, Cc), NAN, dtype=F32, device="cuda")
    _run("ksmi_bn_bwd_apply_add", r.data_ptr(), dev["dout"].data_ptr(), dev["z"].data_ptr(), *par, seq["sums"].data_ptr(), bias.data_ptr(), rows,
         d["count"], npix, Cc, DT[dtype])
    for k, t in seq.items():
        _same(got[k], t.cpu())
    _same(got["r"], r.cpu())
    bias_total(f"bn_bwd_apply_add partial total {name}", bias, r.cpu())         # (the two kernels add their pixel lanes in different orders)
    bias_total(f"bn_bwd_fin_apply_add partial total, accumulate {name}", got["bias"], r.cpu())


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: the launcher returns an error code before any launch, and ksmi_bn_fused_supported says the same
# ------------------------------------------------------------------------------------------------------------------------------
def test_max_rows():
    lib, _, _, _ = _env()
    assert lib.ksmi_bn_fused_max_rows() == N.MAX_ROWS == 256


def test_bad_arguments_are_refused():
    lib, _, DT, st = _env()
    t, chk = _guarded((1 << 16,), F32, 0.0)
    p, bf, f32 = t.data_ptr(), DT[BF16], DT[F32]
    before = t.clone()

    def fwd(partial=p, rows=3, Cs=8, Cc=8, pooled=None, B=1, H=2, W=2, dt=bf):
        return lib.ksmi_bn_fin_add_relu(partial, rows, Cs, Cc, 4.0, p, p, p, p, None, 0.25, 1.0, p, p, p, p, p, p, p, pooled, B, H, W, dt, st)

    def gated(partial=p, rows=3, Cs=8, Cc=8, npix=4, dt=bf):
        return lib.ksmi_bn_bwd_fin_apply_gated(partial, rows, Cs, p, p, p, 0, p, p, p, p, p, p, 4.0, npix, Cc, dt, st)

    def relu(partial=p, rows=3, Cs=8, Cc=8, npix=4, dt=bf):
        return lib.ksmi_bnrelu_bwd_fin_apply(partial, rows, Cs, p, p, p, 0, p, p, p, p, p, p, p, 4.0, npix, Cc, dt, st)

    def add(partial=p, rows=3, Cs=8, Cc=8, npix=4, dt=bf, bias=p, bias_rows=2):
        return lib.ksmi_bn_bwd_fin_apply_add(partial, rows, Cs, p, p, p, 0, p, p, p, p, p, p, bias, bias_rows, 4.0, npix, Cc, dt, st)

    launchers = {"fin_add_relu": fwd, "fin_apply_gated": gated, "bnrelu_fin_apply": relu, "fin_apply_add": add}
    # (what ksmi_bn_fused_supported(C, Cstride, dtype) must refuse as well, the launchers' arguments)
    shapes = {
        "C = 12 in bf16": ((12, 12, bf), dict(Cs=12, Cc=12)),
        "C = 516": ((516, 516, f32), dict(Cs=516, Cc=516, dt=f32)),
        "C = 0": ((0, 8, f32), dict(Cc=0, dt=f32)),
        "Cstride < C": ((16, 8, bf), dict(Cs=8, Cc=16)),
        "Cstride % 4": ((8, 10, bf), dict(Cs=10)),
        "dtype": ((8, 8, 7), dict(dt=7)),
    }
    refused = {}
    for what, (sup, kw) in shapes.items():
        assert lib.ksmi_bn_fused_supported(*sup) == 0, what
        for name, fn in launchers.items():
            refused[f"{name} {what}"] = fn(**kw)
    for sup, ok in (((8, 8, bf), 1), ((4, 8, f32), 1), ((512, 512, bf), 1), ((24, 28, f32), 1), ((4, 4, bf), 0)):
        assert lib.ksmi_bn_fused_supported(*sup) == ok, sup
    for name, fn in launchers.items():
        refused[f"{name} rows = 0"] = fn(rows=0)
        refused[f"{name} partial = NULL"] = fn(partial=None)
    refused["fin_add_relu pooled, odd H"] = fwd(pooled=p, H=3, W=2)
    refused["fin_add_relu pooled, odd W"] = fwd(pooled=p, H=2, W=3)
    refused["fin_add_relu npix = 0"] = fwd(B=0)
    for name in ("fin_apply_gated", "bnrelu_fin_apply", "fin_apply_add"):
        refused[f"{name} npix = 0"] = launchers[name](npix=0)
    refused["fin_apply_add bias_rows = 0"] = add(bias_rows=0)
    refused["fin_apply_add bias_rows = 257"] = add(bias_rows=257)
    refused["fin_apply_add bias_partial = NULL"] = add(bias=None)
    torch.cuda.synchronize()
    accepted = [k for k, rc in refused.items() if rc == 0]
    assert not accepted, accepted
    chk()
    assert torch.equal(t, before)                                               # nothing was launched
