"""The convolution family (ksmi_conv_forward / ksmi_conv_wgrad and every kernel they route to) against the integer oracles of
tests/conv_ref.py, bit for bit.  On the small-integer operands built there every fp32 partial sum is exact, so the summation order,
the split, the ring depth and the MFMA shape cannot change a bit; the oracle is F.conv2d and its autograd in float64 and one rounding
to the storage type (tests/test_conv_ref_cpu.py builds every case here without a GPU and asserts the exactness preconditions and
the routes).  Each case first asserts the route its table row names (ksmi_conv_dispatch_info / ksmi_conv_wgrad_dispatch_info), runs,
and checks that ksmi_last_kernels lists exactly that kernel.  Outputs, gradients, statistics and bias buffers live between guard
words and start as NaN (as integers where the call accumulates); inputs are compared with their host copies afterwards; bf16 tensors
go up as raw bits.  Statistics are compared as the float64 sum over the rows of the buffer against the integer total: exact, because
every row is an integer below 2^24 whatever rows the kernel chose.  The only tolerance in this file is the gaussian cross-check at
the end, which holds the same descriptors to the bound of the earlier suites and prints error / bound.

Out of reach in-process (switches latched in a `static`): weight-gradient core 2 (the first-generation token GEMM) and the three
opt-in igemm4 schedules."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
GUARD = 64
NAN = float("nan")


def _env():
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import DT, stream_ptr
    return _lib.load(), _lib, DT, stream_ptr()


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


def _same(got, want, what=""):
    """bit equality of a device tensor with the host expectation (-0.0 and +0.0 differ, NaN equals the same NaN)"""
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def _kernels(lib):
    buf = C.create_string_buffer(8192)
    n = lib.ksmi_last_kernels(buf, 8192)
    return [s for s in buf.value.decode().split(";") if s] if n else []


def _upload_all(t, keys):
    """the read-only tensors of a case on the device, with the host copies they are compared with afterwards"""
    dev, pairs = {}, []
    for k in keys:
        if k not in t:
            continue
        v = t[k]
        if isinstance(v, (list, tuple)) and len(v) and isinstance(v[0], torch.Tensor):
            dev[k] = [_up(x) for x in v]
            pairs += list(zip(dev[k], v))
        elif isinstance(v, torch.Tensor):
            dev[k] = _up(v)
            pairs.append((dev[k], v))
        else:
            dev[k] = v
    return dev, pairs


# ------------------------------------------------------------------------------------------------------------------------------
# forward and input gradient
# ------------------------------------------------------------------------------------------------------------------------------
def _run_forward(c, t):
    """build, route-check and launch one forward case -> (destinations, statistics [rows, 2, Npad] or None, dispatch info)"""
    from kurosiwo_amd import functional as Fk
    lib, _lib, DT, st = _env()
    dt = c["dtype"]
    dev, pairs = _upload_all(t, ("xs", "scale", "shift", "bias", "resid", "mask", "gate", "w"))
    outs, checks = zip(*[_guarded(tuple(p.shape), dt, p if c["acc"] else NAN) for p in R.forward_prefill(c, t)])
    with _lib.knobs(**c["knobs"]):
        probe = torch.zeros(16, dtype=F32, device="cuda")
        d, table, rows = R.forward_desc(c, dev, list(outs), probe)
        stats = None
        if c["stats"]:
            stats, chk = _guarded((rows, 2, d.Npad), F32)
            checks = checks + (chk,)
            d.stats = stats.data_ptr()
        info = R.assert_forward_route(c, d)
        if c["stats"]:          # the row count is that of the kernel that runs: workgroups of a persistent kernel, tiles of a tile kernel
            assert rows == (info[6] if info[0] >= 3 else lib.ksmi_conv_grid_m(C.byref(d))), (rows, info)
        wpk = Fk._pack(dev["w"], *R.forward_pack_args(c, table), dt)
        d.wpk = wpk.data_ptr()
        _kernels(lib)
        _lib.check(lib.ksmi_conv_forward(C.byref(d), DT[dt], st), c["name"])
        names = _kernels(lib)
    torch.cuda.synchronize()
    assert len(names) == 1 and names[0].startswith(R.forward_kernel_prefix(c, info)), (names, info)
    for chk in checks:
        chk()
    for got, want in pairs:
        _same(got, want, "an input changed")
    return outs, stats, info


@pytest.mark.parametrize("name", [c["name"] for c in R.FWD_CASES])
def test_forward(name):
    c, t = R.FWD_BY_NAME[name], R.make_forward(name)
    outs, stats, _ = _run_forward(c, t)
    for i, (o, want) in enumerate(zip(outs, t["outs"])):
        _same(o, want, f"destination {i}")
    if stats is not None:
        s = stats.cpu()[:, :, :c["N"]]
        assert not torch.isnan(s).any(), "a statistics row was not written"
        got = s.double().sum(0)
        assert torch.equal(got, t["stats"]), (got - t["stats"]).abs().max()


# ------------------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("name", [c["name"] for c in R.WG_CASES])
def test_wgrad(name, accumulate):
    lib, _lib, DT, st = _env()
    c, t = R.WG_BY_NAME[name], R.make_wgrad(name)
    dt = c["dtype"]
    dev, pairs = _upload_all(t, ("xs", "dy", "scale", "shift", "tap_off"))
    grad, chk_g = _guarded(t["shape"], F32, t["prior"] if accumulate else NAN)
    checks = [chk_g]
    with _lib.knobs(**c["knobs"]):
        d, ws = R.wgrad_desc(c, dev, grad, accumulate)
        info = R.assert_wgrad_route(c, d)
        slab, chk_s = _guarded((max(int(ws) // 4, 4),), F32)          # NaN slabs: a slab the reducer reads but no workgroup wrote shows
        checks.append(chk_s)
        d.partial = slab.data_ptr()
        bias = None
        if c["bias"]:
            mode = info[3]
            assert mode == lib.ksmi_conv_wgrad_fuses_bias(C.byref(d), DT[dt])
            init = torch.full((max(info[2], 1), c["N"]), NAN)
            if mode == 1 and accumulate:
                init[0] = t["bias_prior"]
            bias, chk_b = _guarded(tuple(init.shape), F32, init)
            checks.append(chk_b)
            d.bias_grad, d.bias_accumulate = bias.data_ptr(), accumulate if mode == 1 else 0
        _kernels(lib)
        _lib.check(lib.ksmi_conv_wgrad(C.byref(d), DT[dt], st), name)
        names = _kernels(lib)
    torch.cuda.synchronize()
    want = [c["kernel"] or R.WG_CORE[info[0]]] + ([R.WG_REDUCER[info[1]]] if info[1] else [])
    assert len(names) == len(want) and names[0].startswith(want[0]) and names[1:] == want[1:], (names, want)
    for chk in checks:
        chk()
    for got, host in pairs:
        _same(got, host, "an input changed")
    _same(grad, t["grad"][accumulate], "weight gradient")
    if bias is not None:
        b = bias.cpu()
        if mode == 1:
            _same(bias[0], t["db"][accumulate], "bias gradient")
        else:                   # one partial row per split, overwritten: every row an integer, their total the column sum of d out
            assert mode == 2 and not torch.isnan(b).any() and torch.equal(b, b.round())
            assert torch.equal(b.double().sum(0), t["db"][0].double())


# ------------------------------------------------------------------------------------------------------------------------------
# composition and the gaussian cross-check
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.COMPOSE_CASES, ids=lambda c: c[0])
def test_forward_dgrad_wgrad_of_one_layer(case):
    """y = conv3x3(x, w) + b, dx and dW from one dy, through kurosiwo_amd.functional on one set of tensors, against autograd in float64"""
    from kurosiwo_amd import functional as Fk
    lib, _lib, _, _ = _env()
    name, B, H, W, K, N, knobs, k_fwd, k_dgrad = case
    t = R.make_compose(name)
    x, dy, w, b = _up(t["x"]), _up(t["dy"]), _up(t["w"]), _up(t["bias"])
    with _lib.knobs(**knobs):
        _kernels(lib)
        y, _ = Fk.conv3x3([x], w, b)
        n1 = _kernels(lib)
        dx, = Fk.conv3x3_dgrad(dy, w, [K])
        n2 = _kernels(lib)
        dw = Fk.conv3x3_wgrad([x], dy)
        n3 = _kernels(lib)
    torch.cuda.synchronize()
    assert n1[0].startswith(k_fwd) and n2[0].startswith(k_dgrad) and n3[0].startswith("wgrad3_kernel<"), (n1, n2, n3)
    _same(y, t["y"], "y")
    _same(dx, t["dx"], "dx")
    _same(dw, t["dw"], "dW")
    _same(x, t["x"], "x changed")
    _same(dy, t["dy"], "dy changed")


@pytest.mark.parametrize("name", R.GAUSS_CASES)
def test_gaussian_data_agree_with_the_same_oracle(name):
    """the descriptor, packer and oracle code of the integer case on gaussian data, under the bound of the earlier suites"""
    c, t = R.FWD_BY_NAME[name], R.make_forward(name, True)
    outs, stats, _ = _run_forward(c, t)
    ref = t["ref"]
    err = float((outs[0].cpu().double() - ref).abs().max())
    bound = R.GAUSS_TOL * float(ref.abs().max())
    s = stats.cpu()[:, :, :c["N"]].double().sum(0)
    r_stats = float(((s - t["stats"]).abs() / (torch.tensor([[1e-3], [2e-3]], dtype=torch.float64) * t["stats_mag"].max(1, keepdim=True)[0])).max())
    print(f"RATIO gaussian {name}: output {err / bound:.4f} statistics {r_stats:.4f}")
    assert err < bound and r_stats < 1.0, (err, bound, r_stats)
