"""Every entry point of the ECAM head (csrc/head.hip) against the float64 oracles of tests/head_ref.py, bit for bit: the inputs are small
integers, multiples of 1/8 and powers of two on which the kernels' fp32 evaluation is exact whatever the summation order and the
number of pixel splits (the oracles assert that precondition; tests/test_head_ref_cpu.py runs them for every case here without a GPU).
The conventions are those of tests/test_gpu_elementwise.py: inputs go up as host tensors, bf16 as raw bits; every output and every
workspace lives between guard words, outputs start as NaN (argmax as -1); read-only inputs are compared with their host copies after
the call; workspaces are sized by the *_workspace entry points.  The two results that are not dyadic, the sigmoid of the MLP and dx
where 1 / HW is no power of two, are held to the bound the oracle derives from the kernel's operation count; the test prints
error / bound.  test_chain runs the six entry points in sequence on gaussian data against the float64 autograd of the whole head."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
GUARD = 64
NAN = float("nan")
CASE_IDS = [R.case_id(c) for c in R.CASES]


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
    """a device tensor of `shape` between GUARD sentinel elements on either side, filled with `init` -> (view, check)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), 77, dtype=dtype, device="cuda")
    view = flat[GUARD:GUARD + n].view(shape)
    view.fill_(init)

    def check():
        assert (flat[:GUARD] == 77).all() and (flat[GUARD + n:] == 77).all(), "write outside the tensor"
    return view, check


def _workspace(nbytes):
    """a workspace of exactly the size its entry point asks for, between guard bytes"""
    return _guarded((int(nbytes),), torch.uint8, 0)


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


def _x4(stored_xs):
    """the four sources on the device and the pointer array the entry points take"""
    xs = [_up(x) for x in stored_xs]
    return xs, (C.c_void_p * 4)(*[x.data_ptr() for x in xs])


def _f32(d, keys):
    host = {k: d[k].float() for k in keys}
    return host, {k: _up(v) for k, v in host.items()}


def _unchanged(dev, host):
    for k, v in (dev.items() if isinstance(dev, dict) else enumerate(dev)):
        _same(v, host[k])


# ------------------------------------------------------------------------------------------------------------------------------
# pool
# ------------------------------------------------------------------------------------------------------------------------------
def _pool(st, Cc, dtype, B, HW):
    lib, _, DT, _ = _env()
    xs, arr = _x4(st)
    avg, c0 = _guarded((B, 5 * Cc), F32)
    mx, c1 = _guarded((B, 5 * Cc), F32)
    am, c2 = _guarded((B, 5 * Cc), torch.int32, -1)
    ws, c3 = _workspace(lib.ksmi_ecam_pool_workspace(B, HW, Cc))
    _run("ksmi_ecam_pool", arr, avg.data_ptr(), mx.data_ptr(), am.data_ptr(), ws.data_ptr(), B, HW, Cc, DT[dtype])
    for c in (c0, c1, c2, c3):
        c()
    _unchanged(xs, st)
    return avg, mx, am


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
@pytest.mark.parametrize("kind", R.POOL_KINDS)
def test_pool(kind, case):
    """rounding: random integers, bf16 sums of intra that the conversion changes; ties: the top value of every channel at up to three
    pixels, in one thread, two lanes, two waves and two splits"""
    Cc, dtype, B, HW = case
    st, ref = R.case_pool(kind, case)
    avg, mx, am = _pool(st, Cc, dtype, B, HW)
    _same(am, ref["argmax"])
    _same(mx, ref["mx"].float())
    _same(avg, ref["avg"].float())


@pytest.mark.parametrize("case", [(16, F32, 3, 65), (256, F32, 1, 63), (64, BF16, 3, 1000), (512, BF16, 1, 16)], ids=R.case_id)
def test_pool_of_a_nan_channel_keeps_argmax_inside_the_image(case):
    """a channel in which no value compares greater than the start of the maximum search: its argmax must still name a pixel (the
    backward scatters there), its avg is NaN, and every other channel is what it was"""
    Cc, dtype, B, HW = case
    st, ref, nan = R.make_pool_nan(B, HW, Cc, dtype)
    avg, mx, am = (t.cpu() for t in _pool(st, Cc, dtype, B, HW))
    assert int(am.min()) >= 0 and int(am.max()) < HW
    assert bool(torch.isnan(avg[nan]).all())
    _same(am[~nan], ref["argmax"][~nan])
    _same(mx[~nan], ref["mx"].float()[~nan])
    _same(avg[~nan], ref["avg"].float()[~nan])


# ------------------------------------------------------------------------------------------------------------------------------
# the two MLPs
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("CB", R.MLP_CASES, ids=lambda cb: f"C{cb[0]}-B{cb[1]}")
def test_mlp(CB):
    Cc, B = CB
    d = R.case_mlp(Cc, B)
    ref = d["ref"]
    host, dev = _f32(d, ["avg", "mx", "w1", "w2", "v1", "v2"])
    ca, c0 = _guarded((B, 4 * Cc), F32)
    ca1, c1 = _guarded((B, Cc), F32)
    hidden, c2 = _guarded((B, 2, Cc // 2), F32)
    _run("ksmi_ecam_mlp", *[dev[k].data_ptr() for k in ("avg", "mx", "w1", "w2", "v1", "v2")], ca.data_ptr(), ca1.data_ptr(), hidden.data_ptr(),
         B, Cc)
    for c in (c0, c1, c2):
        c()
    _unchanged(dev, host)
    _same(hidden, ref["hidden"].float())
    _within(f"mlp ca C{Cc} B{B}", ca, ref["ca"], ref["ca_bound"])
    _within(f"mlp ca1 C{Cc} B{B}", ca1, ref["ca1"], ref["ca1_bound"])


# ------------------------------------------------------------------------------------------------------------------------------
# fusion + conv_final, forward and the reductions of its backward
# ------------------------------------------------------------------------------------------------------------------------------
def _final_forward(case):
    _, _, DT, _ = _env()
    Cc, dtype, B, HW = case
    d = R.case_final(case, backward=False)
    xs, arr = _x4(d["x"])
    host, dev = _f32(d, ["ca", "ca1", "wf", "bias"])
    logits, chk = _guarded((B, R.NCLS, HW), F32)
    _run("ksmi_ecam_final_forward", arr, dev["ca"].data_ptr(), dev["ca1"].data_ptr(), dev["wf"].data_ptr(), dev["bias"].data_ptr(),
         logits.data_ptr(), B, HW, Cc, R.NCLS, DT[dtype])
    chk()
    _unchanged(xs, d["x"])
    _unchanged(dev, host)
    _same(logits, d["logits"].float())


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_final_forward(case):
    _final_forward(case)


def test_final_forward_grid_stride():
    """more pixels than the 256 x 256 threads of the largest grid: a second trip and its tail"""
    _final_forward(R.GRID_STRIDE_CASE)


@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_final_backward_reduce(case):
    """dca, dca1, dWf and dbias start as NaN and come back overwritten; G and DL are read from the workspace, which keeps them after the
    per-split partials (sizes by ksmi_ecam_bwd_workspace)"""
    lib, _, DT, _ = _env()
    Cc, dtype, B, HW = case
    d = R.case_final(case, forward=False)
    ref = d["reduce"]
    xs, arr = _x4(d["x"])
    host, dev = _f32(d, ["dl", "ca", "ca1", "wf"])
    outs = {"dca": (B, 4 * Cc), "dca1": (B, Cc), "dwf": (R.NCLS, 4 * Cc), "dbias": (R.NCLS,)}
    out = {k: _guarded(shape, F32) for k, shape in outs.items()}
    nbytes = lib.ksmi_ecam_bwd_workspace(B, HW, Cc, R.NCLS)
    ws, chk = _workspace(nbytes)
    _run("ksmi_ecam_final_backward_reduce", arr, *[dev[k].data_ptr() for k in ("dl", "ca", "ca1", "wf")], *[out[k][0].data_ptr() for k in outs],
         ws.data_ptr(), B, HW, Cc, R.NCLS, DT[dtype])
    chk()
    for k in outs:
        out[k][1]()
        _same(out[k][0], ref[k].float())
    _unchanged(xs, d["x"])
    _unchanged(dev, host)
    # workspace: partials [B][S][3][4C] and [B][S][3], then G [B][3][4C], DL [B][3], then the MLP backward's share
    unit, mlp_share = B * R.NCLS * (4 * Cc + 1), B * 6 * Cc
    S, rest = divmod(nbytes // 4 - mlp_share - unit, unit)
    assert rest == 0 and S >= 1, (nbytes, S, rest)
    w = ws.view(F32)[S * unit:(S + 1) * unit]
    _same(w[:B * R.NCLS * 4 * Cc].view(B, R.NCLS, 4 * Cc), ref["G"].float())
    _same(w[B * R.NCLS * 4 * Cc:].view(B, R.NCLS), ref["DL"].float())


# ------------------------------------------------------------------------------------------------------------------------------
# MLP backward
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("CB", R.MLP_CASES, ids=lambda cb: f"C{cb[0]}-B{cb[1]}")
def test_mlp_backward(CB):
    """every gradient output starts as NaN and comes back overwritten (the fc weight gradients are stored with =, not accumulated); ds and
    dh are read from the workspace, which holds nothing else"""
    lib, _, _, _ = _env()
    Cc, B = CB
    d = R.case_mlp_backward(Cc, B)
    ref = d["ref"]
    host, dev = _f32(d, R.MLP_BWD_ARGS)
    Hh = Cc // 4
    outs = {"davg": (B, 5 * Cc), "dmax": (B, 5 * Cc), "gw1": (Hh, 4 * Cc), "gw2": (4 * Cc, Hh), "gv1": (Hh, Cc), "gv2": (Cc, Hh)}
    out = {k: _guarded(shape, F32) for k, shape in outs.items()}
    nbytes = lib.ksmi_ecam_mlp_bwd_workspace(B, Cc)
    assert nbytes == 4 * (B * 5 * Cc + B * 2 * 2 * Hh)
    ws, chk = _workspace(nbytes)
    _run("ksmi_ecam_mlp_backward", *[dev[k].data_ptr() for k in R.MLP_BWD_ARGS], *[out[k][0].data_ptr() for k in outs], ws.data_ptr(), B, Cc)
    chk()
    for k in outs:
        out[k][1]()
        _same(out[k][0], ref[k].float())
    _unchanged(dev, host)
    w = ws.view(F32)
    _same(w[:B * 5 * Cc].view(B, 5 * Cc), ref["ds"].float())
    _same(w[B * 5 * Cc:].view(B, 2, 2 * Hh), ref["dh"].float())


# ------------------------------------------------------------------------------------------------------------------------------
# backward, phase B: dx and the max-pool scatter
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=CASE_IDS)
def test_final_backward_dx(case):
    """HW a power of two: the bits, scatter included (a source's and intra's first maximum meet in one element in some channels);
    otherwise the bound"""
    _, _, DT, _ = _env()
    Cc, dtype, B, HW = case
    d = R.case_dx(case)
    ref = d["ref"]
    host, dev = _f32(d, ["dl", "ca", "wf", "davg", "dmax"])
    am = d["argmax"].cuda()
    dx = [_guarded((B, HW, Cc), dtype) for _ in range(4)]
    arr = (C.c_void_p * 4)(*[t.data_ptr() for t, _ in dx])
    _run("ksmi_ecam_final_backward_dx", arr, *[dev[k].data_ptr() for k in ("dl", "ca", "wf", "davg", "dmax")], am.data_ptr(), B, HW, Cc, R.NCLS,
         DT[dtype])
    worst = 0.0
    for s, (t, chk) in enumerate(dx):
        chk()
        if ref["bound"] is None:
            _same(t, ref["dx"][s].float().to(dtype))
        else:
            assert not torch.isnan(t).any()
            worst = max(worst, R.ratio(t.cpu(), ref["dx"][s], ref["bound"][s]))
    if ref["bound"] is not None:
        print(f"RATIO dx {R.case_id(case)} {worst:.4f}")
        assert worst <= 1.0, f"dx: error / bound = {worst}"
    _unchanged(dev, host)
    _same(am, d["argmax"])


# ------------------------------------------------------------------------------------------------------------------------------
# the six entry points in sequence
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.DTYPE_IDS)
def test_chain(dtype):
    """pool -> mlp -> final_forward -> backward_reduce -> mlp_backward -> backward_dx on gaussian data against the float64 autograd of the
    head.  Per output: max |gpu - ref64| <= 4 * max(max |cpu32 - ref64|, half an ulp of the output dtype at max |ref64|), cpu32 being the
    same function evaluated by torch in fp32 on the CPU (dx rounded to the activation dtype).  The 4 covers another summation order and up to
    three bf16 roundings of a scatter element against one; a missing term is orders of magnitude outside."""
    lib, _, DT, _ = _env()
    Cc, B, HW = R.CHAIN_CASE
    d = R.make_chain(dtype)
    ref64, cpu32 = R.chain_reference(d, dtype, F64), R.chain_reference(d, dtype, F32)
    xs, arr = _x4(d["x"])
    p = {k: _up(v) for k, v in d["p"].items()}
    dl = _up(d["dl"])
    Hh = Cc // 4
    shapes = {"avg": (B, 5 * Cc), "mx": (B, 5 * Cc), "ca": (B, 4 * Cc), "ca1": (B, Cc), "hidden": (B, 2, 2 * Hh), "logits": (B, R.NCLS, HW),
              "dca": (B, 4 * Cc), "dca1": (B, Cc), "dwf": (R.NCLS, 4 * Cc), "dbias": (R.NCLS,), "davg": (B, 5 * Cc), "dmax": (B, 5 * Cc),
              "dw1": (Hh, 4 * Cc), "dw2": (4 * Cc, Hh), "dv1": (Hh, Cc), "dv2": (Cc, Hh)}
    t = {k: _guarded(s, F32) for k, s in shapes.items()}
    t["argmax"] = _guarded((B, 5 * Cc), torch.int32, -1)
    for s in range(4):
        t[f"dx{s}"] = _guarded((B, HW, Cc), dtype)
    ws = {"pool": _workspace(lib.ksmi_ecam_pool_workspace(B, HW, Cc)), "bwd": _workspace(lib.ksmi_ecam_bwd_workspace(B, HW, Cc, R.NCLS)),
          "mlp": _workspace(lib.ksmi_ecam_mlp_bwd_workspace(B, Cc))}
    P = lambda *names: [(t[n][0] if n in t else p[n]).data_ptr() for n in names]  # noqa: E731
    garr = (C.c_void_p * 4)(*P("dx0", "dx1", "dx2", "dx3"))
    dt = DT[dtype]
    _run("ksmi_ecam_pool", arr, *P("avg", "mx", "argmax"), ws["pool"][0].data_ptr(), B, HW, Cc, dt)
    _run("ksmi_ecam_mlp", *P("avg", "mx", "w1", "w2", "v1", "v2", "ca", "ca1", "hidden"), B, Cc)
    _run("ksmi_ecam_final_forward", arr, *P("ca", "ca1", "wf", "bias", "logits"), B, HW, Cc, R.NCLS, dt)
    _run("ksmi_ecam_final_backward_reduce", arr, dl.data_ptr(), *P("ca", "ca1", "wf", "dca", "dca1", "dwf", "dbias"), ws["bwd"][0].data_ptr(),
         B, HW, Cc, R.NCLS, dt)
    _run("ksmi_ecam_mlp_backward", *P("avg", "mx", "hidden", "ca", "ca1", "dca", "dca1", "w1", "w2", "v1", "v2", "davg", "dmax", "dw1", "dw2",
                                      "dv1", "dv2"), ws["mlp"][0].data_ptr(), B, Cc)
    _run("ksmi_ecam_final_backward_dx", garr, dl.data_ptr(), *P("ca", "wf", "davg", "dmax", "argmax"), B, HW, Cc, R.NCLS, dt)
    for _, chk in list(t.values()) + list(ws.values()):
        chk()
    _unchanged(xs, d["x"])
    failed = []
    for name in ref64:
        got = t[name][0].cpu().double()
        assert not torch.isnan(got).any(), name
        err, yard = float((got - ref64[name]).abs().max()), float((cpu32[name] - ref64[name]).abs().max())
        tol = R.chain_tolerance(ref64, cpu32, name, dtype if name.startswith("dx") else F32)
        print(f"CHAIN {R.dtype_id(dtype)} {name}: gpu_err {err:.3e} cpu32_err {yard:.3e} ratio {err / yard if yard else float('inf'):.3f} "
              f"err / tol {err / tol:.4f}")
        if err > tol:
            failed.append((name, err, tol))
    assert not failed, failed


# ------------------------------------------------------------------------------------------------------------------------------
# refusals: the launcher returns an error code before any launch
# ------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused():
    lib, _, DT, st = _env()
    t = torch.full((1 << 18,), NAN, dtype=F32, device="cuda")
    p, bf, f32, bad = t.data_ptr(), DT[BF16], DT[F32], 99
    assert bad not in (bf, f32)
    a4 = (C.c_void_p * 4)(p, p, p, p)
    B, HW = 1, 64

    refused = {}

    def walkers(tag, Cc, ncls, dt):
        """the entry points that walk the activations; the pool has no class count"""
        if ncls == 3:
            refused[f"pool {tag}"] = lib.ksmi_ecam_pool(a4, p, p, p, p, B, HW, Cc, dt, st)
        refused[f"final_forward {tag}"] = lib.ksmi_ecam_final_forward(a4, p, p, p, p, p, B, HW, Cc, ncls, dt, st)
        refused[f"backward_reduce {tag}"] = lib.ksmi_ecam_final_backward_reduce(a4, p, p, p, p, p, p, p, p, p, B, HW, Cc, ncls, dt, st)
        refused[f"backward_dx {tag}"] = lib.ksmi_ecam_final_backward_dx(a4, p, p, p, p, p, p, B, HW, Cc, ncls, dt, st)
    for Cc in (24, 48):                                  # not a multiple of 16; C / VEC does not divide the 256 threads
        for name, dt in (("bf16", bf), ("fp32", f32)):
            walkers(f"C{Cc} {name}", Cc, 3, dt)
    walkers("C512 fp32", 512, 3, f32)                    # 4C / VEC > 256 threads
    walkers("bad dtype", 16, 3, bad)
    walkers("ncls 2", 16, 2, f32)
    refused["mlp C24"] = lib.ksmi_ecam_mlp(p, p, p, p, p, p, p, p, p, B, 24, st)
    refused["mlp_backward C24"] = lib.ksmi_ecam_mlp_backward(*([p] * 18), B, 24, st)
    refused["mlp_backward null workspace"] = lib.ksmi_ecam_mlp_backward(*([p] * 17), None, B, 16, st)
    torch.cuda.synchronize()
    accepted = [k for k, rc in refused.items() if rc == 0]
    assert not accepted, accepted
    assert bool(torch.isnan(t).all())                    # nothing was launched
