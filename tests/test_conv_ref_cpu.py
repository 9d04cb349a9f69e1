"""tests/conv_ref.py without a GPU: the oracles against stock torch (F.conv2d / F.conv_transpose2d and autograd in float64, the mask and
gate epilogues against the block backward they replace, the bf16 rounding against torch on ties), and every case of
tests/test_gpu_conv_exact.py built on CPU tensors: the builders assert the exactness preconditions (accumulators, statistics and
gradient sums below 2^24), and the host-only dispatch hooks must name the route each table row carries -- a row that silently lands on
another kernel fails here.  The argument refusals of ksmi_conv_forward launch nothing and are checked here too."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

from kurosiwo_amd import _lib  # noqa: E402
from kurosiwo_amd.runtime import DT  # noqa: E402

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------------------------------------
# rounding
# ------------------------------------------------------------------------------------------------------------------------------
def test_bf16_rounding_is_to_nearest_even_on_ties():
    # integers 256 .. 1023 hold every tie of the 9- and 10-bit range (257 -> 256, 259 -> 260); negatives, and values just off a tie
    x = torch.arange(-1023, 1024, dtype=F32)
    x = torch.cat([x, x * 0.25, x + 2.0 ** -12, torch.tensor([0.0, -0.0, 65280.0, 65408.0, 3.3895e38])])
    got = R.bf16_rne_bits(x)
    want = x.to(BF16).view(torch.int16).to(torch.int32) & 0xFFFF
    assert torch.equal(got, want)
    t = torch.tensor([257.0, 259.0, -257.0, 1026.0, 1030.0])
    assert R.stored(t.double(), BF16).float().tolist() == [256.0, 260.0, -256.0, 1024.0, 1032.0]
    assert R.stored(torch.tensor([-0.0], dtype=F64), BF16).view(torch.int16).item() == 0          # accumulators start at +0.0


# ------------------------------------------------------------------------------------------------------------------------------
# the oracles against stock torch
# ------------------------------------------------------------------------------------------------------------------------------
def _srcs(t):
    return torch.cat([R.nchw(x.double()) for x in t["xs"]], 1)


def test_deconv_oracle_is_conv_transpose2d():
    name = "ig3 deconv 64->4x16 stats"
    t = R.make_forward(name)
    ref = F.conv_transpose2d(_srcs(t), t["w"].double(), t["bias"].double(), stride=2)
    assert torch.equal(R.nchw(t["outs"][0].double()), R.stored(ref, BF16).double())
    # the statistics are per COLUMN (dy, dx, n) of the 1 x 1 GEMM: their sum over the four taps is the per-channel sum of the output
    co = R.FWD_BY_NAME[name]["N"] // 4
    assert torch.equal(t["stats"][0].view(4, co).sum(0), t["outs"][0].double().sum((0, 1, 2)))


def test_dgrad_oracle_is_the_autograd_of_conv2d():
    for name in ("ig3 dgrad 32->32", "ig3 dgrad 16->16+16+16", "ig4 dgrad <8,4> 128->64"):
        c, t = R.FWD_BY_NAME[name], R.make_forward(name)
        dy, wl = _srcs(t), t["w"].double()                                 # the mirrored layer: x[N] -> y[K], weights wl[K, N, 3, 3]
        x = torch.zeros((c["B"], c["N"], c["H"], c["W"]), dtype=F64, requires_grad=True)
        dx, = torch.autograd.grad(F.conv2d(x, wl, padding=1), x, dy)
        got = torch.cat([R.nchw(o.double()) for o in t["outs"]], 1)
        assert torch.equal(got, R.stored(dx, BF16).double()), name


def test_strided_and_phase_oracles():
    # the 2 x 2 stride-2 convolution is the input gradient of ConvTranspose2d(k2, s2): weights w[N, K, 2, 2] = the deconvolution's [Cin, Cout, 2, 2]
    c, t = R.FWD_BY_NAME["ig3 2x2s2 64->32"], R.make_forward("ig3 2x2s2 64->32")
    x = torch.zeros((c["B"], c["N"], c["H"] // 2, c["W"] // 2), dtype=F64, requires_grad=True)
    dx, = torch.autograd.grad(F.conv_transpose2d(x, t["w"].double(), stride=2), x, _srcs(t))
    assert torch.equal(R.nchw(t["outs"][0].double()), dx)
    # a phase convolution, tap by tap: out[oy, ox] = sum_ab x[oy - py + a, ox - px + b] w[a, b], placed at (2 oy + py, 2 ox + px)
    for name in ("ig4 phase (0,0) 64->128", "ig4 phase (1,1) 64->128"):
        c, t = R.FWD_BY_NAME[name], R.make_forward(name)
        py, px = c["phase"]
        x, w = _srcs(t), t["w"].double()
        H, W = c["H"], c["W"]
        xp = torch.zeros((c["B"], x.shape[1], H + 2, W + 2), dtype=F64)
        xp[:, :, 1:H + 1, 1:W + 1] = x
        ref = t["bias"].double().view(1, -1, 1, 1).expand(c["B"], c["N"], H, W).clone()
        for a in range(2):
            for b in range(2):
                win = xp[:, :, 1 - py + a:1 - py + a + H, 1 - px + b:1 - px + b + W]
                ref += torch.einsum("bchw,nc->bnhw", win, w[:, :, a, b])
        o = t["outs"][0]
        assert torch.equal(o[:, py::2, px::2].double(), R.nhwc(R.stored(ref, BF16).double())), name
        other = torch.ones(o.shape[1:3], dtype=torch.bool)
        other[py::2, px::2] = False
        assert torch.isnan(o[:, other]).all()                               # the other three phases keep their prefill


def test_mask_epilogue_is_the_relu_batchnorm_backward_it_replaces():
    """d(pre-activation) of out = relu(m * scale + shift) given the convolution result as d out, and the BatchNorm-backward sums over it"""
    for name in ("ig3 16->16 mask", "ig4 mask 64->64"):
        t = R.make_forward(name)
        m, mean, rstd, sc, sh = [x.double() for x in t["mask"]]
        v = F.conv2d(_srcs(t), t["w"].double(), padding=1)
        a = (R.nchw(m) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
        g, = torch.autograd.grad(torch.relu(a), a, v)
        assert torch.equal(R.nchw(t["outs"][0].double()), R.stored(g, BF16).double()), name
        xh = (R.nchw(m) - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        assert torch.equal(t["stats"], torch.stack([g.sum((0, 2, 3)), (g * xh).sum((0, 2, 3))])), name


def test_gate_epilogue_is_the_block_backward_it_replaces():
    """out = relu(.) of the block: the TOTAL gradient (this launch + what the other producers left in the destination) passes where
    out > 0; (sum g, sum g * zhat) are the BatchNorm2-backward sums"""
    for name in ("ig4 gate 64->64", "ig4 gate accumulate 96->128"):
        c, t = R.FWD_BY_NAME[name], R.make_forward(name)
        gs, z, mean, rstd = [x.double() for x in t["gate"]]
        tot = F.conv2d(_srcs(t), t["w"].double(), padding=1)
        if c["acc"]:
            tot = tot + R.nchw(t["old"].double())
        pre = R.nchw(gs).clone().requires_grad_(True)
        g, = torch.autograd.grad(torch.relu(pre), pre, tot)                 # relu(pre) > 0 exactly where pre = out > 0
        g = R.stored(g, BF16).double()
        assert torch.equal(R.nchw(t["outs"][0].double()), g), name
        zh = (R.nchw(z) - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1)
        assert torch.equal(t["stats"], torch.stack([g.sum((0, 2, 3)), (g * zh).sum((0, 2, 3))])), name


def test_extras_are_the_residual_block():
    name = "ig4 alpha resid relu 64->64"
    c, t = R.FWD_BY_NAME[name], R.make_forward(name)
    ref = torch.relu(c["extras"] * F.conv2d(_srcs(t), t["w"].double(), t["bias"].double(), padding=1) + R.nchw(t["resid"].double()))
    assert torch.equal(R.nchw(t["outs"][0].double()), R.stored(ref, BF16).double())


def test_weight_gradient_oracle_against_functional_layouts():
    # deconv2x2's gradient: weight [Cin, Cout, 2, 2] of y = conv_transpose2d(x, w, stride 2) -- the source of the descriptor is dy, its "dy" is x
    c, t = R.WG_BY_NAME["patch 2x2s2 32->64 NT4"], R.make_wgrad("patch 2x2s2 32->64 NT4")
    dy_img, x = R.nchw(t["xs"][0].double()), R.nchw(t["dy"].double())
    w = torch.zeros((c["N"], 32, 2, 2), dtype=F64, requires_grad=True)
    g, = torch.autograd.grad(F.conv_transpose2d(x, w, stride=2), w, dy_img)
    assert torch.equal(t["grad"][0].double().view(c["N"], 32, 2, 2), g)
    # a token matrix: dW[N, K] = dy^T x, db = column sums of dy
    c, t = R.WG_BY_NAME["tok slabs ragged 471x64->64"], R.make_wgrad("tok slabs ragged 471x64->64")
    x, dy = t["xs"][0].double().view(471, 64), t["dy"].double().view(471, 64)
    assert torch.equal(t["grad"][0].double().view(64, 64), dy.t() @ x) and torch.equal(t["db"][0].double(), dy.sum(0))
    assert torch.equal(t["grad"][1].double().view(64, 64), dy.t() @ x + t["prior"].double().view(64, 64))
    # pad channels of the source and of d out do not reach the gradient
    t = R.make_wgrad("tok element-wise 128x56of64->64")
    assert t["grad"][0].shape == (64, 56, 1) and torch.equal(t["grad"][0].double().view(64, 56), t["dy"].double().view(128, 64).t() @ t["xs"][0].double().view(128, 64)[:, :56])
    t = R.make_wgrad("wg3 32->2 of 8")
    assert t["grad"][0].shape == (2, 32, 9) and int((t["dy"][..., 2:] != 0).sum()) > 0
    # the phase gradients against the whole ConvTranspose2d(k4, s2, p1): x [Cin] -> y [K] on the doubled map, dW[Cin, K, 4, 4] by autograd; each
    # phase writes four of the sixteen taps, and which four is read off the result, not off the tap table
    for name in ("wg3 phase (0,0) 64->64", "wg3 phase (1,0) 64->64", "wg3 phase (1,1) 64->64"):
        c, t = R.WG_BY_NAME[name], R.make_wgrad(name)
        x, dy_full = R.nchw(t["dy"].double()), R.nchw(t["xs"][0].double())
        w = torch.zeros((c["N"], 64, 4, 4), dtype=F64, requires_grad=True)
        g, = torch.autograd.grad(F.conv_transpose2d(x, w, stride=2, padding=1), w, dy_full)
        got, ref = t["grad"][0].double(), g.reshape(c["N"], 64, 16)
        written = ~torch.isnan(got)
        assert int(written.all(0).all(0).sum()) == 4 == int(written.any(0).any(0).sum()), name
        assert torch.equal(got[written], (ref + 0.0)[written]), name
        py, px = c["phase"]                                                  # taps of one phase share the parity of ky and kx
        ky, kx = written.any(0).any(0).nonzero().flatten() // 4, written.any(0).any(0).nonzero().flatten() % 4
        assert len(set((ky % 2).tolist())) == 1 and len(set((kx % 2).tolist())) == 1
    # a phase gradient writes 4 of the 16 taps
    t = R.make_wgrad("wg3 phase (1,0) 64->64")
    written = ~torch.isnan(t["grad"][0]).all(0).all(0)
    assert sorted(written.nonzero().flatten().tolist()) == sorted(t["tap_off"])
    keep = torch.ones(16, dtype=torch.bool)
    keep[t["tap_off"]] = False
    assert torch.equal(t["grad"][1][..., keep], t["prior"][..., keep])


# ------------------------------------------------------------------------------------------------------------------------------
# every GPU case: preconditions (asserted by the builders) and routes
# ------------------------------------------------------------------------------------------------------------------------------
def _build_forward(c):
    t = R.make_forward(c["name"])
    outs = R.forward_prefill(c, t)
    d, table, rows = R.forward_desc(c, t, outs)
    return t, d, table, rows


@pytest.mark.parametrize("name", [c["name"] for c in R.FWD_CASES])
def test_forward_case_builds_and_routes(name):
    c = R.FWD_BY_NAME[name]
    with _lib.knobs(**c["knobs"]):
        t, d, table, rows = _build_forward(c)
        info = R.assert_forward_route(c, d)
        if c["stats"]:
            assert rows == (info[6] if info[0] >= 3 else _lib.load().ksmi_conv_grid_m(C.byref(d))) >= 1
            # (the two <8, x> rows with an uneven last round need 8 patches of 512 pixels: conv_ref.py, "Grids")
            assert c["B"] * R.out_hw(c)[0] * R.out_hw(c)[1] <= 2000 or (c["uneven"] and info[2] == 8 and t["sq_max"] < 4e6)
        if c["uneven"]:
            tiles, gx, rounds, patch, ry, rx = R.persistent_grid(c, d, info)
            assert info[0] >= 3 and rounds > 1 and tiles % gx != 0 and ry and rx, (name, tiles, gx, rounds, patch)
        if c["gate"]:
            assert _lib.load().ksmi_conv_gate_supported(C.byref(d), DT[c["dtype"]]) == 1
    assert t["acc_max"] < R.LIMIT and (not c["stats"] or t["sq_max"] < R.LIMIT)
    for o, p in zip(t["outs"], R.forward_prefill(c, t)):
        assert o.shape == p.shape and o.dtype == c["dtype"]
    if c["ostride"]:
        assert float(t["outs"][0][..., c["N"]:].abs().max()) == 0.0
    if c["big"] and c["dtype"] == BF16:
        assert t["rounded"] * 10 >= t["outs"][0].numel() and t["ties"] > 0
    if c["route"][0] == 3 and (c["H"], c["W"]) == (31, 25) and c["stride"] == 1:
        assert c["H"] % d.TH and c["W"] % d.TW and d.TH * d.TW <= 256, "the last tile row and column are meant to be partial"
    if c["big"]:
        assert c["dtype"] == BF16
    # the table reaches what its comments promise
    assert len(table) == (sum(-(-x // (32 if c["dtype"] == BF16 else 16)) for x in c["cs"]))


def test_forward_table_coverage():
    """every generation, every igemm4 variant, the igemm3 tap and chunk counts, the chunk counts of igemm4"""
    gens, variants, ig3, ig4_chunks = set(), set(), set(), set()
    for c in R.FWD_CASES:
        nch = sum(-(-x // (32 if c["dtype"] == BF16 else 16)) for x in c["cs"])
        gens.add(c["route"][0])
        if c["route"][0] == 4:
            ig4_chunks.add(nch)
            if len(c["route"]) == 3:
                variants.add(tuple(c["route"][1:]))
        if c["route"][0] == 3:
            ig3.add((c["k"] * c["k"], nch))
    assert gens == {1, 2, 3, 4}
    assert variants == {(4, 4), (8, 4), (4, 2), (8, 2)}
    assert {2, 3, 5} <= ig4_chunks
    assert {(9, 1), (9, 2), (4, 1), (4, 2), (4, 4), (1, 2), (1, 4), (1, 8)} <= ig3
    # ... each of them, every igemm4 variant, the 2 x 2 phases and every 3 x 3 igemm3 row also with an uneven last round on ragged tiles
    un = [c for c in R.FWD_CASES if c["uneven"]]
    nchunks = lambda c: sum(-(-x // 32) for x in c["cs"])      # noqa: E731
    assert {(9, 1), (9, 2), (4, 1), (4, 2), (4, 4), (1, 2), (1, 4), (1, 8)} <= {(c["k"] ** 2, nchunks(c)) for c in un if c["route"][0] == 3}
    assert {tuple(c["route"][1:]) for c in un if c["route"][0] == 4} == {(4, 4), (8, 4), (4, 2), (8, 2)}
    assert sum(1 for c in un if c["phase"] is not None) == 2
    base = {c["name"] for c in R.FWD_CASES if c["route"][0] == 3 and c["k"] == 3 and not c["knobs"] and (c["H"], c["W"]) == (31, 25)}
    assert len(base) >= 16 and all(any(u["name"].startswith(b + " cus") for u in un) for b in base)
    assert {c["route"][0] for c in R.FWD_CASES if c["big"]} == {1, 2, 3, 4}
    assert {c["route"][0] for c in R.FWD_CASES if c["pack"] == "dgrad"} == {1, 2, 3, 4}
    assert {tuple(c["route"][1:]) for c in R.FWD_CASES if c["pack"] == "dgrad" and c["route"][0] == 4} == {(4, 4), (8, 4), (4, 2), (8, 2)}
    assert F32 in {c["dtype"] for c in R.FWD_CASES if c["pack"] == "dgrad"}


@pytest.mark.parametrize("name", [c["name"] for c in R.WG_CASES])
def test_wgrad_case_builds_and_routes(name):
    c, t = R.WG_BY_NAME[name], R.make_wgrad(name)
    with _lib.knobs(**c["knobs"]):
        for acc in (0, 1):
            d, ws = R.wgrad_desc(c, t, torch.empty(t["shape"], dtype=F32), acc)
            info = R.assert_wgrad_route(c, d)
            assert ws == _lib.load().ksmi_conv_wgrad_workspace(C.byref(d), DT[c["dtype"]]) > 0
    assert t["dw_max"] < R.LIMIT
    assert t["grad"][0].shape == t["grad"][1].shape == t["shape"] and t["grad"][0].dtype == F32
    if c["phase"] is None:
        assert not torch.isnan(t["grad"][0]).any()
    assert not torch.isnan(t["grad"][1]).any()


def test_wgrad_table_coverage():
    """every core reachable without a latched switch and all four reducers (+ the direct mode that needs none), both bias modes"""
    routes = [tuple(c["route"]) for c in R.WG_CASES]
    assert {r[0] for r in routes} == {R.PATCH, R.GEMM2, R.WGRAD3}
    assert {r[1] for r in routes} == {R.RED_NONE, R.RED_WGRAD3, R.RED_TREE, R.RED_TN_TR, R.RED_TN}
    assert {r[3] for r in routes if len(r) == 4} == {0, 1, 2}
    assert {tuple(sorted(c["knobs"].items())) for c in R.WG_CASES if c["knobs"]} == {
        tuple(sorted(R.W3(w, n).items())) for w, n in ((1, 2), (2, 3), (3, 4))}


def test_wgrad3_grid_knobs_change_the_split():
    """KSMI_WGRAD3_WGS really shrinks the grid of the knob cases: 1, 2, 3 slabs"""
    for wgs, nst in ((1, 2), (2, 3), (3, 4)):
        c = R.WG_BY_NAME[f"wg3 64->32 wgs{wgs} nst{nst}"]
        t = R.make_wgrad(c["name"])
        with _lib.knobs(**c["knobs"]):
            d, _ = R.wgrad_desc(c, t, torch.empty(t["shape"], dtype=F32), 0)
        assert d.nsplit == wgs


def test_compose_and_gaussian_cases_build():
    for case in R.COMPOSE_CASES:
        t = R.make_compose(case[0])
        assert t["dw"].shape == (case[5], case[4], 3, 3)
    for name in R.GAUSS_CASES:
        t = R.make_forward(name, True)
        assert torch.isfinite(t["ref"]).all() and R.FWD_BY_NAME[name]["stats"]
    assert {R.FWD_BY_NAME[n]["route"][0] for n in R.GAUSS_CASES} == {1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------------------------------------
# refusals of ksmi_conv_forward: decided on the host before anything is launched
# ------------------------------------------------------------------------------------------------------------------------------
def _refused(d, dtype, text):
    lib = _lib.load()
    rc = lib.ksmi_conv_forward(C.byref(d), DT[dtype], None)
    assert rc < 0 and text in lib.ksmi_last_error().decode(), (rc, lib.ksmi_last_error())
    return rc


def test_forward_refusals():
    # the gate epilogue on a descriptor that a tile kernel runs (a 14 x 14 map: too few patches for igemm4 at the default grid)
    c = dict(R.FWD_BY_NAME["ig4 gate accumulate 96->128"], knobs={})
    t, d, _, _ = _build_forward(c)
    assert R.forward_info(d, BF16)[0] == 2 and _lib.load().ksmi_conv_gate_supported(C.byref(d), DT[BF16]) == 0
    assert _refused(d, BF16, "gate epilogue") == -2
    # a statistics buffer sized for another kernel
    c = R.FWD_BY_NAME["ig2 small map 128->64"]
    t, d, _, rows = _build_forward(c)
    d.stats_rows = rows + 1
    assert _refused(d, BF16, "stats_rows") == -1
    # the epilogue extras on the first-generation kernel
    c = dict(R.FWD_BY_NAME["ig1 bf16 16+8+16->16"], extras=0.5)
    t = R.make_forward("ig1 bf16 16+8+16->16")
    t = dict(t, resid=t["outs"][0])
    d, _, _ = R.forward_desc(c, t, R.forward_prefill(c, t))
    assert R.forward_info(d, BF16)[0] == 1
    assert _refused(d, BF16, "alpha/resid/relu_out") == -2
