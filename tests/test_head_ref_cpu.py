"""The float64 oracles of tests/head_ref.py against the float64 autograd of its own chain function (the whole ECAM head written from
the formula) on small random data, and every case of tests/test_gpu_head.py built here: building a case runs its oracle, whose
exactness assertions, and its builder, whose coverage assertions (rounding of intra, tie relations, scatter collisions, unique maxima
of the chain inputs), fail here, without a GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_ref as H  # noqa: E402

F64, F32, BF16 = torch.float64, torch.float32, torch.bfloat16
IDS = H.DTYPE_IDS


def _close(a, b, tol=1e-11):
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------------------------------------
# the oracles against the chain
# ------------------------------------------------------------------------------------------------------------------------------
def _small(B=2, HW=37, Cc=16, seed=300):
    xs = [H.gauss((B, HW, Cc), seed + s) for s in range(4)]
    Hh = Cc // 4
    p = {"w1": H.gauss((Hh, 4 * Cc), seed + 4, 0.2), "w2": H.gauss((4 * Cc, Hh), seed + 5, 0.5), "v1": H.gauss((Hh, Cc), seed + 6, 0.3),
         "v2": H.gauss((Cc, Hh), seed + 7, 0.5), "wf": H.gauss((H.NCLS, 4 * Cc), seed + 8, 0.2), "bias": H.gauss((H.NCLS,), seed + 9)}
    return xs, p, H.gauss((B, H.NCLS, HW), seed + 10)


def _oracle_forward(xs, p):
    pl = H.pool(xs, F64, exact=False)
    m = H.mlp(pl["avg"], pl["mx"], p["w1"], p["w2"], p["v1"], p["v2"], exact=False)
    return pl, m, H.final_forward(xs, m["ca"], m["ca1"], p["wf"], p["bias"], exact=False)


def test_forward_oracles_compose_to_the_chain():
    xs, p, _ = _small()
    _, m, logits = _oracle_forward(xs, p)
    _close(logits, H.chain(xs, p))
    assert bool((m["hidden"] == 0).any()) and bool((m["hidden"] > 0).any())       # both sides of the ReLU


def test_backward_oracles_compose_to_the_chain_autograd():
    xs, p, dl = _small(seed=400)
    gx = [x.clone().requires_grad_(True) for x in xs]
    gp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    H.chain(gx, gp).backward(dl)
    pl, m, _ = _oracle_forward(xs, p)
    r = H.backward_reduce(xs, dl, m["ca"], m["ca1"], p["wf"], exact=False)
    _close(r["dwf"], gp["wf"].grad)
    _close(r["dbias"], gp["bias"].grad)
    b = H.mlp_backward(pl["avg"], pl["mx"], m["hidden"], m["ca"], m["ca1"], r["dca"], r["dca1"], p["w1"], p["w2"], p["v1"], p["v2"], exact=False)
    for ours, name in (("gw1", "w1"), ("gw2", "w2"), ("gv1", "v1"), ("gv2", "v2")):
        _close(b[ours], gp[name].grad)
    dx = H.backward_dx(dl, m["ca"], p["wf"], b["davg"], b["dmax"], pl["argmax"], F64, exact=False)
    for s in range(4):
        _close(dx["dx"][s], gx[s].grad)


def test_chain_is_the_module_formula():
    """the chain against ChannelAttention and the fusion written with torch's own pooling modules (NCHW, tie-free data)"""
    xs, p, _ = _small(B=2, HW=6 * 7, Cc=16, seed=500)
    nchw = [x.permute(0, 2, 1).reshape(2, 16, 6, 7) for x in xs]

    def attention(t, fc1, fc2):
        avg, mx = torch.nn.functional.adaptive_avg_pool2d(t, 1).flatten(1), torch.nn.functional.adaptive_max_pool2d(t, 1).flatten(1)
        return torch.sigmoid(torch.relu(avg @ fc1.T) @ fc2.T + torch.relu(mx @ fc1.T) @ fc2.T)[:, :, None, None]
    out = torch.cat(nchw, 1)
    intra = torch.sum(torch.stack(nchw), dim=0)
    out = attention(out, p["w1"], p["w2"]) * (out + attention(intra, p["v1"], p["v2"]).repeat(1, 4, 1, 1))
    logits = torch.nn.functional.conv2d(out, p["wf"][:, :, None, None], p["bias"])
    _close(H.chain(xs, p), logits.flatten(2))


def test_pool_oracle_tie_rule_and_rounding():
    """the lowest pixel index among equal maxima; intra is rounded to the activation dtype before it is pooled"""
    x = torch.tensor([1.0, 3.0, 3.0, -2.0, 3.0], dtype=F64).view(1, 5, 1)
    z = torch.zeros_like(x)
    r = H.pool([x, z, z, z], F32)
    assert r["argmax"].flatten().tolist() == [1, 0, 0, 0, 1] and r["mx"].flatten().tolist() == [3.0, 0.0, 0.0, 0.0, 3.0]
    assert r["avg"].flatten().tolist() == [1.6, 0.0, 0.0, 0.0, 1.6]
    a, b = torch.tensor([200.0, 257.0], dtype=F64).view(1, 2, 1), torch.tensor([59.0, 0.0], dtype=F64).view(1, 2, 1)
    r = H.pool([a, b, torch.zeros_like(a), torch.zeros_like(a)], BF16)        # intra: 259 -> 260 in bf16, 257 -> 256
    assert r["mx"][0, 4].item() == 260.0 and r["argmax"][0, 4].item() == 0 and r["avg"][0, 4].item() == 258.0
    assert H.pool_unrounded([a, b, torch.zeros_like(a), torch.zeros_like(a)])["mx"][0, 4].item() == 259.0


def test_pair_relations_follow_the_thread_map():
    """C = 64 fp32: 16 channel vectors, 16 pixel lanes, 4 per wave; HW = 1000: 63 pixels per split"""
    rel = H.pair_relations(1000, 64, F32)
    assert rel[0, 16].item() == 0 and rel[0, 1].item() == 1 and rel[1, 16].item() == 2 and rel[0, 4].item() == 3 and rel[62, 63].item() == 4
    assert rel[5, 5].item() == -1 and rel[7, 3].item() == -1
    assert H.feasible_relations(1, 16, F32) == [] and H.feasible_relations(5, 16, F32) == ["splits"]
    assert H.feasible_relations(1000, 16, F32) == ["lanes", "waves", "splits"]          # 64 pixel lanes > 63 pixels: no thread sees two
    assert H.feasible_relations(1024, 64, F32) == H.RELATIONS


def _emulate_dx_fp32(d, dtype):
    """ecam_bwd_dx_kernel and the scatter in the kernel's own fp32 order, on the CPU"""
    dl, ca, wf, davg, dmax = (d[k].float() for k in ("dl", "ca", "wf", "davg", "dmax"))
    B, _, HW = dl.shape
    Cc = ca.shape[1] // 4
    weff = wf[None] * ca[:, None, :]
    cst = (davg[:, :4 * Cc] + davg[:, 4 * Cc:].repeat(1, 4)) * (torch.tensor(1.0, dtype=F32) / torch.tensor(float(HW), dtype=F32))
    a = cst[:, None, :].expand(B, HW, 4 * Cc).clone()
    for k in range(H.NCLS):
        a = a + weff[:, k, None, :] * dl[:, k, :, None]
    v = a.to(dtype)
    bi, ci, am = torch.arange(B)[:, None], torch.arange(Cc)[None, :], d["argmax"].long()
    for s, grp in [(s, s) for s in range(4)] + [(s, 4) for s in range(4)]:
        pix, g = am[:, grp * Cc:(grp + 1) * Cc], dmax[:, grp * Cc:(grp + 1) * Cc]
        v[bi, pix, s * Cc + ci] = (v[bi, pix, s * Cc + ci].float() + g).to(dtype)
    return [v[..., s * Cc:(s + 1) * Cc] for s in range(4)]


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
@pytest.mark.parametrize("HW", [5, 64, 1000])
def test_dx_oracle_against_an_fp32_emulation(HW, dtype):
    """power-of-two HW: the same bits; otherwise inside the bound (which is then not vacuous: the emulation does differ from float64)"""
    d = H.case_dx((16, dtype, 3, HW))
    got = _emulate_dx_fp32(d, dtype)
    worst, differs = 0.0, False
    for s in range(4):
        ref, bound = d["ref"]["dx"][s], d["ref"]["bound"]
        if bound is None:
            assert torch.equal(got[s].double(), ref)
        else:
            worst = max(worst, H.ratio(got[s], ref, bound[s]))
            differs = differs or not torch.equal(got[s].double(), ref)
    assert worst <= 1.0, worst
    assert differs == (not H.is_pow2(HW))


def test_sigmoid_bound_admits_torch_fp32():
    """the bound of ca is a few fp32 ulps: torch's own fp32 sigmoid of the exact argument lies inside twice of it, a wrong argument far outside"""
    d = H.case_mlp(64, 3)
    r = d["ref"]
    assert H.ratio(torch.sigmoid(r["z"].float()), r["ca"], 2 * r["ca_bound"]) <= 1.0
    assert H.ratio(torch.sigmoid((r["z"] * (1 + 2.0 ** -20)).float()), r["ca"], r["ca_bound"]) > 1.0
    assert float(r["z"].abs().max()) < 30 and float(r["z"].abs().mean()) > 0.1                  # neither saturated nor all zero


# ------------------------------------------------------------------------------------------------------------------------------
# every case of the GPU file builds
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_gpu_cases_are_exactly_computable(dtype):
    cases = [c for c in H.CASES if c[1] == dtype]
    assert len(cases) == 32 and {c[2] for c in cases} == {1, 3}
    for c in cases:
        Cc, _, B, HW = c
        H.case_pool("rounding", c)
        _, ref = H.case_pool("ties", c)
        assert all(ref["coverage"][name] > 0 for name in ref["feasible"]), (c, ref["coverage"])
        assert ref["feasible"] or HW == 1
        top = ref["all5"] == ref["all5"].max(1, keepdim=True).values
        assert HW == 1 or not bool(top.all(1).any())                     # no channel is constant: something is strictly lower
        H.case_final(c)
        d = H.case_dx(c)
        assert 0 <= int(d["argmax"].min()) and int(d["argmax"].max()) < HW
        _, _, nan = H.make_pool_nan(B, HW, Cc, dtype)
        assert int(nan.sum()) == 2


def test_gpu_cases_without_a_dtype_are_exactly_computable():
    for Cc, B in H.MLP_CASES:
        r = H.case_mlp(Cc, B)["ref"]
        assert bool((r["hidden"] == 0).any()) and bool((r["hidden"] > 0).any())
        assert float(r["z"].abs().max()) < 30 and float(r["z1"].abs().max()) < 30
        b = H.case_mlp_backward(Cc, B)["ref"]
        assert bool((b["dh"] != 0).any()) and bool((b["davg"] != b["dmax"]).any())
    H.case_final(H.GRID_STRIDE_CASE, backward=False)


def test_every_relation_is_met_somewhere():
    """over the cases of a dtype each of the five tie relations is feasible, hence (by the builder's assertion) covered"""
    for dtype in H.DTYPES:
        seen = set()
        for Cc, dt, _, HW in H.CASES:
            if dt == dtype:
                seen.update(H.feasible_relations(HW, Cc, dtype))
        assert seen == set(H.RELATIONS), seen


@pytest.mark.parametrize("dtype", H.DTYPES, ids=IDS)
def test_chain_inputs_have_unique_maxima(dtype):
    d = H.make_chain(dtype)
    all5 = H.pool([x.double() for x in d["x"]], dtype, exact=False)["all5"]
    top = all5 == all5.max(1, keepdim=True).values
    assert bool((top.sum(1) == 1).all()) and d["gap"] >= 0.25
    ref64, cpu32 = H.chain_reference(d, dtype, F64), H.chain_reference(d, dtype, F32)
    for name in ref64:
        out_dtype = dtype if name.startswith("dx") else F32
        tol = H.chain_tolerance(ref64, cpu32, name, out_dtype)
        assert 0 < tol < 0.05 * float(ref64[name].abs().max()), (name, tol)     # the tolerance of the GPU test is far below a missing term
