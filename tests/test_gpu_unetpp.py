"""GPU parity of the UNet++(resnet18) path (kurosiwo_amd/unetpp.py, unet_plan.UnetPlusPlusPlan) against the CPU restatement
tests/unetpp_ref.py, with the structure, batch and bounds of tests/test_gpu_unet.py (the project's yardstick for this encoder and block
type).  PARITY UNPINNED: segmentation-models-pytorch is not installed; the restatement is the only reference.
The CPU reference and one GPU step per precision are computed once and shared by the tests below."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unetpp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

CLASS_WEIGHTS = [0.3715753140309927, 14.009780283125977, 8.20405370357821]
B = 2
BLOCKS = [f"x_{d}_{l}" for l in range(4) for d in range(l + 1)] + ["x_0_4"]


def sar_like(name, shape):
    from oracle.seeded import seeded_tensor
    return seeded_tensor(name, shape).clamp_(-2.23, 5.75)


def build(precision):
    from kurosiwo_amd.unetpp import UnetPlusPlus
    from oracle.seeded import seeded_fill_
    model = UnetPlusPlus("resnet18", encoder_weights=None, in_channels=2, classes=3, precision=precision)
    sd = seeded_fill_(R.new_state_dict(2, 3))
    assert list(model.state_dict().keys()) == list(sd.keys())
    model.load_state_dict(sd)
    return model.cuda(), sd


def nchw(t):
    return t.float().cpu().permute(0, 3, 1, 2)


def relerr(a, b):
    return float((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-12))


@functools.lru_cache(maxsize=None)
def _batch():
    from oracle.seeded import seeded_labels
    return sar_like("unetpp.train.x", (B, 2, 224, 224)), seeded_labels("unetpp.train.lbl", (B, 224, 224))


@functools.lru_cache(maxsize=None)
def _reference():
    """the fp32 restatement's train step on the shared batch (read-only for every test)"""
    from oracle.seeded import seeded_fill_
    x, lbl = _batch()
    return R.loss_and_grads(seeded_fill_(R.new_state_dict(2, 3)), x, lbl, CLASS_WEIGHTS, grad_of=("f1",))


@functools.lru_cache(maxsize=None)
def _gpu_step(precision):
    """two identical train steps (forward, weighted cross entropy, backward) from the same state -> what the tests compare, on the CPU"""
    x, lbl = _batch()
    model, _ = build(precision)
    model.train()
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        logits = model(x.cuda())
        loss = torch.nn.functional.cross_entropy(logits, lbl.cuda(), weight=torch.tensor(CLASS_WEIGHTS, device="cuda"), ignore_index=3)
        loss.backward()
        torch.cuda.synchronize()
        runs.append((logits.detach().cpu(), float(loss), model.flat_grads.detach().cpu().clone()))
    plan = model.plan(B, 224, 224, True, True)
    named = {k: nchw(v) for k, v in plan.named.items()}
    df1 = nchw(plan.gbuf(plan.named["f1"]))
    grads = {k: p.grad.detach().float().cpu().clone() for k, p in model.named_parameters()}
    return {"runs": runs, "named": named, "df1": df1, "grads": grads}


def test_eval_forward():
    model, sd = build("fp32")
    model.eval()
    x = sar_like("unetpp.eval.x", (1, 2, 224, 224))
    with torch.no_grad():
        ref = R.unetpp_forward(sd, x, training=False)
        out = model(x.cuda())
    err = relerr(out.cpu(), ref)
    print("eval relerr", err)
    assert err < 1e-3
    margin = ref.topk(2, dim=1).values
    confident = (margin[:, 0] - margin[:, 1]) > 1e-3 * float(ref.abs().max())
    assert (out.argmax(1).cpu() == ref.argmax(1))[confident].all()


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_forward(precision):
    ref, got = _reference(), _gpu_step(precision)
    tol = 1e-3 if precision == "fp32" else 0.15
    errs = {k: relerr(got["named"][k], ref["inter"][k]) for k in [f"f{i}" for i in range(1, 6)] + BLOCKS}
    errs["logits"] = relerr(got["runs"][0][0], ref["logits"])
    print(precision, "forward relerr", errs)
    assert not {k: v for k, v in errs.items() if not v < tol}, errs


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_train_backward(precision):
    """the bounds of tests/test_gpu_unet.py (unmasked oracle: isolated ReLU flips perturb single gradients, hence l2 < 3e-2 per key in
    fp32; in bf16 the per-key cosine is a sanity bound only)"""
    ref, got = _reference(), _gpu_step(precision)
    dl = abs(got["runs"][0][1] - ref["loss"])
    coss, worst = [], {}
    for k, g in got["grads"].items():
        r = ref["grads"][k]
        if float(r.abs().max()) < 1e-12:
            continue
        cos = float((g.double() * r.double()).sum() / (g.double().norm() * r.double().norm() + 1e-30))
        coss.append(cos)
        l2 = float((g - r).double().norm() / (r.double().norm() + 1e-30))
        if precision == "fp32" and not l2 < 3e-2:
            worst[k] = l2
        if precision == "bf16" and not cos > 0.3:
            worst[k] = cos
    print(precision, "loss", got["runs"][0][1], "ref", ref["loss"], "median cos", float(np.median(coss)), "min cos", min(coss), "worst", worst)
    assert dl < (1e-3 if precision == "fp32" else 5e-2)
    assert float(np.median(coss)) > (0.9999 if precision == "fp32" else 0.75), float(np.median(coss))
    assert not worst, f"{precision}: {len(worst)}: {dict(list(worst.items())[:10])}"


def test_f1_gradient_sums_its_five_consumers():
    """d(f1) has five writers (the skips of x_0_3, x_1_3, x_2_3, x_3_3 and the stem's max pool): a missing "+=" drops a share.  The plan's
    buffer holds the gradient after the stem's ReLU mask, so both sides are compared on the GPU's active set."""
    ref, got = _reference(), _gpu_step("fp32")
    mask = (got["named"]["f1"] > 0).float()
    g, r = got["df1"] * mask, ref["inter_grads"]["f1"] * mask
    l2 = float((g - r).double().norm() / (r.double().norm() + 1e-30))
    print("d(f1) l2", l2)
    assert l2 < 3e-2


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_step_is_repeatable(precision):
    """two identical steps from the same state: bit-identical logits and gradients (the accumulate order is fixed)"""
    (l0, loss0, g0), (l1, loss1, g1) = _gpu_step(precision)["runs"]
    assert torch.equal(l0, l1) and loss0 == loss1 and torch.equal(g0, g1)


def _train_step(model, Bq, S, loss="cross_entropy", **kw):
    from kurosiwo_amd.trainer import SegTrainStep
    return SegTrainStep(model, Bq, loss, (1.0, 2.0, 3.0), image_size=(S, S), lr=1e-3, **kw)


def test_compiled_launch_list_equals_the_python_walk(monkeypatch):
    """as tests/test_gpu_graph.py::test_compiled_launch_list_equals_the_python_walk: the compiled list (typed thunks of the two new entry
    points included) gives the Python walk's trajectory bit for bit, weight gradients on the side stream"""
    from kurosiwo_amd import launch as sp
    from kurosiwo_amd.unetpp import UnetPlusPlus
    Bq, S = 4, 224
    g = torch.Generator().manual_seed(47)
    data = [(torch.randn(Bq, 2, S, S, generator=g), torch.randint(0, 3, (Bq, S, S), generator=g)) for _ in range(2)]
    out = []
    for fast in (False, True):
        monkeypatch.setattr(sp.LaunchList, "fast", fast)
        torch.manual_seed(5)
        m = UnetPlusPlus("resnet18", encoder_weights=None, in_channels=2, classes=3, precision="bf16").cuda().train()
        st = _train_step(m, Bq, S, overlap_wgrad=True, overlap_lanes=True, graph=False)
        losses = [st.step(x.cuda(), y.cuda()).clone() for x, y in data]
        torch.cuda.synchronize()
        assert (st.plan.bwd._compiled is not None) == fast and st._ss._runner is not None      # (one runner under both walks)
        names = [c[2] for c in st.plan.fwd.calls + st.plan.bwd.calls]
        assert "ksmi_upsample2_backward_acc" in names and "ksmi_affine_relu_upsample2" in names
        out.append((losses, m.flat_params.clone(), m.flat_grads.clone()))
    for a, b in zip(out[0][0], out[1][0]):
        assert torch.equal(a, b), (a.tolist(), b.tolist())
    assert torch.equal(out[0][2], out[1][2]) and torch.equal(out[0][1], out[1][1])


def test_fused_upsample_knob_off_gives_the_same_step(monkeypatch):
    """KSMI_UNETPP_FUSED_UP=0 (the two-launch pair, kept for the A/B) and the fused pass: bit-identical logits and gradients"""
    from kurosiwo_amd.unetpp import UnetPlusPlus
    g = torch.Generator().manual_seed(3)
    x, y = torch.randn(2, 2, 64, 64, generator=g), torch.randint(0, 3, (2, 64, 64), generator=g)
    out = []
    for knob in ("1", "0"):
        monkeypatch.setenv("KSMI_UNETPP_FUSED_UP", knob)
        torch.manual_seed(5)
        m = UnetPlusPlus("resnet18", encoder_weights=None, in_channels=2, classes=3, precision="bf16").cuda().train()
        logits = m(x.cuda())
        torch.nn.functional.cross_entropy(logits, y.cuda()).backward()
        torch.cuda.synchronize()
        names = [c[2] for c in m.plan(2, 64, 64, True, True).fwd.calls]
        assert ("ksmi_affine_relu_upsample2" in names) == (knob == "1")
        out.append((logits.detach().clone(), m.flat_grads.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.parametrize("loss", ["cross_entropy", "ce+dice", "dice", "iou", "focal"])
def test_seg_train_step_with_every_loss(loss):
    """SegTrainStep on the UNet++ plan with every loss of create_loss: finite loss, parameters move"""
    from kurosiwo_amd.unetpp import UnetPlusPlus
    g = torch.Generator().manual_seed(9)
    x, y = torch.randn(2, 2, 64, 64, generator=g), torch.randint(0, 3, (2, 64, 64), generator=g)
    torch.manual_seed(5)
    m = UnetPlusPlus("resnet18", encoder_weights=None, in_channels=2, classes=3, precision="bf16").cuda().train()
    st = _train_step(m, 2, 64, loss)
    before = m.flat_params.clone()              # (the arena moves to the device when the first plan is built)
    out = st.step(x.cuda(), y.cuda()).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(m.flat_params).all()
    assert not torch.equal(before, m.flat_params)


def test_main_entry_unetplusplus_end_to_end_tiny(tmp_path, monkeypatch):
    import shutil
    import main as entry
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shutil.copytree(os.path.join(root, "configs"), tmp_path / "configs")
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("KSMI_SYNTHETIC_TILES", "8,4,4")
    miou = entry.main(["--method", "unetplusplus", "--inputs", "post_event", "--batch_size", "4"])
    assert 0.0 <= miou <= 100.0
    assert (tmp_path / "checkpoints" / "UnetPlusPlus" / "resnet18").is_dir()        # create_checkpoint_directory: architecture / backbone / ...
