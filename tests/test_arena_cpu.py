"""What every model class relies on in kurosiwo_amd.arena.ArenaModule, on CPU tensors: the arena survives load_state_dict and is
rebuilt (values kept, plan cache emptied) after nn.Module._apply replaced the parameter tensors; BatchNorm running statistics start at
(0, 1) and the counters at 0; parameter views are aligned to ARENA_ALIGN floats; PlanFn hands autograd one None per forward argument."""
import pytest
import torch


def _snunet():
    from kurosiwo_amd.snunet import SNUNet_ECAM
    return SNUNet_ECAM(2, 3, base_channel=8, precision="fp32")


def _siam():
    from kurosiwo_amd.fcsiam import SiamUnet_conc
    return SiamUnet_conc(2, 3, precision="fp32")


def _families():
    from kurosiwo_amd.bitcd import define_G
    from kurosiwo_amd.changeformer import ChangeFormerV6
    from kurosiwo_amd.fcsiam import SiamUnet_diff
    from kurosiwo_amd.floodvit import FinetunerSegmentation, ViT
    from kurosiwo_amd.mae import MAE
    from kurosiwo_amd.unet import Unet

    def vit():
        return ViT(image_size=32, patch_size=16, num_classes=10, dim=1024, depth=1, heads=2, mlp_dim=64, channels=2)
    yield "snunet", _snunet()
    yield "changeformer", ChangeFormerV6(input_nc=2, output_nc=3, decoder_softmax=True, embed_dim=32)
    yield "floodvit", FinetunerSegmentation(vit(), {"decoder": True, "num_classes": 3, "image_size": 32})
    yield "mae", MAE(encoder=vit(), decoder_dim=64, configs={"image_size": 32})
    yield "unet", Unet("resnet18", encoder_weights=None, in_channels=2, classes=3)
    yield "siam-conc", _siam()
    yield "siam-diff", SiamUnet_diff(2, 3)
    yield "bit-cd resnet", define_G({"net_G": "base_resnet18"}, 2)
    yield "bit-cd transformer", define_G({"net_G": "base_transformer_pos_s4"}, 2)


def test_every_model_class_is_an_arena_module():
    from kurosiwo_amd.arena import ArenaModule
    for name, m in _families():
        assert ArenaModule in type(m).__mro__, name


@pytest.mark.parametrize("make", [_snunet, _siam])
def test_arena_survives_load_and_is_rebuilt_after_apply(make):
    torch.manual_seed(3)
    m = make()
    sd = {k: torch.randn(v.shape) if v.is_floating_point() else torch.full_like(v, 7) for k, v in m.state_dict().items()}
    m._plans["stale"] = object()
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert m._arena_ok() and "stale" in m._plans                  # copy_ into the views: same arena, the plans' pointers still hold
    base = m.flat_params.data_ptr()
    m._ensure_arena()
    assert m.flat_params.data_ptr() == base and "stale" in m._plans
    # what nn.Module._apply (.to(device), .float(), ...) does: every tensor replaced by a fresh one
    for p in m.parameters():
        p.data = p.data.clone()
    for mod in m.modules():
        for k, b in mod._buffers.items():
            mod._buffers[k] = b.clone()
    assert not m._arena_ok()
    m._ensure_arena()
    assert m._arena_ok() and m._plans == {}
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k]), k
    for k in m._pspec:
        assert m._param_obj(k).data_ptr() == m.flat_params.data_ptr() + 4 * m._poff[k], k
    for k in m._bspec:
        assert m._buffer_obj(k).data_ptr() == m.flat_buffers.data_ptr() + 4 * m._boff[k], k
    for k in m._ispec:
        assert m._buffer_obj(k).data_ptr() == m.flat_counters.data_ptr() + 8 * m._ioff[k], k


def test_cached_plan_builds_once_per_key_on_a_valid_arena():
    m = _siam()
    built = []
    assert m._cached_plan("a", lambda: built.append("a") or "plan a") == "plan a"
    assert m._cached_plan("a", lambda: built.append("a again") or "other") == "plan a"
    assert built == ["a"]
    for p in m.parameters():
        p.data = p.data.clone()
    assert m._cached_plan("a", lambda: "rebuilt") == "rebuilt" and m._arena_ok()


def test_fresh_running_statistics_and_counters():
    for name, m in _families():
        n = 0
        for k, v in m.state_dict().items():
            if k.endswith("running_var"):
                assert torch.equal(v, torch.ones_like(v)), (name, k)
            elif k.endswith(("running_mean", "num_batches_tracked")):
                assert torch.equal(v, torch.zeros_like(v)), (name, k)
            else:
                continue
            n += 1
        assert n == len(m._bspec) + len(m._ispec), name
        assert all(k.endswith(("running_mean", "running_var")) for k in m._bspec), name
        assert int(m.flat_grads.abs().max()) == 0


def test_parameter_views_are_aligned_per_class():
    for name, m in _families():
        align = 4 if name == "snunet" else 8
        assert type(m).ARENA_ALIGN == align, name
        assert all(o % align == 0 for o in m._poff.values()), name
        assert m.flat_params.numel() % align == 0 and m.flat_grads.numel() == m.flat_params.numel(), name
        assert all(o % 4 == 0 for o in m._boff.values()), name
    m = _snunet()                                                   # the last view (conv_final.bias, 3 floats) is padded to 4, not 8
    assert m.flat_params.numel() == m._poff["conv_final.bias"] + 4


class _StubPlan:
    def __init__(self):
        self.seen, self.dout = None, None

    def run_forward(self, *inputs):
        self.seen = inputs
        return sum(x.sum() for x in inputs if x is not None).reshape(1)

    def run_backward(self, dout):
        self.dout = dout


@pytest.mark.parametrize("inputs", [(torch.ones(2), torch.ones(3)), (torch.ones(2), torch.ones(3), None)])
def test_planfn_backward_returns_one_none_per_forward_argument(inputs):
    from kurosiwo_amd.arena import PlanFn
    m, plan = _siam(), _StubPlan()

    class Ctx:
        pass
    ctx = Ctx()
    out = PlanFn.forward(ctx, m._grad_anchor(torch.device("cpu")), m, plan, *inputs)
    assert plan.seen == inputs and float(out) == 5.0
    grads = PlanFn.backward(ctx, torch.ones(1))
    assert grads == (None,) * (3 + len(inputs))                     # anchor, model, plan, then the inputs

    # and through autograd itself (which checks the count), by the path every forward() takes
    m, plan = _siam(), _StubPlan()
    out = m._apply_plan(plan, True, *inputs)
    assert out.requires_grad and plan.seen == inputs
    (2 * out).sum().backward()
    assert torch.equal(plan.dout, torch.full((1,), 2.0))
    for k in m._pspec:
        assert m._param_obj(k).grad.data_ptr() == m.flat_grads.data_ptr() + 4 * m._poff[k], k
    with torch.no_grad():
        assert not m._wants_grad()
    assert m._wants_grad() and not m._apply_plan(plan, False, *inputs).requires_grad
