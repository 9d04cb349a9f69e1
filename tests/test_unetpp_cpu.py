"""UNet++ (kurosiwo_amd/unetpp.py) against its plain-torch restatement tests/unetpp_ref.py on the CPU: state-dict keys and order,
parameter count, the block table, and the restatement's own shape / mode behaviour.  Nothing here needs the GPU or the HIP library."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unetpp_ref as R  # noqa: E402

# (in, skip, out) of the eleven DecoderBlocks, written out: smp 0.3.2 UnetPlusPlusDecoder with encoder channels (c, 64, 64, 128, 256, 512)
# and decoder channels (256, 128, 64, 32, 16), in construction order
BLOCKS = [("x_0_0", (512, 256, 256)),
          ("x_0_1", (256, 256, 128)), ("x_1_1", (256, 128, 128)),
          ("x_0_2", (128, 192, 64)), ("x_1_2", (128, 128, 64)), ("x_2_2", (128, 64, 64)),
          ("x_0_3", (64, 256, 32)), ("x_1_3", (64, 192, 64)), ("x_2_3", (64, 128, 64)), ("x_3_3", (64, 64, 64)),
          ("x_0_4", (32, 0, 16))]


def _model(**kw):
    from kurosiwo_amd.unetpp import UnetPlusPlus
    return UnetPlusPlus("resnet18", encoder_weights=None, in_channels=2, classes=3, **kw)


def _expected_parameters(cin, classes):
    bn = lambda c: 2 * c
    n = 64 * cin * 49 + bn(64)                                   # stem
    c_in = 64
    for ch, stride in ((64, 1), (128, 2), (256, 2), (512, 2)):   # layer1..4, two BasicBlocks each
        for bi in range(2):
            n += ch * c_in * 9 + bn(ch) + ch * ch * 9 + bn(ch)
            if bi == 0 and (stride != 1 or c_in != ch):
                n += ch * c_in + bn(ch)
            c_in = ch
    for _, (ci, cs, co) in BLOCKS:
        n += co * (ci + cs) * 9 + bn(co) + co * co * 9 + bn(co)
    return n + classes * 16 * 9 + classes


def test_state_dict_keys_and_order():
    sd = R.new_state_dict(2, 3)
    msd = _model().state_dict()
    assert list(msd.keys()) == list(sd.keys())
    assert all(tuple(msd[k].shape) == tuple(sd[k].shape) and msd[k].dtype == sd[k].dtype for k in sd)
    blocks = [k.split(".")[2] for k in sd if k.startswith("decoder.blocks.") and k.endswith("conv1.0.weight")]
    assert blocks == [name for name, _ in BLOCKS]                 # outer loop l, inner loop d, then x_0_4
    enc = [k for k in sd if k.startswith("encoder.")]
    from oracle.unet_ref import new_state_dict as unet_sd
    assert enc == [k for k in unet_sd(2, 3) if k.startswith("encoder.")]


def test_parameter_count():
    want = _expected_parameters(2, 3)
    assert want == 15967603
    assert sum(p.numel() for p in _model().parameters()) == want
    assert sum(v.numel() for k, v in R.new_state_dict(2, 3).items() if not R.is_buffer(k)) == want


def test_block_table():
    from kurosiwo_amd.unetpp import block_table, forward_order
    assert list(block_table().items()) == BLOCKS
    assert list(R.block_channels().items()) == BLOCKS
    assert forward_order() == ["x_0_0", "x_1_1", "x_2_2", "x_3_3", "x_0_1", "x_1_2", "x_2_3", "x_0_2", "x_1_3", "x_0_3", "x_0_4"]


def test_constructor_refuses_what_unet_refuses():
    import pytest
    from kurosiwo_amd._lib import KsmiError
    for kw in (dict(encoder_name="resnet34"), dict(encoder_depth=4), dict(decoder_channels=(128, 64, 32, 16, 8)), dict(decoder_use_batchnorm=False),
               dict(activation="sigmoid"), dict(classes=9), dict(decoder_attention_type="scse")):
        args = dict(encoder_name="resnet18", encoder_weights=None, in_channels=2, classes=3)
        args.update(kw)
        from kurosiwo_amd.unetpp import UnetPlusPlus
        with pytest.raises(NotImplementedError):
            UnetPlusPlus(**args)
    with pytest.raises(KsmiError):
        _model_with_weights()


def _model_with_weights():
    from kurosiwo_amd.unetpp import UnetPlusPlus
    return UnetPlusPlus("resnet18", encoder_weights="imagenet", in_channels=2, classes=3)


def test_restatement_shape_and_modes():
    from oracle.seeded import seeded_fill_, seeded_tensor
    sd = seeded_fill_(R.new_state_dict(2, 3))
    x = seeded_tensor("unetpp.cpu.x", (2, 2, 64, 64))
    inter = {}
    with torch.no_grad():
        tr = R.unetpp_forward(sd, x, training=True, inter=inter)
        ev = R.unetpp_forward(sd, x, training=False)
    assert tuple(tr.shape) == tuple(ev.shape) == (2, 3, 64, 64)
    assert torch.isfinite(tr).all() and torch.isfinite(ev).all()
    assert not torch.allclose(tr, ev)
    for name, (_, _, co) in BLOCKS:
        l = int(name.split("_")[2])
        assert tuple(inter[name].shape) == (2, co, 4 << l, 4 << l), name


def test_factory_and_config():
    """initialize_segmentation_model builds it from configs/method/unetplusplus/unetplusplus.json with the unet branch's arguments"""
    from kurosiwo_amd.config import load_json5
    from kurosiwo_amd.model_utilities import initialize_segmentation_model
    from kurosiwo_amd.unetpp import UnetPlusPlus
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mc = load_json5(os.path.join(root, "configs/method/unetplusplus/unetplusplus.json"))
    ref = load_json5(os.path.join(root, "configs/method/unet/unet.json"))
    assert set(mc) == set(ref) and mc["architecture"] == "UnetPlusPlus" and mc["method"] == "unetplusplus"
    model = initialize_segmentation_model({"method": "unetplusplus", "num_channels": 2, "num_classes": 3, "device": "cpu"}, mc)
    assert isinstance(model, UnetPlusPlus) and model.in_channels == 2 and model.classes == 3
