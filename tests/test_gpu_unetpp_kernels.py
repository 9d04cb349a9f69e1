"""The two glue kernels of the UNet++ plan (csrc/tokens.hip): ksmi_upsample2_backward_acc against avg_pool2d * 4 on small-integer data
(every sum is exact in fp32 and in bf16, so the assertions are bit-equality) and ksmi_affine_relu_upsample2 against the two-launch
pair it replaces, ksmi_affine(relu=1) + ksmi_upsample2_forward(relu=0), bit for bit.  Every output lives between guard words."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, h, w, C): one 16-byte bf16 vector per pixel at odd sizes; odd sizes with several vectors (two workgroups in fp32); several workgroups in both
SHAPES = [(2, 3, 3, 8), (1, 5, 7, 48), (2, 6, 10, 64)]
DTYPES = [torch.bfloat16, torch.float32]
GUARD = 64


def _ints(shape, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, shape, generator=g).to(dtype).cuda()


def _guarded(shape, dtype, fill):
    """a tensor of `shape` inside a flat buffer with GUARD sentinel elements on either side -> (view, check)"""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), 77.0, dtype=dtype, device="cuda")
    view = flat[GUARD:GUARD + n].view(shape)
    view.fill_(fill)

    def check():
        assert (flat[:GUARD] == 77.0).all() and (flat[GUARD + n:] == 77.0).all(), "write outside the tensor"
    return view, check


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample2_backward_acc(shape, dtype, accumulate, relu):
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import DT, stream_ptr
    B, h, w, Cc = shape
    lib = _lib.load()
    dy = _ints((B, 2 * h, 2 * w, Cc), 1, dtype)
    xpre = _ints((B, h, w, Cc), 2, dtype)
    prior = _ints((B, h, w, Cc), 3, dtype)
    dx, check = _guarded((B, h, w, Cc), dtype, float("nan"))
    if accumulate:
        dx.copy_(prior)
    _lib.check(lib.ksmi_upsample2_backward_acc(dy.data_ptr(), xpre.data_ptr() if relu else None, dx.data_ptr(), accumulate, B, h, w, Cc, relu,
                                               DT[dtype], stream_ptr()), "upsample2_backward_acc")
    torch.cuda.synchronize()
    want = torch.nn.functional.avg_pool2d(dy.float().permute(0, 3, 1, 2), 2).mul(4).permute(0, 2, 3, 1)
    if relu:
        want = want * (xpre.float() > 0)
    if accumulate:
        want = want + prior.float()
    check()
    assert torch.isfinite(dx.float()).all()                      # accumulate = 0 never reads the NaN-filled destination
    assert torch.equal(dx.float(), want)


def test_upsample2_backward_acc_refuses_bad_arguments():
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import DT, stream_ptr
    lib = _lib.load()
    t = torch.zeros(2 * 4 * 4 * 8, dtype=torch.bfloat16, device="cuda")
    assert lib.ksmi_upsample2_backward_acc(t.data_ptr(), None, t.data_ptr(), 0, 1, 2, 2, 4, 0, DT[torch.bfloat16], stream_ptr()) != 0     # C % 8
    assert lib.ksmi_upsample2_backward_acc(t.data_ptr(), None, t.data_ptr(), 0, 1, 2, 2, 8, 1, DT[torch.bfloat16], stream_ptr()) != 0     # relu without x_pre
    assert lib.ksmi_affine_relu_upsample2(t.data_ptr(), None, None, t.data_ptr(), t.data_ptr(), 1, 2, 2, 8, DT[torch.bfloat16], stream_ptr()) != 0


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_affine_relu_upsample2_equals_the_pair(shape, dtype):
    from kurosiwo_amd import _lib
    from kurosiwo_amd.runtime import DT, stream_ptr
    B, h, w, Cc = shape
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    z = torch.randn((B, h, w, Cc), generator=g).mul(3).to(dtype).cuda()
    scale = torch.randn(Cc, generator=g).cuda()
    shift = torch.randn(Cc, generator=g).cuda()
    y0, c0 = _guarded((B, h, w, Cc), dtype, float("nan"))
    U0, c1 = _guarded((B, 2 * h, 2 * w, Cc), dtype, float("nan"))
    y1, c2 = _guarded((B, h, w, Cc), dtype, float("nan"))
    U1, c3 = _guarded((B, 2 * h, 2 * w, Cc), dtype, float("nan"))
    st = stream_ptr()
    _lib.check(lib.ksmi_affine(z.data_ptr(), scale.data_ptr(), shift.data_ptr(), y0.data_ptr(), B * h * w, Cc, 1, C.c_float(1.0), DT[dtype], st), "affine")
    _lib.check(lib.ksmi_upsample2_forward(y0.data_ptr(), U0.data_ptr(), B, h, w, Cc, 0, DT[dtype], st), "upsample2_forward")
    _lib.check(lib.ksmi_affine_relu_upsample2(z.data_ptr(), scale.data_ptr(), shift.data_ptr(), y1.data_ptr(), U1.data_ptr(), B, h, w, Cc, DT[dtype], st),
               "affine_relu_upsample2")
    torch.cuda.synchronize()
    for c in (c0, c1, c2, c3):
        c()
    assert torch.equal(_bits(y1), _bits(y0))
    assert torch.equal(_bits(U1), _bits(U0))
    # (and the pair itself is what it says: the stored y, repeated 2 x 2)
    ref = torch.relu(z.float() * scale + shift)
    # (fp32: a fused multiply-add against torch's two roundings differs by an ulp of the product, |z * scale| < ~100 here)
    assert torch.allclose(y0.float(), ref, rtol=2 ** -7 if dtype == torch.bfloat16 else 1e-6, atol=2e-5)
    assert torch.equal(_bits(U0), _bits(y0.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)))
