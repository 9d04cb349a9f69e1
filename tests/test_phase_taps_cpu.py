"""The 2x2 phase tap tables of the stride-2 (de)convolutions (runtime.phase_taps_k4s2 / phase_taps_k3s2: every plan's phase loops read
them) against the closed forms of their derivation, and against the stride-2 operator they decompose, computed by torch on the CPU."""
import pytest
import torch
import torch.nn.functional as F

from kurosiwo_amd.runtime import phase_taps_k3s2, phase_taps_k4s2

PHASES = [(py, px) for py in range(2) for px in range(2)]


@pytest.mark.parametrize("py,px", PHASES)
def test_k4s2_closed_forms(py, px):
    fwd = [(3 - 2 * a if py == 0 else 2 - 2 * a) * 4 + (3 - 2 * b if px == 0 else 2 - 2 * b) for a in range(2) for b in range(2)]
    bwd = [(2 * a if py else 1 + 2 * a) * 4 + (2 * b if px else 1 + 2 * b) for a in range(2) for b in range(2)]
    assert phase_taps_k4s2(py, px, True) == fwd
    assert phase_taps_k4s2(py, px, False) == bwd


def test_k4s2_tables():
    assert [phase_taps_k4s2(py, px, True) for py, px in PHASES] == [[15, 13, 7, 5], [14, 12, 6, 4], [11, 9, 3, 1], [10, 8, 2, 0]]
    assert [phase_taps_k4s2(py, px, False) for py, px in PHASES] == [[5, 7, 13, 15], [4, 6, 12, 14], [1, 3, 9, 11], [0, 2, 8, 10]]
    for transposed in (True, False):                      # the four phases share out the 16 taps
        assert sorted(t for py, px in PHASES for t in phase_taps_k4s2(py, px, transposed)) == list(range(16))


def test_k3s2_tables():
    k = lambda p, a: (1 if a == 0 else -1) if p == 0 else (2 if a == 0 else 0)
    for py, px in PHASES:
        want = [-1 if k(py, a) < 0 or k(px, b) < 0 else k(py, a) * 3 + k(px, b) for a in range(2) for b in range(2)]
        assert phase_taps_k3s2(py, px) == want
    assert [phase_taps_k3s2(py, px) for py, px in PHASES] == [[4, -1, -1, -1], [5, 3, -1, -1], [7, -1, 1, -1], [8, 6, 2, 0]]
    assert sorted(t for py, px in PHASES for t in phase_taps_k3s2(py, px) if t >= 0) == list(range(9))


def _phase_conv(src, w, taps, K, pad_y, pad_x):
    """2x2 stride-1 convolution of src [1, Ci, H, W] with taps (a, b) -> w[:, :, tap // K, tap % K] (w as [Co][Ci][K][K]); -1 = no tap"""
    H, W = src.shape[2:]
    p = F.pad(src, (1, 1, 1, 1))
    out = torch.zeros(1, w.shape[0], H, W, dtype=src.dtype)
    for a in range(2):
        for b in range(2):
            t = taps[a * 2 + b]
            if t < 0:
                continue
            win = p[:, :, 1 - pad_y + a:1 - pad_y + a + H, 1 - pad_x + b:1 - pad_x + b + W]
            out += torch.einsum("oc,bchw->bohw", w[:, :, t // K, t % K], win)
    return out


def test_phases_compose_the_stride2_operators():
    torch.manual_seed(5)
    H, W, Ci, Co = 5, 6, 3, 4
    x = torch.randn(1, Ci, H, W, dtype=torch.float64)
    wt = torch.randn(Ci, Co, 4, 4, dtype=torch.float64)                    # ConvTranspose2d(k4, s2, p1) weight [in][out][ky][kx]
    ref = F.conv_transpose2d(x, wt, stride=2, padding=1)
    out = torch.zeros_like(ref)
    for py, px in PHASES:
        out[:, :, py::2, px::2] = _phase_conv(x, wt.transpose(0, 1), phase_taps_k4s2(py, px, True), 4, 1 - py, 1 - px)
    torch.testing.assert_close(out, ref)
    # its input gradient: a 4x4 stride-2 convolution of dOut, as 2x2 convolutions over the parity sub-images of dOut
    dout = torch.randn(1, Co, 2 * H, 2 * W, dtype=torch.float64)
    ref = F.conv2d(dout, wt, stride=2, padding=1)
    dx = sum(_phase_conv(dout[:, :, py::2, px::2], wt, phase_taps_k4s2(py, px, False), 4, py, px) for py, px in PHASES)
    torch.testing.assert_close(dx, ref)
    # input gradient of Conv2d(k3, s2, p1) = ConvTranspose2d(k3, s2, p1, output_padding 1) of dy
    w3 = torch.randn(Co, Ci, 3, 3, dtype=torch.float64)
    dy = torch.randn(1, Co, H, W, dtype=torch.float64)
    ref = F.conv_transpose2d(dy, w3, stride=2, padding=1, output_padding=1)
    dx = torch.zeros_like(ref)
    for py, px in PHASES:
        dx[:, :, py::2, px::2] = _phase_conv(dy, w3.transpose(0, 1), phase_taps_k3s2(py, px), 3, 0, 0)
    torch.testing.assert_close(dx, ref)
