"""The few-channel data gradient of the 7x7 stems (lwg_conv2d_backward_data: stride 1, k 7, pad 3, Cin == 8,
Cout % 64 == 0; csrc/train.hip, stem_dgrad_kernel) against fp64 autograd of F.conv2d.

The cycle pass of post-personalisation feeds the first pass's image into both stems of a second pass (reference:
models/imitator.py:384-406), so its backward needs d(conv)/d(input) of Conv2d(8 <- 6 padded, 64, 7, 1, 3)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, H, W): smaller than a tile with every tap clipped; odd, one past a tile edge; several tiles with ragged edges; whole tiles
SHAPES = [(1, 7, 7), (2, 9, 33), (3, 24, 40), (1, 64, 64)]
COUT = 64


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-12)


def _case(N, H, W, cout=COUT):
    g = torch.Generator().manual_seed(100 * H + W)
    w = torch.randn(cout, 8, 7, 7, generator=g) * 0.05
    w[:, 6:] = 0                                      # the stem's input has 6 real channels, padded to 8
    dy = torch.randn(N, cout, H, W, generator=g)
    x = torch.zeros(N, 8, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=1, padding=3).backward(dy.double())
    return dy.permute(0, 2, 3, 1).contiguous().cuda(), w.cuda(), x.grad.permute(0, 2, 3, 1)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_stem_data_gradient(N, H, W):
    from impersonator_amd import ops
    dy, w, ref = _case(N, H, W)
    dx = ops.conv2d_backward_data(dy, w, (N, H, W, 8), 1, 3)
    assert tuple(dx.shape) == (N, H, W, 8)
    rel = _rel(dx.cpu().double(), ref)
    print("stem dgrad (%d,%d,%d): rel %.3g" % (N, H, W, rel))
    assert rel < 1e-5                                 # fp32 sums of 3136 products (test_heads_ops' bound)
    assert float(dx[..., 6:].abs().max()) == 0.0      # zero filter columns give exact zeros
    # exact fp32 whatever the descriptor's precision says, and no atomics: the same bits every time
    assert torch.equal(ops.conv2d_backward_data(dy, w, (N, H, W, 8), 1, 3, precision="bf16x3"), dx)
    assert torch.equal(ops.conv2d_backward_data(dy, w, (N, H, W, 8), 1, 3), dx)


def test_stem_data_gradient_wider_layer():
    """Cout = 128: sixteen channel chunks, every filter column live."""
    from impersonator_amd import ops
    g = torch.Generator().manual_seed(7)
    N, H, W, cout = 2, 20, 35, 128
    w = torch.randn(cout, 8, 7, 7, generator=g) * 0.05
    dy = torch.randn(N, cout, H, W, generator=g)
    x = torch.zeros(N, 8, H, W, dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), None, stride=1, padding=3).backward(dy.double())
    dx = ops.conv2d_backward_data(dy.permute(0, 2, 3, 1).contiguous().cuda(), w.cuda(), (N, H, W, 8), 1, 3)
    assert _rel(dx.cpu().double(), x.grad.permute(0, 2, 3, 1)) < 1e-5      # 6272 products; the same bound holds


def test_neighbouring_shapes_stay_refused():
    """Only k 7, Cin 8, Cout % 64 == 0 is the new case: what was refused next to it stays refused, with its message."""
    from impersonator_amd import _lib, ops
    z = lambda *s: torch.zeros(*s, device="cuda")
    for cout, k in ((32, 7), (64, 5), (64, 3)):
        with pytest.raises(_lib.LwgError, match="multiple of 64 output channels"):
            ops.conv2d_backward_data(z(1, 16, 16, cout), z(cout, 8, k, k), (1, 16, 16, 8), 1, k // 2)
    with pytest.raises(_lib.LwgError, match="'same' padding"):
        ops.conv2d_backward_data(z(1, 14, 14, 64), z(64, 8, 7, 7), (1, 16, 16, 8), 1, 2)
