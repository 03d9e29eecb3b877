"""GPU: the HMR, LPIPS and Inception convolutions are ONE arithmetic (csrc/igemm32.h), and so are their 3x3 stride-2 max pools
(csrc/maxpool.h).

Each network's op-level tests (test_gpu_hmr.py, test_gpu_lpips.py, test_gpu_inception.py) hold its own entry point against fp64.
What none of them says is that the three entry points agree with each other: with no bias, no scale / shift, no prologue, no
residual and relu = 0 the policies add nothing to the accumulator, so the outputs must be the same bits -- torch.equal, no
tolerance.  The cases reach the vector gather (Cin % 4 == 0) with a K tail, a partial second M tile and two column tiles, and the
scalar gather (Cin = 3) with a single partial stage; the pools are compared where all three entries accept the size and, for HMR's
ceil mode, where it coincides with floor mode."""
import numpy as np
import pytest
import torch

from impersonator_amd import _lib

pytestmark = pytest.mark.gpu


def _inputs(seed, N, H, W, Cin, Cout, k):
    rs = np.random.RandomState(seed)
    x = torch.from_numpy(rs.standard_normal((N, H, W, Cin)).astype(np.float32)).cuda()             # NHWC
    w = torch.from_numpy(rs.standard_normal((k, k, Cin, Cout)).astype(np.float32)).cuda()          # [kh][kw][ci][co]
    return x, w


def _run(call, shape):
    """y NaN-prefilled, a guard tensor allocated right behind it: every element written, none past the end"""
    y = torch.full(shape, float("nan"), device="cuda")
    guard = torch.full((4096,), 7.0, device="cuda")
    _lib.check(call(y))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y).all()) and bool((guard == 7.0).all())
    return y


def _hmr_conv(x, w, k, stride, pad, shape):
    lib, (N, H, W, Cin), Cout = _lib.load(), x.shape, w.shape[3]
    return _run(lambda y: lib.lwg_hmr_conv(_lib.ptr(x), N, H, W, Cin, _lib.ptr(w), Cout, k, stride, pad, None, None, None, None, None,
                                           None, 0, 0, 0, _lib.ptr(y), _lib.stream_ptr()), shape)


def _lpips_conv(x, w, k, stride, pad, shape):
    lib, (N, H, W, Cin), Cout = _lib.load(), x.shape, w.shape[3]
    return _run(lambda y: lib.lwg_lpips_conv(_lib.ptr(x), N, H, W, Cin, _lib.ptr(w), None, Cout, k, stride, pad, 0, -1, _lib.ptr(y),
                                             _lib.stream_ptr()), shape)


def _inception_conv(x, w, k, stride, pad, shape):
    lib, (N, H, W, Cin), Cout = _lib.load(), x.shape, w.shape[3]
    return _run(lambda y: lib.lwg_inception_conv(_lib.ptr(x), N, H, W, Cin, _lib.ptr(w), None, None, Cout, k, k, stride, pad, pad, 0, -1,
                                                 _lib.ptr(y), Cout, 0, _lib.stream_ptr()), shape)


@pytest.mark.parametrize("N,S,Cin,Cout", [
    (2, 5, 36, 64),      # M = 50 under one tile, K = 324: ten full stages and a 4-wide K tail
    (1, 9, 8, 128),      # M = 81: a second, partial M tile; two column tiles
])
def test_vector_gather_is_the_same_bits_through_all_three_entries(N, S, Cin, Cout):
    """(k3, s1, p1) is the one geometry all three entries accept"""
    x, w = _inputs(100 + S, N, S, S, Cin, Cout, 3)
    shape = (N, S, S, Cout)
    hmr, lpips, inception = (f(x, w, 3, 1, 1, shape) for f in (_hmr_conv, _lpips_conv, _inception_conv))
    assert float(hmr.abs().max()) > 0
    assert torch.equal(hmr, lpips) and torch.equal(hmr, inception)


def test_scalar_gather_is_the_same_bits_through_hmr_and_lpips():
    """Cin = 3 as NHWC (Inception takes 3 channels as frames only): K = 27, a single partial stage"""
    x, w = _inputs(200, 2, 6, 6, 3, 64, 3)
    shape = (2, 6, 6, 64)
    hmr, lpips = _hmr_conv(x, w, 3, 1, 1, shape), _lpips_conv(x, w, 3, 1, 1, shape)
    assert float(hmr.abs().max()) > 0
    assert torch.equal(hmr, lpips)


def _pool(entry, x, shape):
    lib, (N, H, W, C) = _lib.load(), x.shape
    if entry == "inception":
        return _run(lambda y: lib.lwg_inception_maxpool(_lib.ptr(x), N, H, W, C, _lib.ptr(y), C, 0, _lib.stream_ptr()), shape)
    fn = lib.lwg_hmr_maxpool if entry == "hmr" else lib.lwg_lpips_maxpool
    return _run(lambda y: fn(_lib.ptr(x), N, H, W, C, _lib.ptr(y), _lib.stream_ptr()), shape)


@pytest.mark.parametrize("H,W,entries", [
    (7, 7, ("lpips", "inception", "hmr")),     # odd: ceil and floor mode coincide
    (8, 8, ("lpips", "inception")),            # even: the last row and column belong to no floor-mode window
    (9, 5, ("lpips", "inception", "hmr")),     # odd and not square
])
def test_max_pools_are_the_same_bits(H, W, entries):
    x = torch.from_numpy(np.random.RandomState(300 + H).standard_normal((2, H, W, 8)).astype(np.float32)).cuda()
    shape = (2, (H - 3) // 2 + 1, (W - 3) // 2 + 1, 8)
    outs = [_pool(e, x, shape) for e in entries]
    for other in outs[1:]:
        assert torch.equal(outs[0], other)
