"""Toom-Cook F(2,2) down-sampling conv1d (a2m_conv1d_down_fwd_f32 / gemm_pipe_kernel_down, reached
through F.conv1d(wino=True) at (k, stride, pad) == (4, 2, 1)).

Held against an fp64 conv1d(stride=2, padding=1) at TOL32 = 1e-5 of max |ref| (the tap path's
bound, tests/test_gpu_tapconv.py) and at 1e-5 against the existing route (im2col and the dense
tile at Co >= 128, the gathered tile below) on the same inputs.  The shapes are the smallest at
which each mechanism can fail: one channel chunk with one live clip of 8 outputs in an eight-clip
tile; partial M and N tiles with clip edges inside the tile; an odd chunk count (the A stages and
the plane-1 units alternate by chunk parity); exactly one tile; one clip a tile; the step's K at a
small batch.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
from conv_helpers import bn_lrelu_ref, bn_params as _bn, plan_override  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL32 = 1e-5

SHAPES = [(1, 32, 64, 16), (5, 64, 20, 16), (3, 96, 96, 32), (2, 128, 64, 64), (2, 64, 64, 128), (4, 512, 512, 64)]


def _conv_ref(x, w, b=None):
    return torch.nn.functional.conv1d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)


def _inputs(B, Ci, Co, T, seed=0):
    g = torch.Generator().manual_seed(seed + B * 7 + Ci + T)
    x = torch.randn(B, Ci, T, generator=g)
    w = torch.randn(Co, Ci, 4, generator=g) / np.sqrt(4 * Ci)
    b = torch.randn(Co, generator=g)
    return x, w, b


@pytest.mark.parametrize('B,Ci,Co,T', SHAPES)
def test_down_conv1d_matches_fp64_and_existing_route(B, Ci, Co, T):
    from a2m import functional as F
    x, w, b = _inputs(B, Ci, Co, T)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    cache = {}
    y = F.conv1d(xd, wd, bd, 2, 1, cache=cache, wino=True)
    assert 'down_w' in cache and 'wino_w' not in cache and 'w' not in cache, 'down-sampling tile not taken'
    old = F.conv1d(xd, wd, bd, 2, 1, cache={})
    ref = _conv_ref(x, w, b)
    e_n, e_o = rel_err(y.cpu().double(), ref), rel_err(old.cpu().double(), ref)
    print(f'B={B} Ci={Ci} Co={Co} Tin={T}: existing route {e_o:.2e} down tile {e_n:.2e} ratio {e_n / max(e_o, 1e-30):.2f}')
    assert e_n < TOL32, (e_n, e_o)
    assert rel_err(y.cpu(), old.cpu()) < 1e-5


def test_down_conv1d_split_k(plan_override):
    from a2m import functional as F
    B, Ci, Co, T = 2, 128, 64, 64
    x, w, b = _inputs(B, Ci, Co, T, seed=1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    old = F.conv1d(xd, wd, bd, 2, 1, cache={})
    plan_override(64, 2)
    out = torch.empty(B, Co, T // 2, device=DEV)
    r = F.conv1d_down_route(xd, Co, out)
    assert r['splits'] == 2 and r['flags'] & F.ROUTE_DOWN and r['flags'] & 8
    cache = {}
    y = F.conv1d(xd, wd, bd, 2, 1, out=out, cache=cache, wino=True)
    assert 'down_w' in cache
    assert rel_err(y.cpu().double(), _conv_ref(x, w, b)) < TOL32
    assert rel_err(y.cpu(), old.cpu()) < 1e-5


def test_down_conv1d_epilogue_views_and_cache():
    """BN-eval + LeakyReLU, x a channel slice of a wider buffer (the UNet's cat[:, 2C:]), out a
    contiguous tensor (the float4 epilogue) and a strided view (the scalar epilogue); an in-place
    weight update rebuilds the packed U each time."""
    from a2m import functional as F
    g = torch.Generator().manual_seed(3)
    B, Ci, Co, T = 4, 64, 96, 32
    cat = torch.randn(B, 3 * Ci, T, generator=g).to(DEV)
    x = cat[:, 2 * Ci:]
    w = (torch.randn(Co, Ci, 4, generator=g) * 0.05).to(DEV)
    bias = torch.randn(Co, generator=g).to(DEV)
    bn = _bn(Co, g)

    def ref_of(w):
        return bn_lrelu_ref(_conv_ref(x.cpu(), w.cpu(), bias.cpu()), bn)

    cache = {}
    y = F.conv1d(x, w, bias, 2, 1, bn=bn, act=F.ACT_LRELU, slope=0.2, cache=cache, wino=True)
    assert 'down_w' in cache and y.is_contiguous()
    assert rel_err(y.cpu().double(), ref_of(w)) < TOL32
    packed_before = cache['down_w'].clone()
    with torch.no_grad():
        w.mul_(-1.5)
    outbuf = torch.zeros(B, T // 2, 2 * Co, device=DEV)
    out = outbuf[:, :, Co:].permute(0, 2, 1)
    F.conv1d(x, w, bias, 2, 1, bn=bn, act=F.ACT_LRELU, slope=0.2, out=out, cache=cache, wino=True)
    assert not torch.equal(cache['down_w'], packed_before)
    assert rel_err(out.cpu().double(), ref_of(w)) < TOL32
    assert outbuf[:, :, :Co].abs().max().item() == 0.0
    packed_before = cache['down_w'].clone()
    with torch.no_grad():
        w.add_(0.01)
    y = F.conv1d(x, w, bias, 2, 1, bn=bn, act=F.ACT_LRELU, slope=0.2, cache=cache, wino=True)
    assert not torch.equal(cache['down_w'], packed_before)
    assert rel_err(y.cpu().double(), ref_of(w)) < TOL32


def test_down_pack_layout():
    from a2m import functional as F
    import down_ref as DR
    g = torch.Generator().manual_seed(5)
    w = torch.randn(20, 96, 4, generator=g)
    packed = F.conv1d_down_packed(w.to(DEV)).cpu().numpy()
    assert np.array_equal(packed, DR.pack_u(w.numpy()))


@pytest.mark.parametrize('T', [16, 32, 64])
def test_down_conv1d_clip_edges_exact(T):
    """x is nonzero (1.0) only at t = 0 and T - 1 of each clip and every weight row has a single
    nonzero tap (1.0): the result is y[t] = x[2t - 1 + tap] exactly (0 / 1 values are exact), so a
    pair that reads across a clip boundary shows."""
    from a2m import functional as F
    B, C = 6, 32
    x = torch.zeros(B, C, T)
    x[:, :, 0] = 1.0
    x[:, :, T - 1] = 1.0
    xd = x.to(DEV)
    for tap in range(4):
        w = torch.zeros(C, C, 4)
        w[torch.arange(C), torch.arange(C), tap] = 1.0
        cache = {}
        y = F.conv1d(xd, w.to(DEV), None, 2, 1, cache=cache, wino=True).cpu()
        assert 'down_w' in cache
        ref = torch.zeros(B, C, T // 2)
        for t in range(T // 2):
            if 0 <= 2 * t - 1 + tap < T:
                ref[:, :, t] = x[:, :, 2 * t - 1 + tap]
        assert torch.equal(y, ref), (tap, (y - ref).abs().max().item())


def test_down_refusals_fall_back_bitwise():
    """Tin = 8, other k / s / p, Ci % 32 != 0, misaligned x and bf16 precision take today's route
    through F.conv1d(wino=True): bitwise the outputs of wino=False; the C entry itself returns the
    documented error."""
    import a2m
    from a2m import _native as N
    from a2m import functional as F
    g = torch.Generator().manual_seed(9)
    w4 = (torch.randn(64, 64, 4, generator=g) / 16).to(DEV)
    w5 = (torch.randn(64, 64, 5, generator=g) / 16).to(DEV)
    w48 = (torch.randn(64, 48, 4, generator=g) / 14).to(DEV)
    x8 = torch.randn(8, 64, 8, generator=g).to(DEV)
    x64 = torch.randn(2, 64, 64, generator=g).to(DEV)
    x48 = torch.randn(2, 48, 64, generator=g).to(DEV)
    xmis = torch.randn(2, 64, 68, generator=g).to(DEV)[:, :, 1:65]   # rows start 4 bytes off a 16-byte boundary

    def down_entry(x, w, ks, stride, pad):
        B, Ci, T = x.shape
        packed = torch.zeros(w.shape[0] * Ci * 6, device=DEV)
        y = torch.empty(B, w.shape[0], (T + 2 * pad - ks) // stride + 1, device=DEV)
        return N.lib.a2m_conv1d_down_fwd_f32(x.data_ptr(), x.stride(0), x.stride(1), B, Ci, T, packed.data_ptr(), None,
                                             w.shape[0], ks, stride, pad, None, None, None, None, 1e-5, 0, 0.2,
                                             y.data_ptr(), y.stride(0), y.stride(1), 1, None, 0, None)

    for x, w, stride, pad in ((x8, w4, 2, 1), (x64, w4, 1, 1), (x64, w4, 2, 0), (x64, w4, 2, 2), (x64, w5, 2, 1),
                              (x48, w48, 2, 1), (xmis, w4, 2, 1)):
        c1, c0 = {}, {}
        a = F.conv1d(x, w, None, stride, pad, cache=c1, wino=True)
        b = F.conv1d(x, w, None, stride, pad, cache=c0)
        assert 'down_w' not in c1 and torch.equal(a, b), (tuple(x.shape), tuple(w.shape), stride, pad)
        rc = down_entry(x, w, w.shape[2], stride, pad)
        assert rc == N.A2M_EINVAL and 'not a down-sampling launch' in N.last_error()
    with a2m.gemm_precision('bf16'):
        c1 = {}
        a = F.conv1d(x64, w4, None, 2, 1, cache=c1, wino=True)
        b = F.conv1d(x64, w4, None, 2, 1, cache={})
        assert 'down_w' not in c1 and torch.equal(a, b)
        rc = down_entry(x64, w4, 4, 2, 1)
        assert rc == N.A2M_EINVAL and 'not a down-sampling launch' in N.last_error()


def test_down_kernel_counts_under_the_pipelined_kind():
    from a2m import _native as N
    from a2m import functional as F
    x, w, b = _inputs(2, 64, 64, 32, seed=2)
    xd, wd = x.to(DEV), w.to(DEV)
    cache = {}
    packed = F.conv1d_down_packed(wd, cache)
    assert packed.numel() == 64 * 64 * 6
    c = (ctypes.c_int64 * 4)()
    N.check(N.lib.a2m_gemm_kernel_counts(c, 1))
    F.conv1d_down(xd, wd, cache=cache)
    N.check(N.lib.a2m_gemm_kernel_counts(c, 1))
    assert list(c) == [0, 0, 1, 0]
