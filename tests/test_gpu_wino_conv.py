"""Winograd F(2,3) conv1d (a2m_conv1d_wino_fwd_f32 / gemm_pipe_kernel_wino, F.conv1d(wino=True)).

Held against an fp64 conv1d at TOL32 = 1e-5 of max |ref| (the tap path's bound,
tests/test_gpu_tapconv.py) and at 1e-5 against the direct tap path on the same inputs.  The shapes
are the smallest at which each mechanism can fail: one channel chunk with a single live clip in a
four-clip tile; partial M and N tiles with clip edges inside the tile; an odd chunk count; one clip
per tile; the decoders' shape.
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

SHAPES = [(1, 32, 64, 16), (5, 64, 20, 16), (3, 96, 96, 32), (2, 128, 64, 64), (64, 256, 256, 64)]


def _conv_ref(x, w, b=None):
    return torch.nn.functional.conv1d(x.double(), w.double(), None if b is None else b.double(), padding=1)


def _inputs(B, Ci, Co, T, seed=0):
    g = torch.Generator().manual_seed(seed + B * 7 + Ci + T)
    x = torch.randn(B, Ci, T, generator=g)
    w = torch.randn(Co, Ci, 3, generator=g) / np.sqrt(3 * Ci)
    b = torch.randn(Co, generator=g)
    return x, w, b


@pytest.mark.parametrize('B,Ci,Co,T', SHAPES)
def test_wino_conv1d_matches_fp64_and_direct(B, Ci, Co, T):
    from a2m import functional as F
    x, w, b = _inputs(B, Ci, Co, T)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    cache = {}
    y = F.conv1d(xd, wd, bd, 1, 1, cache=cache, wino=True)
    assert 'wino_w' in cache and 'w' not in cache, 'Winograd path not taken'
    direct = F.conv1d(xd, wd, bd, 1, 1, cache={})
    ref = _conv_ref(x, w, b)
    e_w, e_d = rel_err(y.cpu().double(), ref), rel_err(direct.cpu().double(), ref)
    print(f'B={B} Ci={Ci} Co={Co} T={T}: direct {e_d:.2e} winograd {e_w:.2e} ratio {e_w / max(e_d, 1e-30):.2f}')
    assert e_w < TOL32, (e_w, e_d)
    assert rel_err(y.cpu(), direct.cpu()) < 1e-5


def test_wino_conv1d_split_k(plan_override):
    from a2m import functional as F
    B, Ci, Co, T = 2, 128, 64, 64
    x, w, b = _inputs(B, Ci, Co, T, seed=1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    plan_override(64, 2)
    out = torch.empty(B, Co, T, device=DEV)
    r = F.conv1d_wino_route(xd, Co, out)
    assert r['splits'] == 2 and r['flags'] & F.ROUTE_WINO and r['flags'] & 8
    cache = {}
    y = F.conv1d(xd, wd, bd, 1, 1, out=out, cache=cache, wino=True)
    assert 'wino_w' in cache
    direct = F.conv1d(xd, wd, bd, 1, 1, cache={})
    assert rel_err(y.cpu().double(), _conv_ref(x, w, b)) < TOL32
    assert rel_err(y.cpu(), direct.cpu()) < 1e-5


def test_wino_conv1d_epilogue_views_residual_and_cache():
    """BN-eval + LeakyReLU, a residual operand, x a channel slice of a wider buffer, out a strided
    view (the scalar epilogue) and a contiguous one (the float4 epilogue); an in-place weight update
    rebuilds the packed U."""
    from a2m import functional as F
    g = torch.Generator().manual_seed(3)
    B, Ci, Co, T = 4, 64, 96, 32
    cat = torch.randn(B, 2 * Ci, T, generator=g).to(DEV)
    x = cat[:, Ci:]
    w = (torch.randn(Co, Ci, 3, generator=g) * 0.05).to(DEV)
    bias = torch.randn(Co, generator=g).to(DEV)
    bn = _bn(Co, g)

    def ref_of(w):
        return bn_lrelu_ref(_conv_ref(x.cpu(), w.cpu(), bias.cpu()), bn)

    outbuf = torch.zeros(B, T, 2 * Co, device=DEV)
    out = outbuf[:, :, Co:].permute(0, 2, 1)
    cache = {}
    F.conv1d(x, w, bias, 1, 1, bn=bn, act=F.ACT_LRELU, slope=0.2, out=out, cache=cache, wino=True)
    assert 'wino_w' in cache
    assert rel_err(out.cpu().double(), ref_of(w)) < TOL32
    assert outbuf[:, :, :Co].abs().max().item() == 0.0
    res = torch.randn(B, Co, T, generator=g).to(DEV)
    y = F.conv1d_wino(x, w, bias, bn=bn, act=F.ACT_LRELU, slope=0.2, cache=cache, res=res)
    assert rel_err(y.cpu().double(), ref_of(w) + res.cpu().double()) < TOL32
    resv = torch.randn(B, T, 2 * Co, generator=g).to(DEV)[:, :, Co:].permute(0, 2, 1)
    F.conv1d_wino(x, w, bias, bn=bn, act=F.ACT_LRELU, slope=0.2, out=out, cache=cache, res=resv)
    assert rel_err(out.cpu().double(), ref_of(w) + resv.cpu().double()) < TOL32
    packed_before = cache['wino_w'].clone()
    with torch.no_grad():
        w.mul_(-1.5)
    y = F.conv1d(x, w, bias, 1, 1, bn=bn, act=F.ACT_LRELU, slope=0.2, cache=cache, wino=True)
    assert not torch.equal(cache['wino_w'], packed_before)
    assert rel_err(y.cpu().double(), ref_of(w)) < TOL32


def test_wino_pack_layout():
    from a2m import functional as F
    import wino_ref as WR
    g = torch.Generator().manual_seed(5)
    w = torch.randn(20, 96, 3, generator=g)
    packed = F.conv1d_wino_packed(w.to(DEV)).cpu().numpy()
    assert np.array_equal(packed, WR.pack_u(w.numpy()))


@pytest.mark.parametrize('T', [16, 32, 64])
def test_wino_conv1d_clip_edges_exact(T):
    """x is nonzero only at t = 0 and T - 1 of each clip and w has a single nonzero tap: the result
    is the shifted input exactly (0 / 1 values are exact), so a pair that reads across a clip
    boundary shows."""
    from a2m import functional as F
    B, C = 6, 32
    x = torch.zeros(B, C, T)
    x[:, :, 0] = 1.0
    x[:, :, T - 1] = 1.0
    xd = x.to(DEV)
    for tap in range(3):
        w = torch.zeros(C, C, 3)
        w[torch.arange(C), torch.arange(C), tap] = 1.0
        cache = {}
        y = F.conv1d(xd, w.to(DEV), None, 1, 1, cache=cache, wino=True).cpu()
        assert 'wino_w' in cache
        ref = torch.zeros_like(x)
        s = tap - 1
        for t in range(T):
            if 0 <= t + s < T:
                ref[:, :, t] = x[:, :, t + s]
        assert torch.equal(y, ref), (tap, (y - ref).abs().max().item())


def test_wino_refusals_fall_back_bitwise():
    """T = 8, stride 2 and bf16 precision take the direct route through F.conv1d(wino=True): bitwise
    the outputs of wino=False; the C entry itself returns the documented error."""
    import a2m
    from a2m import _native as N
    from a2m import functional as F
    g = torch.Generator().manual_seed(9)
    w = (torch.randn(64, 64, 3, generator=g) / 14).to(DEV)
    x8 = torch.randn(8, 64, 8, generator=g).to(DEV)
    x64 = torch.randn(2, 64, 64, generator=g).to(DEV)
    for x, stride in ((x8, 1), (x64, 2)):
        c1, c0 = {}, {}
        a = F.conv1d(x, w, None, stride, 1, cache=c1, wino=True)
        b = F.conv1d(x, w, None, stride, 1, cache=c0)
        assert 'wino_w' not in c1 and torch.equal(a, b)
    with a2m.gemm_precision('bf16'):
        c1 = {}
        a = F.conv1d(x64, w, None, 1, 1, cache=c1, wino=True)
        b = F.conv1d(x64, w, None, 1, 1, cache={})
        assert 'wino_w' not in c1 and torch.equal(a, b)
        packed = F.conv1d_wino_packed(w)
        y = torch.empty(2, 64, 64, device=DEV)
        rc = N.lib.a2m_conv1d_wino_fwd_f32(x64.data_ptr(), 64 * 64, 64, 2, 64, 64, packed.data_ptr(), None, 64,
                                           None, None, None, None, 1e-5, 0, 0.2, None, y.data_ptr(), 64 * 64, 64, 1,
                                           None, 0, None)
        assert rc == N.A2M_EINVAL and 'not a Winograd launch' in N.last_error()
    packed = F.conv1d_wino_packed(w)
    y = torch.empty(8, 64, 8, device=DEV)
    rc = N.lib.a2m_conv1d_wino_fwd_f32(x8.data_ptr(), 64 * 8, 8, 8, 64, 8, packed.data_ptr(), None, 64, None, None,
                                       None, None, 1e-5, 0, 0.2, None, y.data_ptr(), 64 * 8, 8, 1, None, 0, None)
    assert rc == N.A2M_EINVAL and 'not a Winograd launch' in N.last_error()


def test_wino_kernel_counts_under_the_pipelined_kind():
    from a2m import _native as N
    from a2m import functional as F
    x, w, b = _inputs(2, 64, 64, 32, seed=2)
    xd, wd = x.to(DEV), w.to(DEV)
    packed = F.conv1d_wino_packed(wd)
    assert packed.numel() == 64 * 64 * 4
    c = (ctypes.c_int64 * 4)()
    N.check(N.lib.a2m_gemm_kernel_counts(c, 1))
    F.conv1d_wino(xd, wd)
    N.check(N.lib.a2m_gemm_kernel_counts(c, 1))
    assert list(c) == [0, 0, 1, 0]


def test_wino_group_equals_single_launches():
    """The grouped entry (the decoders' schedule) gives each problem its own launch's result."""
    from a2m import functional as F
    g = torch.Generator().manual_seed(11)
    G, B, Ci, Co, T = 3, 4, 64, 96, 32
    xs_all = torch.randn(G, B, Ci, T, generator=g).to(DEV)
    outs_all = torch.empty(G, B, Co, T, device=DEV)
    ws = [(torch.randn(Co, Ci, 3, generator=g) / 14).to(DEV) for _ in range(G)]
    bias = torch.randn(G, Co, generator=g).to(DEV)
    packed = torch.stack([F.conv1d_wino_packed(w) for w in ws])
    xs, outs = list(xs_all.unbind(0)), list(outs_all.unbind(0))
    assert F.conv1d_wino_group_taken(xs, Co, outs)
    F.conv1d_wino_group(xs, packed, bias, Co, None, F.ACT_RELU, 0.2, outs)
    for i in range(G):
        single = F.conv1d_wino(xs[i], ws[i], bias[i], act=F.ACT_RELU)
        assert torch.equal(outs[i], single), i
