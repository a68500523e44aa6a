"""One launch per kernel kind of the GEMM engine (A2M_GEMM_KIND_*), each at the smallest shape that
reaches it: the launch counters (a2m_gemm_kernel_counts) show exactly that kind, the route query
(a2m_gemm_f32_route) with the tensors' real pointers names the kind that ran, and the result
matches torch at the tolerance of tests/test_gpu_pipe.py.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 1e-4   # fp32, tests/test_gpu_pipe.py


@pytest.fixture
def eng():
    from a2m import _native as N
    from a2m import functional as F
    yield N, F
    N.check(N.lib.a2m_gemm_pipe_override(-1))
    N.check(N.lib.a2m_convt_pair_override(-1))


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _rel(a, ref):
    return ((a.double() - ref).abs().max() / ref.abs().max()).item()


def _route_kind(N, M, Nn, K, A, a_m, a_k, B, b_n, b_k, C):
    out = (ctypes.c_int32 * 8)()
    N.check(N.lib.a2m_gemm_f32_route(M, Nn, 1, K, 1, 1, A.data_ptr(), 0, a_m, a_k, 0, B.data_ptr(), 0, b_n, 0, b_k,
                                     0, C.data_ptr(), 0, Nn, 1, 0, None, 1.0, 0, out))
    return out[0]


# name -> (M, N, K), B stored [K][N] (dense_kr), pipe override, the kind that runs
GEMM_CASES = {
    'tile_ks2_dense_64': ((64, 64, 64), False, 0, 'GEMM_KIND_TILE_KS2'),
    'tile_kr_64': ((64, 64, 64), True, 0, 'GEMM_KIND_TILE'),
    'pipe_dense_64': ((64, 64, 64), False, -1, 'GEMM_KIND_PIPE'),
    # K = 33 is no multiple of 4, so neither operand is loader mode 0 (float4 rows) and the launch
    # stays on gemm_tile, as before the route refactor; the nearest ragged shape on the pipelined
    # tile has K % 4 == 0 (M, N, K still no multiples of the 64 x 64 x 32 tile)
    'tile_dense_ragged_65x68x33': ((65, 68, 33), False, -1, 'GEMM_KIND_TILE'),
    'pipe_dense_ragged_65x68x36': ((65, 68, 36), False, -1, 'GEMM_KIND_PIPE'),
}


@pytest.mark.parametrize('name', sorted(GEMM_CASES))
def test_gemm_launch_kind(eng, name):
    N, F = eng
    (M, Nn, K), b_kr, pipe, kind = GEMM_CASES[name]
    kind = getattr(F, kind)
    A = _rand(M, K, seed=1)
    B = _rand(K, Nn, seed=2) if b_kr else _rand(Nn, K, seed=2)
    C = torch.empty(M, Nn, device=DEV)
    b_n, b_k = (1, Nn) if b_kr else (K, 1)
    ref = A.double() @ (B.double() if b_kr else B.double().t())
    N.check(N.lib.a2m_gemm_pipe_override(pipe))
    F.gemm_kernel_counts(reset=True)
    F.gemm(M, Nn, K, A, K, 1, B, b_n, b_k, C, Nn, 1)
    counts = F.gemm_kernel_counts()
    assert counts == [int(k == kind) for k in range(4)], (name, counts)
    assert _route_kind(N, M, Nn, K, A, K, 1, B, b_n, b_k, C) == kind
    assert F.gemm_kernel_counts() == counts   # the query launches nothing
    assert _rel(C, ref) < TOL


def test_pair_launch_kind(eng):
    """The n32_partial_tile case of tests/test_gpu_convt_pair.py with the pair forced on."""
    N, F = eng
    B, Ci, Co, Tin = 2, 64, 64, 16
    cpu = torch.Generator().manual_seed(41)
    x = torch.randn(B, Ci, Tin, generator=cpu)
    w = torch.randn(Ci, Co, 3, generator=cpu) * 0.1
    b = torch.randn(Co, generator=cpu)
    ref = torch.nn.functional.conv_transpose1d(x.double(), w.double(), b.double(), stride=2, padding=1,
                                               output_padding=1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    cache = {}
    N.check(N.lib.a2m_convt_pair_override(1))
    F.gemm_kernel_counts(reset=True)
    y = F.convt1d(xd, wd, bd, 2, 1, 1, cache=cache)
    assert F.gemm_kernel_counts() == [0, 0, 0, 1]
    assert _rel(y.cpu(), ref) < TOL
