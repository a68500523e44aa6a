"""The Winograd request in the pure launch decision (gemm_route, csrc/gemm_route.cpp) through
a2m_conv1d_wino_route and a2m_gemm_f32_route: no GPU, the pointers are fake addresses that are only
inspected for alignment.

With the request and an eligible shape the route is the pipelined kind with the Winograd flag and
the direct conv's plan; every ineligibility gives exactly the route without the request; without
the request nothing changes (the parent's launches of tests/golden/gemm_route_parent_log.txt)."""
import ctypes
import re

import pytest

from test_gemm_route_cpu import (BASE_A, BASE_B, BASE_C, HALO, KIND_PIPE, PARENT_ROWS, REDUCE, case_strides,
                                 route as gemm_route)

WINO = 16
KEYS = ('kind', 'tile', 'bk', 'splits', 'kchunk', 'ma', 'mb', 'flags')


@pytest.fixture
def lib():
    from a2m import _native as N
    yield N.lib
    N.check(N.lib.a2m_gemm_pipe_override(-1))
    N.check(N.lib.a2m_gemm_plan_override(0, 0))
    N.check(N.lib.a2m_set_gemm_precision(0))


def conv_route(lib, B, Ci, Co, T, wino, G=1, px=BASE_B, py=BASE_C, xs_c=None, ys_t=1):
    """Route of the 3-tap pad-1 conv of a contiguous x [B][Ci][T] into y [B][Co][T]."""
    out = (ctypes.c_int32 * 8)()
    xs_c = T if xs_c is None else xs_c
    rc = lib.a2m_conv1d_wino_route(px, B * Ci * T if G > 1 else 0, Ci * xs_c, xs_c, G, B, Ci, T, BASE_A, Co, None,
                                   py, B * Co * T if G > 1 else 0, Co * T * ys_t, T * ys_t, ys_t, wino, out)
    assert rc == 0, lib.a2m_last_error()
    return dict(zip(KEYS, out))


# the step's six shapes (B = 64 clips of 64 frames): the decoders' conv and the UNet's five
STEP_SHAPES = [(64, 256, 256, 64), (64, 256, 512, 64), (64, 512, 1024, 32), (64, 1024, 2048, 16),
               (64, 2048, 1024, 32), (64, 1024, 512, 64)]


@pytest.mark.parametrize('B,Ci,Co,T', STEP_SHAPES + [(1, 32, 64, 16), (5, 64, 20, 16), (3, 96, 96, 32), (2, 128, 64, 64)])
def test_request_on_eligible_shape(lib, B, Ci, Co, T):
    from a2m import _native as N
    direct = conv_route(lib, B, Ci, Co, T, 0)
    assert direct['kind'] == KIND_PIPE and direct['flags'] & HALO and not direct['flags'] & WINO
    r = conv_route(lib, B, Ci, Co, T, 1)
    # the Winograd kind is the pipelined kind (a2m_gemm_kernel_counts keeps four entries) plus the flag;
    # the plan is the direct conv's (K = 3 Ci, splits on whole 96-k chunks)
    if r['flags'] & WINO:
        assert r == dict(direct, flags=direct['flags'] | WINO)
        assert r['kchunk'] % 96 == 0 and r['tile'] == 64 and r['bk'] == 32
    else:   # a shape class the rule table keeps on the direct tile: exactly today's route
        assert r == direct
    assert conv_route(lib, B, Ci, Co, T, 1) == r   # deterministic
    # forced split-K keeps the kind
    N.check(lib.a2m_gemm_plan_override(64, 2))
    if Ci >= 64:
        r2 = conv_route(lib, B, Ci, Co, T, 1)
        assert r2['splits'] == 2 and r2['flags'] & REDUCE and r2['kchunk'] % 96 == 0
        assert bool(r2['flags'] & WINO) == bool(r['flags'] & WINO)


def test_small_shapes_take_the_winograd_tile(lib):
    """The shapes of the GPU test are outside every direct-tile rule."""
    for B, Ci, Co, T in [(1, 32, 64, 16), (5, 64, 20, 16), (3, 96, 96, 32), (2, 128, 64, 64)]:
        assert conv_route(lib, B, Ci, Co, T, 1)['flags'] & WINO


@pytest.mark.parametrize('why,kw', [
    ('T = 8 (no halo layout)', dict(T=8)),
    ('T = 128 (does not tile the 64 rows)', dict(T=128)),
    ('Ci % 32 != 0', dict(Ci=48)),
    ('T = 4', dict(T=4)),
])
def test_ineligible_request_is_todays_route(lib, why, kw):
    args = dict(B=4, Ci=64, Co=64, T=32)
    args.update(kw)
    r = conv_route(lib, wino=1, **args)
    assert not r['flags'] & WINO, why
    assert r == conv_route(lib, wino=0, **args), why


def test_precision_and_overrides_refuse(lib):
    from a2m import _native as N
    args = (4, 64, 64, 32)
    assert conv_route(lib, *args, 1)['flags'] & WINO
    N.check(lib.a2m_set_gemm_precision(1))            # bf16 operands
    assert conv_route(lib, *args, 1) == conv_route(lib, *args, 0)
    N.check(lib.a2m_set_gemm_precision(0))
    N.check(lib.a2m_gemm_pipe_override(0))            # gemm_tile instead of the pipelined tile
    assert conv_route(lib, *args, 1) == conv_route(lib, *args, 0)
    N.check(lib.a2m_gemm_pipe_override(-1))
    N.check(lib.a2m_gemm_plan_override(128, 0))       # 128x128 tiles
    assert conv_route(lib, *args, 1) == conv_route(lib, *args, 0)


@pytest.mark.parametrize('cfg,line', PARENT_ROWS,
                         ids=['{case}-{prec}-split{split}-pipe{pipe}'.format(**c) for c, _ in PARENT_ROWS])
def test_request_unset_is_the_parent_route(lib, cfg, line):
    """a2m_gemm_f32 carries no request: its routes are the parent's, never the Winograd tile."""
    f = dict(re.findall(r'(\w+)=([\d,]+)', line))
    M, N, K, a_m, a_k, b_n, b_k = case_strides(cfg['case'])
    assert lib.a2m_set_gemm_precision({'fp32': 0, 'bf16': 1}[cfg['prec']]) == 0
    assert lib.a2m_gemm_plan_override(64, int(cfg['split'])) == 0
    assert lib.a2m_gemm_pipe_override(int(cfg['pipe'])) == 0
    r = gemm_route(lib, M, N, K, a_m, a_k, b_n, b_k)
    assert (r['tile'], r['bk'], r['splits']) == (int(f['tile']), int(f['bk']), int(f['splits']))
    assert [r['ma'], r['mb']] == [int(v) for v in f['modes'].split(',')]
    assert (r['kind'] == KIND_PIPE) == ('(pipe)' in line)
    assert not r['flags'] & WINO


def test_route_query_counts_nothing(lib):
    c = (ctypes.c_int64 * 4)()
    assert lib.a2m_gemm_kernel_counts(c, 1) == 0
    conv_route(lib, 4, 64, 64, 32, 1)
    assert lib.a2m_gemm_kernel_counts(c, 0) == 0
    assert list(c) == [0, 0, 0, 0]
