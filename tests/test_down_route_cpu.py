"""The request for the Toom-Cook F(2,2) down-sampling tile in the pure launch decision (gemm_route,
csrc/gemm_route.cpp) through a2m_conv1d_down_route: no GPU, the pointers are fake addresses that
are only inspected for alignment.

With the request and an eligible shape the route is the pipelined kind with the down flag and the
planner's fields (64x64 tile, bk 32, kchunk in whole 128-k chunks); every ineligibility gives
exactly the route without the request, which is the route a2m_conv1d_fwd_f32 takes today (im2col
and the dense pipelined tile at Co >= 128, the gathered tile below)."""
import ctypes

import pytest

from test_gemm_route_cpu import BASE_A, BASE_B, BASE_C, KIND_PIPE, REDUCE, VEC4, route as gemm_route

DOWN = 32
KEYS = ('kind', 'tile', 'bk', 'splits', 'kchunk', 'ma', 'mb', 'flags')

# the step's two shapes (B = 64 clips of 64 frames), then the GPU test's
STEP_SHAPES = [(64, 512, 512, 64), (64, 1024, 1024, 32)]
SMALL_SHAPES = [(1, 32, 64, 16), (5, 64, 20, 16), (3, 96, 96, 32), (2, 128, 64, 64), (2, 64, 64, 128),
                (4, 512, 512, 64)]


@pytest.fixture
def lib():
    from a2m import _native as N
    yield N.lib
    N.check(N.lib.a2m_gemm_pipe_override(-1))
    N.check(N.lib.a2m_gemm_plan_override(0, 0))
    N.check(N.lib.a2m_set_gemm_precision(0))


def conv_route(lib, B, Ci, Co, Tin, down, ks=4, stride=2, pad=1, px=BASE_B, py=BASE_C, xs_c=None, xs_b=None,
               ys_t=1):
    """Route of the conv of x [B][Ci][Tin] (channel stride xs_c) into a contiguous-or-strided y."""
    out = (ctypes.c_int32 * 8)()
    xs_c = Tin if xs_c is None else xs_c
    xs_b = Ci * xs_c if xs_b is None else xs_b
    Tout = (Tin + 2 * pad - ks) // stride + 1
    rc = lib.a2m_conv1d_down_route(px, xs_b, xs_c, B, Ci, Tin, BASE_A, Co, ks, stride, pad, py, Co * Tout * ys_t,
                                   Tout * ys_t, ys_t, down, out)
    assert rc == 0, lib.a2m_last_error()
    return dict(zip(KEYS, out))


@pytest.mark.parametrize('B,Ci,Co,Tin', STEP_SHAPES + SMALL_SHAPES)
def test_request_on_eligible_shape(lib, B, Ci, Co, Tin):
    from a2m import _native as N
    today = conv_route(lib, B, Ci, Co, Tin, 0)
    assert not today['flags'] & DOWN
    r = conv_route(lib, B, Ci, Co, Tin, 1)
    if r['flags'] & DOWN:
        assert r['kind'] == KIND_PIPE and r['tile'] == 64 and r['bk'] == 32 and r['ma'] == 0
        assert r['kchunk'] % 128 == 0 and r['splits'] == -(-4 * Ci // r['kchunk'])
        assert bool(r['flags'] & REDUCE) == (r['splits'] > 1)
        assert r['flags'] & VEC4          # contiguous y with Tout % 4 == 0, or slabs
    else:   # a shape class the rule table keeps on today's route
        assert r == today
    assert conv_route(lib, B, Ci, Co, Tin, 1) == r   # deterministic
    # forced split-K keeps the kind
    N.check(lib.a2m_gemm_plan_override(64, 2))
    if Ci >= 64:
        r2 = conv_route(lib, B, Ci, Co, Tin, 1)
        assert bool(r2['flags'] & DOWN) == bool(r['flags'] & DOWN)
        if r2['flags'] & DOWN:
            assert r2['kind'] == KIND_PIPE and r2['splits'] == 2 and r2['flags'] & REDUCE
            assert r2['kchunk'] % 128 == 0 and r2['kchunk'] * 2 >= 4 * Ci


def test_small_shapes_take_the_down_tile(lib):
    """The shapes of the GPU test are outside every rule that keeps a shape on today's route."""
    for B, Ci, Co, Tin in SMALL_SHAPES:
        assert conv_route(lib, B, Ci, Co, Tin, 1)['flags'] & DOWN


def test_a_launch_that_fills_the_chip_takes_one_split(lib):
    """At 256 tiles or more the tile runs at one split (no slabs, no reduce launch); below, the
    planner's split-K fills the chip as for every other tile."""
    for B, Ci, Co, Tin in STEP_SHAPES:
        r = conv_route(lib, B, Ci, Co, Tin, 1)
        if r['flags'] & DOWN:
            assert r['splits'] == 1 and r['kchunk'] == 4 * Ci and not r['flags'] & REDUCE
    r = conv_route(lib, 4, 512, 512, 64, 1)     # 16 tiles, K = 2048
    assert r['flags'] & DOWN and r['splits'] > 1 and r['flags'] & REDUCE


def test_unrequested_route_is_todays(lib):
    """Co >= 128: the dense GEMM over the im2col matrix (M = Co, N = B Tout, K = 4 Ci), exactly
    a2m_gemm_f32_route's answer for those operands; below, the gathered conv operand (no pipelined tile)."""
    for B, Ci, Co, Tin in STEP_SHAPES + [(4, 512, 512, 64)]:
        r = conv_route(lib, B, Ci, Co, Tin, 0)
        K, N = 4 * Ci, B * Tin // 2
        g = gemm_route(lib, Co, N, K, K, 1, K, 1)
        assert {k: r[k] for k in KEYS[:7]} == {k: g[k] for k in KEYS[:7]}
        assert r['kind'] == KIND_PIPE and (r['ma'], r['mb']) == (0, 0)
    r = conv_route(lib, 2, 128, 64, 64, 0)
    assert r['kind'] != KIND_PIPE and r['mb'] not in (0, 5)


@pytest.mark.parametrize('why,kw', [
    ('Tin = 8', dict(Tin=8)),
    ('Tin = 256 (a clip does not fit the tile)', dict(Tin=256)),
    ('Tin = 48 (clips do not tile 128 samples)', dict(Tin=48)),
    ('Ci % 32 != 0', dict(Ci=48)),
    ('k = 3', dict(ks=3)),
    ('stride 1', dict(stride=1, pad=1, ks=3)),
    ('k = 4, stride 1', dict(stride=1)),
    ('pad 0', dict(pad=0)),
    ('pad 2', dict(pad=2)),
    ('x not 16-byte aligned', dict(px=BASE_B + 4)),
    ('channel stride not a multiple of 4', dict(xs_c=34)),
    ('batch stride not a multiple of 4', dict(xs_b=64 * 32 + 2)),
])
def test_ineligible_request_is_todays_route(lib, why, kw):
    args = dict(B=4, Ci=64, Co=192, Tin=32)
    args.update(kw)
    r = conv_route(lib, down=1, **args)
    assert not r['flags'] & DOWN, why
    assert r == conv_route(lib, down=0, **args), why


def test_precision_and_overrides_refuse(lib):
    from a2m import _native as N
    args = (4, 64, 192, 32)
    assert conv_route(lib, *args, 1)['flags'] & DOWN
    N.check(lib.a2m_set_gemm_precision(1))            # bf16 operands
    assert conv_route(lib, *args, 1) == conv_route(lib, *args, 0)
    N.check(lib.a2m_set_gemm_precision(0))
    N.check(lib.a2m_gemm_pipe_override(0))            # gemm_tile instead of the pipelined tile
    assert conv_route(lib, *args, 1) == conv_route(lib, *args, 0)
    N.check(lib.a2m_gemm_pipe_override(-1))
    N.check(lib.a2m_gemm_plan_override(128, 0))       # 128x128 tiles
    assert conv_route(lib, *args, 1) == conv_route(lib, *args, 0)


def test_strided_views_stay_eligible(lib):
    """x as a channel slice of a wider buffer (a larger batch stride) and y as a strided view."""
    from a2m import _native as N
    N.check(lib.a2m_gemm_plan_override(64, 1))        # one split: the tile writes y itself (slabs are always float4)
    r = conv_route(lib, 4, 64, 192, 32, 1, xs_b=3 * 64 * 32)
    assert r['flags'] & DOWN and r['flags'] & VEC4 and not r['flags'] & REDUCE
    r = conv_route(lib, 4, 64, 192, 32, 1, ys_t=2)
    assert r['flags'] & DOWN and not r['flags'] & VEC4


def test_route_query_counts_nothing(lib):
    c = (ctypes.c_int64 * 4)()
    assert lib.a2m_gemm_kernel_counts(c, 1) == 0
    conv_route(lib, 4, 64, 192, 32, 1)
    assert lib.a2m_gemm_kernel_counts(c, 0) == 0
    assert list(c) == [0, 0, 0, 0]
