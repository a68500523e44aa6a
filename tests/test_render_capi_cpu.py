"""Argument checks and zero-size contracts of a2m_render_poses_u8 and a2m_track_blend_f32
(csrc/render.hip).  Both return before any launch, so the library is called here without a GPU,
with host buffers standing in for device pointers."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def abi():
    from a2m import _native as N
    buf = (ctypes.c_float * 1024)()
    return N, ctypes.cast(buf, ctypes.c_void_p)


def _i32(*v):
    return np.array(v, np.int32)


def _render(N, p, n=2, P=1, K=4, idx=(0, 1, 2), off=(0, 3), L=1, hw=1.5, W=8, H=8, null=None):
    idx, off, rgb, bg = _i32(*idx), _i32(*off), np.zeros(3 * max(L, 1), np.uint8), np.zeros(3, np.uint8)
    args = dict(kp=p, idx=idx.ctypes.data, off=off.ctypes.data, rgb=rgb.ctypes.data, xform=p,
                bg=bg.ctypes.data, out=p)
    if null:
        args[null] = None
    return N.lib.a2m_render_poses_u8(args['kp'], n, P, K, args['idx'], args['off'], args['rgb'], L,
                                     args['xform'], hw, args['bg'], W, H, args['out'], None)


def test_both_entry_points_are_exported():
    from a2m import _native as N
    assert {'a2m_render_poses_u8', 'a2m_track_blend_f32'} <= set(N.exported_symbols())


@pytest.mark.parametrize('null', ['kp', 'idx', 'off', 'rgb', 'xform', 'bg', 'out'])
def test_render_rejects_a_null_pointer(abi, null):
    N, p = abi
    assert _render(N, p, null=null) == N.A2M_EINVAL
    assert 'null' in N.last_error()


@pytest.mark.parametrize('kw', [dict(P=0), dict(K=0), dict(L=-1), dict(W=0), dict(H=0), dict(n=-1),
                                dict(hw=-0.5), dict(hw=float('nan')), dict(hw=float('inf'))],
                         ids=lambda kw: '%s=%s' % next(iter(kw.items())))
def test_render_rejects_bad_sizes(abi, kw):
    N, p = abi
    assert _render(N, p, **kw) == N.A2M_EINVAL
    assert 'render_poses' in N.last_error()


def test_render_rejects_bad_polyline_tables(abi):
    N, p = abi
    assert _render(N, p, idx=(0, 1, 2), off=(0, 1, 3), L=2) == N.A2M_EINVAL     # one-point polyline
    assert 'polyline 0 has 1' in N.last_error()
    assert _render(N, p, idx=(0, 1), off=(0, 0, 2), L=2) == N.A2M_EINVAL        # empty polyline
    assert _render(N, p, idx=(0, 1, 2, 3), off=(0, 3, 2), L=2) == N.A2M_EINVAL  # offsets go backwards
    assert _render(N, p, idx=(0, 1, 2), off=(1, 3), L=1) == N.A2M_EINVAL        # does not start at 0
    assert _render(N, p, idx=(0, 4), off=(0, 2), L=1) == N.A2M_EINVAL           # index == K
    assert 'outside' in N.last_error()
    assert _render(N, p, idx=(-1, 2), off=(0, 2), L=1) == N.A2M_EINVAL
    assert _render(N, p, idx=(0, 1) * 129, off=tuple(range(0, 260, 2)), L=129) == N.A2M_EINVAL  # limits
    assert _render(N, p, idx=tuple(range(4)) * 129, off=(0, 516), L=1) == N.A2M_EINVAL
    assert _render(N, p, P=5, K=1000, idx=(0, 1), off=(0, 2)) == N.A2M_EINVAL


def test_render_of_no_frames_is_a_no_op(abi):
    N, p = abi
    assert N.lib.a2m_render_poses_u8(None, 0, 1, 52, None, None, None, 14, None, 1.5, None, 96, 40, None, None) == 0
    assert _render(N, p, n=0) == 0
    assert _render(N, p, n=0, P=0) == N.A2M_EINVAL         # the sizes are still checked


def test_track_blend_contracts(abi):
    N, p = abi
    f, EINVAL = N.lib.a2m_track_blend_f32, N.A2M_EINVAL
    assert f(p, 2, 8, 104, 5, None, None, p, None) == EINVAL           # overlap > T/2
    assert 'overlap' in N.last_error()
    assert f(p, 2, 8, 104, -1, None, None, p, None) == EINVAL
    assert f(p, 2, 7, 104, 4, None, None, p, None) == EINVAL           # T/2 rounds down
    assert f(p, 2, 8, 104, 2, p, None, p, None) == EINVAL              # mean without std
    assert f(p, 2, 8, 104, 2, None, p, p, None) == EINVAL
    assert f(p, 2, 0, 104, 0, None, None, p, None) == EINVAL           # T < 1
    assert f(p, 2, 8, 0, 0, None, None, p, None) == EINVAL
    assert f(p, -1, 8, 104, 0, None, None, p, None) == EINVAL
    assert f(None, 2, 8, 104, 2, None, None, p, None) == EINVAL
    assert f(p, 2, 8, 104, 2, None, None, None, None) == EINVAL
    assert 'null' in N.last_error()
    assert f(None, 0, 8, 104, 4, None, None, None, None) == 0
    assert f(None, 0, 8, 104, 5, None, None, None, None) == EINVAL     # still checked when empty
