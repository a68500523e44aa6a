"""The argument checks of a2m_batch_gather_f32 (csrc/data.hip), which return before any launch:
A2M_EINVAL with the message set for every refused case, A2M_OK for an empty batch with null
pointers.  No GPU is needed: nothing is launched."""
import ctypes

import pytest


@pytest.fixture(scope='module')
def abi():
    from a2m import _native as N
    buf = (ctypes.c_float * 1024)()
    addr = (ctypes.addressof(buf) + 15) // 16 * 16          # the kernel moves float4: 16-byte aligned
    return N, addr


def _call(N, addr, n_mod=2, C=(128, 104), window=(382, 64), interval=(6, 1), mode=(1, 2), arena=True, start=True,
          mean=(True, True), std=(True, True), out=True, order=True, b0=0, n=4, arrays=True):
    k = len(C)

    def ptrs(flags):
        flags = flags if isinstance(flags, tuple) else (flags,) * k
        return (ctypes.c_void_p * k)(*[addr if f else None for f in flags])

    def ints(v):
        return (ctypes.c_int32 * k)(*v)

    if not arrays:
        return N.lib.a2m_batch_gather_f32(n_mod, None, None, None, None, None, None, None, None, None,
                                          addr if order else None, b0, n, None)
    return N.lib.a2m_batch_gather_f32(n_mod, ptrs(arena), ptrs(start), ints(C), ints(window), ints(interval),
                                      ints(mode), ptrs(mean), ptrs(std), ptrs(out), addr if order else None,
                                      b0, n, None)


REFUSED = {
    'n_mod 0': dict(n_mod=0),
    'n_mod 5': dict(n_mod=5),
    'null arrays': dict(arrays=False),
    'null order': dict(order=False),
    'null arena': dict(arena=(True, False)),
    'null start': dict(start=(False, True)),
    'null out': dict(out=(True, False)),
    'window 0': dict(window=(0, 64)),
    'window negative': dict(window=(382, -64)),
    'interval 0': dict(interval=(6, 0)),
    'interval negative': dict(interval=(-6, 1)),
    'C not a multiple of 4': dict(C=(126, 104)),
    'mean given for raw': dict(mode=(0, 2), std=(False, True)),
    'std given for raw': dict(mode=(0, 2), mean=(False, True)),
    'mean missing for standardise': dict(mean=(False, True)),
    'std missing for standardise': dict(std=(False, True)),
    'mean missing for neck-sub': dict(mean=(True, False)),
    'std missing for neck-sub': dict(std=(True, False)),
    'neck-sub with C 128': dict(mode=(2, 2), C=(128, 104)),
    'neck-sub with C 52': dict(C=(128, 52)),
    'unknown mode': dict(mode=(1, 3)),
    'negative n': dict(n=-1),
    'negative b0': dict(b0=-4),
}


@pytest.mark.parametrize('case', list(REFUSED))
def test_batch_gather_refuses(abi, case):
    N, addr = abi
    assert N.lib.a2m_window_gather_f32(None, 0, 0, None, 0, 0, 0, None, None, None, None) == N.A2M_EINVAL
    assert 'batch_gather' not in N.last_error()
    assert _call(N, addr, **REFUSED[case]) == N.A2M_EINVAL, case
    assert N.last_error().startswith('batch_gather:'), N.last_error()
    with pytest.raises(N.A2MError, match='batch_gather'):
        N.check(N.A2M_EINVAL)


def test_batch_gather_empty_batch_is_a_no_op(abi):
    """n = 0: nothing to read, nothing launched, whatever the pointers."""
    N, addr = abi
    assert _call(N, addr, n=0, arrays=False, order=False) == 0
    assert _call(N, addr, n=0, arena=False, start=False, out=False, mean=False, std=False, order=False) == 0
    assert _call(N, addr, n=0, n_mod=1, C=(104,), window=(64,), interval=(1,), mode=(0,), mean=False, std=False) == 0
    assert _call(N, addr, n=0, n_mod=5, arrays=False) == N.A2M_EINVAL
