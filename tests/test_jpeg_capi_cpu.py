"""Argument checks and the zero-size contract of a2m_jpeg_encode_u8 / a2m_jpeg_ws_bytes
(csrc/jpeg.hip), and the quantiser tables of a2m.jpeg.  Every refusal returns before any launch, so
the library is called here without a GPU, with host buffers standing in for device pointers."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def abi():
    from a2m import _native as N
    buf = (ctypes.c_uint8 * 4096)()
    return N, ctypes.cast(buf, ctypes.c_void_p)


def _encode(N, p, n=2, W=13, H=9, ql=None, qc=None, cap=1024, ws_bytes=None, null=None):
    ql = np.full(64, 16, np.uint16) if ql is None else np.asarray(ql, np.uint16)
    qc = np.full(64, 17, np.uint16) if qc is None else np.asarray(qc, np.uint16)
    args = dict(frames=p, ql=ql.ctypes.data, qc=qc.ctypes.data, out=p, offsets=p, ws=p)
    if null:
        args[null] = None
    if ws_bytes is None:
        ws_bytes = N.lib.a2m_jpeg_ws_bytes(n, W, H)
    return N.lib.a2m_jpeg_encode_u8(args['frames'], n, W, H, args['ql'], args['qc'], args['out'], cap,
                                    args['offsets'], args['ws'], ws_bytes, None)


def test_entry_points_are_exported():
    from a2m import _native as N
    assert {'a2m_jpeg_encode_u8', 'a2m_jpeg_ws_bytes'} <= set(N.exported_symbols())


@pytest.mark.parametrize('null', ['frames', 'ql', 'qc', 'out', 'offsets', 'ws'])
def test_rejects_a_null_pointer(abi, null):
    N, p = abi
    assert _encode(N, p, null=null) == N.A2M_EINVAL
    assert 'null' in N.last_error()


@pytest.mark.parametrize('kw', [dict(W=0), dict(H=0), dict(W=65536), dict(H=65536), dict(W=-3), dict(n=-1),
                                dict(cap=-1)], ids=lambda kw: '%s=%s' % next(iter(kw.items())))
def test_rejects_bad_sizes(abi, kw):
    N, p = abi
    assert _encode(N, p, ws_bytes=1 << 40, **kw) == N.A2M_EINVAL
    assert 'jpeg_encode' in N.last_error()


@pytest.mark.parametrize('table', ['ql', 'qc'])
@pytest.mark.parametrize('value', [0, 256, 65535])
def test_rejects_a_quantiser_outside_the_baseline_range(abi, table, value):
    N, p = abi
    q = np.full(64, 16, np.uint16)
    q[37] = value
    assert _encode(N, p, **{table: q}) == N.A2M_EINVAL
    assert 'quantiser entry 37' in N.last_error()


def test_rejects_a_small_workspace(abi):
    N, p = abi
    need = N.lib.a2m_jpeg_ws_bytes(2, 13, 9)
    assert need > 0
    assert _encode(N, p, ws_bytes=need - 1) == N.A2M_EINVAL
    assert 'workspace' in N.last_error()


def test_workspace_size():
    from a2m import _native as N
    ws = N.lib.a2m_jpeg_ws_bytes
    assert ws(0, 13, 9) == 0 and ws(1, 0, 9) == 0 and ws(1, 13, 65536) == 0
    # 2 x 2 MCUs: 12 blocks of 64 int16 coefficients, a bit position and 208 scratch bytes each
    assert 12 * (128 + 4 + 208) <= ws(1, 13, 9) <= 12 * (128 + 4 + 208) + 8 * 256
    assert ws(2, 13, 9) > ws(1, 13, 9) and ws(1, 16, 16) == ws(1, 13, 9)
    assert ws(1, 65535, 65535) > 8192 * 8192 * 3 * (128 + 208)                  # no 32-bit overflow
    assert ws(2 ** 31 - 1, 65535, 65535) == 0                                   # more than one launch takes


def test_rejects_more_blocks_than_one_launch(abi):
    N, p = abi
    assert _encode(N, p, n=2 ** 31 - 1, W=65535, H=65535, ws_bytes=2 ** 64 - 1) == N.A2M_EINVAL
    assert 'one launch' in N.last_error()


def test_no_frames_is_a_no_op(abi):
    N, p = abi
    assert N.lib.a2m_jpeg_encode_u8(None, 0, 13, 9, None, None, None, 0, None, None, 0, None) == 0
    assert _encode(N, p, n=0) == 0
    assert _encode(N, p, n=0, W=0) == N.A2M_EINVAL          # the sizes are still checked


def test_quant_tables_endpoints():
    from a2m import jpeg as A
    q50, q1, q100 = A.quant_tables(50), A.quant_tables(1), A.quant_tables(100)
    assert q50.shape == (2, 64) and q50.dtype == np.uint16
    assert q50[0].tolist() == list(A.BASE_LUMA) and q50[1].tolist() == list(A.BASE_CHROMA)
    assert (q100 == 1).all()
    assert (q1 == 255).all()                                # scale 5000 %: every entry clamps
    q90 = A.quant_tables(90)
    assert q90[0, :4].tolist() == [3, 2, 2, 3] and q90[1, 63] == 20
    assert A.quant_tables(25)[0, 0] == 32
    for bad in (0, 101, 50.5, -1):
        with pytest.raises(ValueError):
            A.quant_tables(bad)


def test_header_layout():
    from a2m import jpeg as A
    h = A.jpeg_header(1500, 500, A.quant_tables(90))
    assert h[:4] == b'\xff\xd8\xff\xe0' and h[6:11] == b'JFIF\0'
    sof = h.index(b'\xff\xc0')
    assert h[sof + 4:sof + 10] == bytes([8]) + (500).to_bytes(2, 'big') + (1500).to_bytes(2, 'big') + b'\x03'
    dri = h.index(b'\xff\xdd')
    assert h[dri + 2:dri + 6] == b'\x00\x04' + (188).to_bytes(2, 'big')
    assert h[-14:-12] == b'\xff\xda' and h.count(b'\xff\xc4') == 4 and h.count(b'\xff\xdb') == 2
    for bad in ((0, 5), (5, 65536)):
        with pytest.raises(ValueError):
            A.jpeg_header(*bad, A.quant_tables(90))
    with pytest.raises(ValueError):
        A.jpeg_header(8, 8, np.zeros((2, 64), np.int64))
