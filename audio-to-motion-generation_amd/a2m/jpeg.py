"""Baseline JPEG on the device (csrc/jpeg.hip; the byte stream is specified in include/a2m.h):
planar full-range YCbCr frames uint8 [N, 3, H, W], as a2m.video.render_poses draws them from a
palette converted by a2m.video.rgb_to_ycbcr_full, to 4:4:4 baseline sequential JPEG files whose
restart interval is one MCU row.  Only the compressed bytes cross to the host.

  quant_tables(quality)                  libjpeg's scaling of the ITU-T T.81 Annex K tables
  jpeg_header(W, H, qtables)             SOI, APP0/JFIF, DQT, SOF0, DHT, DRI, SOS
  encode_scans(frames, qtables)          -> (host uint8 buffer, int64 offsets [N + 1])
  encode_scans_into(frames, qtables, out, offsets, ws)   the launches alone (graph capture)
  encode_jpeg(frames, quality, qtables)  -> list of N bytes objects, each a complete file
  free_buffers()                         drop the buffers encode_scans keeps between calls

No PIL, libjpeg or ffmpeg is used.  The Huffman tables are the typical tables of Annex K (K.3-K.6)
and are written into every header, so any baseline decoder reads the files.
"""
import struct

import numpy as np
import torch

from . import functional as F
from ._native import check, lib

# ITU-T T.81 Annex K.1 / K.2 in natural (row-major) order: entry [8 v + u] divides coefficient (v, u)
BASE_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
             14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
BASE_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
               24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32

# ZIGZAG[k] = natural index 8 v + u of the k-th coefficient in zig-zag order
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
          12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
          58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)

# Annex K.3-K.6: (BITS: codes of length 1..16, HUFFVAL: the symbols in code order)
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125), (
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07,
    0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0,
    0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28,
    0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49,
    0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
    0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7,
    0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5,
    0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119), (
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71,
    0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0,
    0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
    0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
    0xf9, 0xfa))

EOI = b'\xff\xd9'


def quant_tables(quality):
    """libjpeg's jpeg_set_quality: the Annex K tables scaled by 5000/quality below 50 and by
    200 - 2 quality from 50 up, clamped to the 8-bit range of baseline tables.
    -> uint16 [2, 64] (luma, chroma) in natural order."""
    q = int(quality)
    if q != quality or not 1 <= q <= 100:
        raise ValueError(f'quality must be an integer in [1, 100], got {quality!r}')
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([BASE_LUMA, BASE_CHROMA], np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


def _qtables(qtables):
    qt = np.asarray(qtables)
    if qt.shape != (2, 64) or not np.issubdtype(qt.dtype, np.integer) or qt.min() < 1 or qt.max() > 255:
        raise ValueError('qtables are two tables (luma, chroma) of 64 integers in [1, 255], natural order')
    return np.ascontiguousarray(qt.astype(np.uint16))


def _segment(marker, payload):
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def jpeg_header(W, H, qtables):
    """Everything of the file before the entropy-coded scan."""
    if not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f'a JPEG frame is 1..65535 pixels a side, got {W} x {H}')
    qt = _qtables(qtables)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    for t in range(2):
        out.append(_segment(0xDB, bytes([t]) + bytes(int(qt[t, z]) for z in ZIGZAG)))
    out.append(_segment(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack('>H', (W + 7) // 8)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(out)


def _frames(frames):
    if not (torch.is_tensor(frames) and frames.dtype == torch.uint8 and frames.dim() == 4
            and frames.shape[1] == 3):
        raise ValueError('frames must be a uint8 device tensor [N, 3, H, W] of Y, Cb, Cr planes')
    if not frames.is_cuda:
        raise RuntimeError('a2m ops need device tensors (no CPU fallback); got a CPU tensor')
    N, _, H, W = frames.shape
    if N and not (1 <= W <= 65535 and 1 <= H <= 65535):
        raise ValueError(f'a JPEG frame is 1..65535 pixels a side, got {W} x {H}')
    return frames.contiguous(), N, H, W


def workspace_bytes(N, W, H):
    return int(lib.a2m_jpeg_ws_bytes(N, W, H))


def encode_scans_into(frames, qtables, out, offsets, ws):
    """The stream-ordered launches alone, no copy and no synchronisation (so a graph can capture
    them): frames uint8 [N, 3, H, W] -> the frames' scans back to back in `out` (uint8 device
    tensor, its length is the capacity) and their positions in `offsets` (int64 device tensor
    [N + 1]).  ws: a uint8 device tensor of workspace_bytes(N, W, H).  Scan bytes beyond the
    capacity are dropped, never written: offsets[N] > len(out) says so and is the size needed."""
    frames, N, H, W = _frames(frames)
    qt = _qtables(qtables)
    for t, dt, n in ((out, torch.uint8, None), (offsets, torch.int64, N + 1), (ws, torch.uint8, None)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.dim() == 1 and t.is_contiguous()
                and (n is None or t.numel() == n)):
            raise ValueError('out and ws are contiguous uint8 device vectors, offsets int64 [N + 1]')
    if N == 0:
        offsets.zero_()
        return
    check(lib.a2m_jpeg_encode_u8(F._p(frames), N, W, H, qt[0].ctypes.data, qt[1].ctypes.data, F._p(out),
                                 out.numel(), F._p(offsets), F._p(ws), ws.numel(), F._stream()),
          value_error=True)


_cache = {}     # per device: workspace, output buffer, pinned host buffer (grown, never shrunk)


def _buffer(key, nbytes, pinned=False):
    buf = _cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(nbytes, dtype=torch.uint8).pin_memory() if pinned else \
            torch.empty(nbytes, dtype=torch.uint8, device=key[1])
        _cache[key] = buf
    return buf


def free_buffers():
    """Drop the cached workspace, output and pinned buffers (the workspace is 340 bytes a block:
    773 MB for 64 frames of 1500 x 500)."""
    _cache.clear()


def encode_scans(frames, qtables, capacity=None):
    """frames -> (host uint8 numpy buffer of offsets[N] bytes, int64 numpy offsets [N + 1]): frame
    i's entropy-coded scan is buffer[offsets[i]:offsets[i + 1]].  Two copies cross to the host:
    the offsets, then offsets[N] bytes through a pinned buffer.  capacity: the first guess of the
    output size in bytes (default: an eighth of the raw frames); when the scans need more, the
    encoder says how much and the call runs once more with a buffer of that size.  The returned
    buffer is a view of a pinned buffer that the next call on this device reuses: copy what must
    outlive it."""
    frames, N, H, W = _frames(frames)
    qt = _qtables(qtables)
    if N == 0:
        return np.empty(0, np.uint8), np.zeros(1, np.int64)
    dev = str(frames.device)
    ws = _buffer(('ws', dev), workspace_bytes(N, W, H))
    cap = int(capacity) if capacity is not None else N * (3 * H * W // 8 + 4096)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=frames.device)
    for attempt in range(2):
        out = _buffer(('out', dev), cap)
        out = out[:cap] if capacity is not None else out
        encode_scans_into(frames, qt, out, offsets, ws)
        off = offsets.cpu().numpy()
        need = int(off[N])
        if need <= out.numel():
            break
        cap, capacity = need, None
    else:
        raise RuntimeError(f'jpeg: the scans need {need} bytes after a retry sized by the encoder')
    host = _buffer(('host', dev), max(need, 1), pinned=True)[:need]
    host.copy_(out[:need], non_blocking=True)
    torch.cuda.current_stream().synchronize()
    return host.numpy(), off


def encode_jpeg(frames, quality=90, qtables=None):
    """Device uint8 [N, 3, H, W] full-range Y, Cb, Cr planes -> list of N bytes, each a complete
    baseline JPEG file (header + scan + EOI).  qtables (uint16 [2, 64], natural order) overrides
    quality."""
    frames, N, H, W = _frames(frames)
    qt = _qtables(quant_tables(quality) if qtables is None else qtables)
    if N == 0:
        return []
    buf, off = encode_scans(frames, qt)
    header = jpeg_header(W, H, qt)
    return [header + buf[off[i]:off[i + 1]].tobytes() + EOI for i in range(N)]
