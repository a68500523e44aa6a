"""A numpy restatement of the byte stream that include/a2m.h specifies for a2m_jpeg_encode_u8
(baseline JPEG, 4:4:4, one MCU row per restart interval), a decoder for it, and the cases that
tests/test_jpeg_ref_cpu.py and tests/test_gpu_jpeg.py share.

The level shift, DCT and quantisation are integer numpy; the Huffman coding is a Python loop.
Nothing here imports a2m: the tables are this file's own copy of ITU-T T.81 Annex K.
"""
import functools
import struct

import numpy as np

C = (2896, 4017, 3784, 3406, 2896, 2276, 1567, 799)     # A2M_JPEG_C0 .. C7
PASS1_SHIFT, PASS2_SHIFT = 7, 19

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5,
                   12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                   58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

BASE_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55,
             14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
BASE_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
               24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32

DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66,
     177, 193, 21, 82, 209, 240, 36, 51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41,
     42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88, 89, 90,
     99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166,
     167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199,
     200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231,
     232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250],
    [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161,
     177, 193, 9, 35, 51, 82, 240, 21, 98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38,
     39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74, 83, 84, 85, 86, 87, 88,
     89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
     132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164,
     165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197,
     198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230,
     231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])


def quant_tables(quality):
    """libjpeg's jpeg_set_quality -> int [2, 64], natural order."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array([BASE_LUMA, BASE_CHROMA]) * scale + 50) // 100, 1, 255)


def dct_matrix():
    m = np.zeros((8, 8), np.int64)
    for u in range(8):
        for x in range(8):
            k = (2 * x + 1) * u % 32
            sign = 1
            if k > 16:
                k = 32 - k
            if k > 8:
                k, sign = 16 - k, -1
            m[u, x] = C[0] if u == 0 else sign * C[k]
    return m


M = dct_matrix()


def dct_int(s):
    """s int [..., 8(y), 8(x)] level-shifted samples -> d int [..., 8(v), 8(u)]."""
    s = np.asarray(s, np.int64)
    a = np.einsum('...yx,ux->...yu', s, M)
    assert np.abs(a).max(initial=0) < 2 ** 31
    t = (a + (1 << (PASS1_SHIFT - 1))) >> PASS1_SHIFT
    b = np.einsum('...yu,vy->...vu', t, M)
    assert np.abs(b).max(initial=0) < 2 ** 31
    return (b + (1 << (PASS2_SHIFT - 1))) >> PASS2_SHIFT


def dct_float(s):
    """The orthonormal DCT-II in float64."""
    u, x = np.arange(8)[:, None], np.arange(8)[None]
    B = 0.5 * np.where(u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16)
    return np.einsum('vy,...yx,ux->...vu', B, np.asarray(s, np.float64), B)


def blocks_of(planes):
    """uint8 [3, H, W] -> level-shifted int [MH, MW, 3, 8, 8], edges replicated."""
    _, H, W = planes.shape
    MH, MW = (H + 7) // 8, (W + 7) // 8
    ys, xs = np.minimum(np.arange(8 * MH), H - 1), np.minimum(np.arange(8 * MW), W - 1)
    p = planes[:, ys][:, :, xs].astype(np.int64) - 128
    return p.reshape(3, MH, 8, MW, 8).transpose(1, 3, 0, 2, 4)


def quantise(d, qt):
    """d int [MH, MW, 3, 8, 8], qt [2, 64] natural -> int [MH, MW, 3, 64] in zig-zag order."""
    Q = np.asarray(qt, np.int64)[[0, 1, 1]].reshape(3, 8, 8)
    mag = (2 * np.abs(d) + Q) // (2 * Q)
    lim = np.full((8, 8), 1023)
    lim[0, 0] = 1024
    q = np.sign(d) * np.minimum(mag, lim)
    return q.reshape(*q.shape[:3], 64)[..., ZIGZAG]


def coefficients(planes, qt):
    return quantise(dct_int(blocks_of(planes)), qt)


def huff_codes(bits, vals):
    """symbol -> (code, length), T.81 Annex C."""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = [huff_codes(DC_BITS[t], DC_VALS[t]) for t in range(2)]
AC_CODES = [huff_codes(AC_BITS[t], AC_VALS[t]) for t in range(2)]


def _value_bits(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def encode_interval(row):
    """row int [MW, 3, 64] -> the interval's bytes: padded with 1-bits, 0xFF stuffed."""
    acc, n = 0, 0

    def put(code, length):
        nonlocal acc, n
        acc = (acc << length) | code
        n += length

    pred = [0, 0, 0]
    for mcu in row:
        for c in range(3):
            t = int(c != 0)
            blk = [int(v) for v in mcu[c]]
            size, bits = _value_bits(blk[0] - pred[c])
            pred[c] = blk[0]
            put(*DC_CODES[t][size])
            put(bits, size)
            run = 0
            for k in range(1, 64):
                if blk[k] == 0:
                    run += 1
                    continue
                while run >= 16:
                    put(*AC_CODES[t][0xF0])
                    run -= 16
                size, bits = _value_bits(blk[k])
                put(*AC_CODES[t][(run << 4) | size])
                put(bits, size)
                run = 0
            if run:
                put(*AC_CODES[t][0x00])
    pad = -n % 8
    put((1 << pad) - 1, pad)
    return acc.to_bytes(n // 8, 'big').replace(b'\xff', b'\xff\x00')


def encode_scan(coef):
    """coef int [MH, MW, 3, 64] -> the frame's entropy-coded scan."""
    out = []
    for r, row in enumerate(coef):
        if r:
            out.append(bytes([0xFF, 0xD0 + (r - 1) % 8]))
        out.append(encode_interval(row))
    return b''.join(out)


def _segment(marker, payload):
    return struct.pack('>BBH', 0xFF, marker, len(payload) + 2) + payload


def header(W, H, qt):
    qt = np.asarray(qt)
    out = [b'\xff\xd8', _segment(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')]
    for t in range(2):
        out.append(_segment(0xDB, bytes([t]) + bytes(int(v) for v in qt[t][ZIGZAG])))
    out.append(_segment(0xC0, struct.pack('>BHHB', 8, H, W, 3) + bytes([1, 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, bits, vals in ((0x00, DC_BITS[0], DC_VALS[0]), (0x10, AC_BITS[0], AC_VALS[0]),
                              (0x01, DC_BITS[1], DC_VALS[1]), (0x11, AC_BITS[1], AC_VALS[1])):
        out.append(_segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals)))
    out.append(_segment(0xDD, struct.pack('>H', (W + 7) // 8)))
    out.append(_segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    return b''.join(out)


def encode(planes, qt):
    """uint8 [3, H, W] Y, Cb, Cr planes -> a complete file."""
    _, H, W = planes.shape
    return header(W, H, qt) + encode_scan(coefficients(planes, qt)) + b'\xff\xd9'


# ------------------------------------------------------------------------------ decoder
def decode(data):
    """A file as `encode` writes it -> dict(W, H, qt [2, 64] natural, dri, coef [MH, MW, 3, 64]
    zig-zag with the DC prediction undone, restarts: the RSTn numbers met).  Every table is read
    from the file's own segments."""
    assert data[:2] == b'\xff\xd8' and data[-2:] == b'\xff\xd9'
    i, qt, huff, info = 2, {}, {}, {}
    while True:
        assert data[i] == 0xFF, hex(data[i])
        marker, length = data[i + 1], struct.unpack('>H', data[i + 2:i + 4])[0]
        seg = data[i + 4:i + 2 + length]
        i += 2 + length
        if marker == 0xDB:
            assert seg[0] in (0, 1) and len(seg) == 65          # 8-bit table
            table = np.zeros(64, np.int64)
            table[ZIGZAG] = list(seg[1:])
            qt[seg[0]] = table
        elif marker == 0xC0:
            prec, H, W, nc = struct.unpack('>BHHB', seg[:6])
            assert prec == 8 and nc == 3
            info['comps'] = [tuple(seg[6 + 3 * c:9 + 3 * c]) for c in range(3)]
            assert all(c[1] == 0x11 for c in info['comps'])     # 4:4:4
        elif marker == 0xC4:
            p = 0
            while p < len(seg):
                bits = list(seg[p + 1:p + 17])
                vals = list(seg[p + 17:p + 17 + sum(bits)])
                huff[seg[p]] = {(ln, code): sym for sym, (code, ln) in huff_codes(bits, vals).items()}
                p += 17 + sum(bits)
        elif marker == 0xDD:
            info['dri'] = struct.unpack('>H', seg)[0]
        elif marker == 0xDA:
            assert seg[0] == 3 and tuple(seg[7:]) == (0, 63, 0)
            sel = [seg[2 + 2 * c] for c in range(3)]
            break
        else:
            assert marker == 0xE0, hex(marker)
    MH, MW = (H + 7) // 8, (W + 7) // 8
    assert info['dri'] == MW
    scan, restarts, parts, start, j = data[i:-2], [], [], 0, 0
    while j < len(scan):                  # split at RSTn; 0xFF 0x00 is a stuffed byte
        if scan[j] == 0xFF:
            assert j + 1 < len(scan) and (scan[j + 1] == 0 or 0xD0 <= scan[j + 1] <= 0xD7), 'stray marker'
            if scan[j + 1] != 0:
                restarts.append(scan[j + 1] - 0xD0)
                parts.append(scan[start:j])
                start = j + 2
            j += 2
        else:
            j += 1
    parts.append(scan[start:])
    assert len(parts) == MH
    coef = np.zeros((MH, MW, 3, 64), np.int64)
    for r, part in enumerate(parts):
        raw = part.replace(b'\xff\x00', b'\xff')
        bits = bin(int.from_bytes(b'\x01' + raw, 'big'))[3:]
        pos, pred = 0, [0, 0, 0]

        def symbol(table):
            nonlocal pos
            code = 0
            for ln in range(1, 17):
                code = (code << 1) | (bits[pos + ln - 1] == '1')
                if (ln, code) in table:
                    pos += ln
                    return table[(ln, code)]
            raise AssertionError('no Huffman code matches')

        def value(size):
            nonlocal pos
            if size == 0:
                return 0
            v = int(bits[pos:pos + size], 2)
            pos += size
            return v if v >> (size - 1) else v - (1 << size) + 1

        for m in range(MW):
            for c in range(3):
                pred[c] += value(symbol(huff[sel[c] >> 4]))
                coef[r, m, c, 0] = pred[c]
                k = 1
                while k < 64:
                    rs = symbol(huff[0x10 | (sel[c] & 15)])
                    if rs == 0:
                        break
                    if rs == 0xF0:
                        k += 16
                        continue
                    k += rs >> 4
                    coef[r, m, c, k] = value(rs & 15)
                    k += 1
                assert k <= 64
        assert len(bits) - pos < 8 and set(bits[pos:]) <= {'1'}, 'an interval ends with 1-bits'
    return dict(W=W, H=H, qt=np.stack([qt[0], qt[1]]), dri=info['dri'], coef=coef, restarts=restarts)


def idct_planes(coef, qt, W, H):
    """Float64 reconstruction (dequantise, inverse orthonormal DCT, +128, clip, round)."""
    u, x = np.arange(8)[:, None], np.arange(8)[None]
    B = 0.5 * np.where(u == 0, np.sqrt(0.5), 1.0) * np.cos((2 * x + 1) * u * np.pi / 16)
    nat = np.zeros(coef.shape, np.float64)
    nat[..., ZIGZAG] = coef
    d = nat.reshape(*coef.shape[:3], 8, 8) * np.asarray(qt, np.float64)[[0, 1, 1]].reshape(3, 8, 8)
    px = np.einsum('vy,...vu,ux->...yx', B, d, B) + 128
    MH, MW = coef.shape[:2]
    full = px.transpose(2, 0, 3, 1, 4).reshape(3, 8 * MH, 8 * MW)[:, :H, :W]
    return np.clip(np.floor(full + 0.5), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------ the cases
SHAPES = ((8, 8, 1), (16, 8, 3), (13, 9, 2), (8, 80, 1), (200, 64, 2))      # (W, H, N)
# beyond them, where the device code takes another path: 261 blocks in one interval (its scan of
# block sizes runs 256 at a time) and 260 frames (so does its scan of frame sizes)
WIDE, MANY = (696, 8, 1), (8, 8, 260)
FLAT16 = np.full((2, 64), 16)
# (content, (W, H, N), quantiser tables)
CASES = tuple(
    [(content, shape, qt) for shape in SHAPES[:4]
     for content, qt in (('white', quant_tables(90)), ('noise', quant_tables(100)),
                         ('noise', quant_tables(50)), ('alternating', quant_tables(100)))] +
    [('last_ac', SHAPES[1], FLAT16), ('zz17', SHAPES[1], FLAT16),
     ('noise', SHAPES[4], quant_tables(100)), ('lines', SHAPES[4], quant_tables(90)),
     ('noise', WIDE, quant_tables(50)), ('noise', MANY, quant_tables(50))])


def case_id(case):
    content, (W, H, N), qt = case
    return f'{content}-{W}x{H}x{N}-q{int(qt[0, 0])}'


def _cosine_block(v, u, amplitude):
    y, x = np.arange(8)[:, None], np.arange(8)[None]
    return 128 + amplitude * np.cos((2 * y + 1) * v * np.pi / 16) * np.cos((2 * x + 1) * u * np.pi / 16)


def case_frames(content, shape):
    """uint8 [N, 3, H, W].  'lines' is synthetic here (thin coloured lines on white); the GPU
    test replaces it by a frame from render_poses."""
    W, H, N = shape
    rng = np.random.default_rng(1000 * W + 10 * H + N)
    if content == 'white':
        fr = np.empty((N, 3, H, W), np.uint8)
        fr[:, 0], fr[:, 1:] = 255, 128
    elif content == 'noise':
        fr = rng.integers(0, 256, (N, 3, H, W), dtype=np.uint8)
    elif content == 'alternating':
        yy, xx = np.arange(H)[:, None] // 8, np.arange(W)[None] // 8
        fr = np.broadcast_to((((yy + xx) % 2) * 255).astype(np.uint8), (N, 3, H, W)).copy()
        fr[:, 1] = 255 - fr[:, 1]
    elif content in ('last_ac', 'zz17'):
        # 4 * amplitude / 16 = 5 after quantisation; rounding the pixels moves every other
        # coefficient by less than 8, which a quantiser of 16 takes to 0
        v, u = (7, 7) if content == 'last_ac' else divmod(int(ZIGZAG[17]), 8)
        blk = np.floor(_cosine_block(v, u, 20.0) + 0.5).astype(np.uint8)
        fr = np.broadcast_to(np.tile(blk, ((H + 7) // 8, (W + 7) // 8))[:H, :W], (N, 3, H, W)).copy()
    elif content == 'lines':
        fr = np.empty((N, 3, H, W), np.uint8)
        fr[:, 0], fr[:, 1:] = 255, 128
        for n in range(N):
            for _ in range(6):
                x0, y0 = rng.integers(0, W), rng.integers(0, H)
                t = np.arange(40)
                xs, ys = np.clip(x0 + t, 0, W - 1), np.clip(y0 + (t * rng.uniform(-1, 1)).astype(int), 0, H - 1)
                fr[n, :, ys, xs] = rng.integers(0, 256, 3, dtype=np.uint8)
    else:
        raise KeyError(content)
    return fr


@functools.lru_cache(maxsize=None)
def _encoded(index):
    content, shape, qt = CASES[index]
    frames = case_frames(content, shape)
    frames.setflags(write=False)
    return frames, tuple(encode(fr, qt) for fr in frames)


def encoded_case(index):
    """-> (frames uint8 [N, 3, H, W], tuple of N files); computed once, shared, read-only."""
    return _encoded(index)
