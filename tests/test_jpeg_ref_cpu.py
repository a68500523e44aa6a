"""tests/jpeg_ref.py pinned without a GPU: its entropy coder against its own decoder, its integer
DCT against the float64 DCT, its files against PIL (libjpeg) as an independent decoder and
encoder, its tables against a2m.jpeg's, and one golden file.

Bounds, each from a measurement on the CPU ("JPEG encoder", carries the figures):
  DCT_BOUND    largest |integer DCT - float64 DCT| over the blocks below measured 0.5721: 0.5 of
               the final rounding, the rest from the 13-bit matrix (an entry is off by up to
               2^-14, which two passes over samples of 128 can raise to 0.35) and the six fraction
               bits kept after the first pass (0.02).  The bound is the measurement rounded up
               to 0.6.
  PIL margins  libjpeg's forward DCT rounds differently (a coefficient that sits near a rounding
               boundary lands one quantiser step away from ours), so per frame our decode error
               is compared with libjpeg's own on the same planes and tables.  Measured over the
               39 frames below: our maximum error never exceeds libjpeg's (MAX_MARGIN = 0); our
               mean-square error exceeds it by at most 0.48 % where it is large (quality 50
               noise, about 510) and by at most 0.021 where it is small (quality 100 noise,
               0.104 against 0.083 on 384 samples), so the margin is 1 % of libjpeg's plus 0.03.
"""
import io
import os

import numpy as np
import pytest

import jpeg_ref as J

DCT_BOUND = 0.6
MAX_MARGIN = 0
MSE_MARGIN = 0.01, 0.03      # relative, absolute
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg_ref_13x9_q50.jpg')
GOLDEN_CASE = next(i for i, c in enumerate(J.CASES) if J.case_id(c) == 'noise-13x9x2-q16')
CASE_IDS = [J.case_id(c) for c in J.CASES]
# the 260-frame case exists for the device's scan over frames, which PIL never sees (every frame is
# its own file); its 8 x 8 frames would only repeat noise-8x8x1 259 times
PIL_INDICES = [i for i, c in enumerate(J.CASES) if c[1] != J.MANY]


@pytest.mark.parametrize('index', range(len(J.CASES)), ids=CASE_IDS)
def test_decoder_returns_the_quantised_coefficients(index):
    content, (W, H, N), qt = J.CASES[index]
    frames, files = J.encoded_case(index)
    assert len(files) == N
    for fr, data in zip(frames, files):
        got = J.decode(data)
        assert (got['W'], got['H'], got['dri']) == (W, H, (W + 7) // 8)
        assert np.array_equal(got['qt'], qt)
        assert np.array_equal(got['coef'], J.coefficients(fr, qt))
        MH = (H + 7) // 8
        assert got['restarts'] == [r % 8 for r in range(MH - 1)]


def test_cases_have_the_structure_they_are_named_for():
    by_id = {J.case_id(c): J.encoded_case(i) for i, c in enumerate(J.CASES)}
    coef = J.decode(by_id['white-16x8x3-q3'][1][0])['coef']
    assert (coef[..., 1:] == 0).all() and coef[0, 0, 0, 0] != 0               # DC + EOB only
    coef = J.decode(by_id['last_ac-16x8x3-q16'][1][0])['coef']
    assert (coef[..., 1:63] == 0).all() and (coef[..., 63] != 0).all()        # three ZRLs, no EOB
    coef = J.decode(by_id['zz17-16x8x3-q16'][1][0])['coef']
    assert (coef[..., 1:17] == 0).all() and (coef[..., 17] != 0).all() and (coef[..., 18:] == 0).all()
    coef = J.decode(by_id['alternating-16x8x3-q1'][1][0])['coef']
    assert abs(int(coef[0, 1, 0, 0]) - int(coef[0, 0, 0, 0])) == 2040         # DC category 11
    assert J.decode(by_id['noise-8x80x1-q1'][1][0])['restarts'] == [0, 1, 2, 3, 4, 5, 6, 7, 0]
    noise = by_id['noise-200x64x2-q1'][1][0]
    assert noise.count(b'\xff\x00') > 20                                      # stuffed bytes


def test_integer_dct_against_float64():
    rng = np.random.default_rng(3)
    y, x = np.arange(8)[:, None], np.arange(8)[None]
    checker = np.where((x + y) % 2 == 0, 127, -128)
    blocks = np.concatenate([
        rng.integers(-128, 128, (4000, 8, 8)),
        np.stack([np.full((8, 8), -128), np.full((8, 8), 127), checker, -1 - checker,
                  np.where((x + 0 * y) % 2 == 0, 127, -128), np.where((y + 0 * x) % 2 == 0, -128, 127)]),
        rng.choice([-128, 127], (2000, 8, 8))])
    err = np.abs(J.dct_int(blocks) - J.dct_float(blocks)).max()
    print(f'integer DCT against float64: largest difference {err:.4f}')
    assert err <= DCT_BOUND
    d = J.dct_int(blocks)
    assert np.abs(d[..., 0, 0]).max() <= 1024 and np.abs(d.reshape(-1, 64)[:, 1:]).max() <= 928


def test_tables_are_those_of_the_package():
    """a2m.jpeg holds its own copy of the Annex K tables and writes the header the device scan
    belongs to: both must be what the restatement uses."""
    from a2m import jpeg as A
    for q in (1, 50, 90, 100):
        assert np.array_equal(A.quant_tables(q), J.quant_tables(q))
        assert A.jpeg_header(13, 9, A.quant_tables(q)) == J.header(13, 9, J.quant_tables(q))
    assert tuple(J.ZIGZAG) == A.ZIGZAG


def _pil_decode(data, W, H):
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    assert im.format == 'JPEG' and im.size == (W, H)
    im.draft('YCbCr', (W, H))
    assert im.mode == 'YCbCr'
    return np.asarray(im).transpose(2, 0, 1).astype(np.int64)


@pytest.mark.parametrize('index', PIL_INDICES, ids=[CASE_IDS[i] for i in PIL_INDICES])
def test_pil_decodes_our_files_as_well_as_its_own(index):
    pytest.importorskip('PIL')
    from PIL import Image
    content, (W, H, N), qt = J.CASES[index]
    frames, files = J.encoded_case(index)
    for fr, data in zip(frames, files):
        ours = _pil_decode(data, W, H) - fr
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(fr.transpose(1, 2, 0)), 'YCbCr').save(
            buf, 'JPEG', subsampling=0, optimize=False, qtables=[[int(v) for v in t] for t in qt])
        theirs = _pil_decode(buf.getvalue(), W, H) - fr
        o_max, t_max = np.abs(ours).max(), np.abs(theirs).max()
        o_mse, t_mse = (ours ** 2).mean(), (theirs ** 2).mean()
        print(f'{CASE_IDS[index]}: max error ours {o_max} libjpeg {t_max}; '
              f'mean-square ours {o_mse:.4f} libjpeg {t_mse:.4f}')
        assert o_max <= t_max + MAX_MARGIN
        assert o_mse <= t_mse * (1 + MSE_MARGIN[0]) + MSE_MARGIN[1]


def test_pil_reads_the_dht_segments_pil_writes():
    """The Huffman tables are Annex K's: the four DHT segments equal those of a baseline file
    that libjpeg writes without optimisation."""
    pytest.importorskip('PIL')
    from PIL import Image
    buf = io.BytesIO()
    Image.new('YCbCr', (16, 16)).save(buf, 'JPEG', optimize=False, subsampling=0, quality=50)
    theirs, ours = buf.getvalue(), J.header(16, 16, J.quant_tables(50))

    def segments(data, marker):
        out, i = [], 2
        while data[i + 1] != 0xDA:
            length = int.from_bytes(data[i + 2:i + 4], 'big')
            if data[i + 1] == marker:
                out.append(data[i + 4:i + 2 + length])
            i += 2 + length
        return out
    assert sorted(segments(ours, 0xC4)) == sorted(segments(theirs, 0xC4))
    assert segments(ours, 0xDB) == segments(theirs, 0xDB)         # quality 50 = the Annex K tables


def test_idct_of_the_decoded_coefficients_is_close_to_the_source():
    """The decoder's output is meaningful without PIL too: a float64 inverse DCT of what it
    returns reproduces a quality-100 noise frame to within 2 grey levels."""
    index = CASE_IDS.index('noise-13x9x2-q1')
    frames, files = J.encoded_case(index)
    got = J.decode(files[0])
    back = J.idct_planes(got['coef'], got['qt'], 13, 9)
    assert np.abs(back.astype(int) - frames[0]).max() <= 2


def test_golden_file():
    frames, files = J.encoded_case(GOLDEN_CASE)
    with open(GOLDEN, 'rb') as f:
        assert f.read() == files[0]
