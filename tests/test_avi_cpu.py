"""a2m.avi without a GPU: the writer, the reader and the remuxer on hand-made payloads."""
import struct
import wave

import numpy as np
import pytest


def _frames(n, odd=True):
    return [b'\xff\xd8' + bytes([i]) * (2 * i + (1 if odd else 2)) + b'\xff\xd9' for i in range(n)]


def _walk(data):
    """[(fourcc or list kind, position, size)] of every chunk and list, depth first; asserts that
    every chunk is padded to even length and every list is filled exactly."""
    out = []

    def walk(lo, hi):
        while lo < hi:
            cc, size = data[lo:lo + 4], struct.unpack('<I', data[lo + 4:lo + 8])[0]
            assert lo % 2 == 0 and lo + 8 + size <= hi
            if cc == b'LIST':
                out.append((data[lo + 8:lo + 12], lo, size))
                walk(lo + 12, lo + 8 + size)
            else:
                out.append((cc, lo, size))
            lo += 8 + size + (size & 1)
        assert lo == hi

    assert data[:4] == b'RIFF' and data[8:12] == b'AVI '
    assert struct.unpack('<I', data[4:8])[0] == len(data) - 8
    walk(12, len(data))
    return out


def test_video_only_with_odd_chunks(tmp_path):
    from a2m import avi
    fn = str(tmp_path / 'v.avi')
    frames = _frames(5)
    assert all(len(f) % 2 for f in frames)
    with avi.AVIWriter(fn, 97, 41) as w:
        for f in frames:
            w.write_frame(f[:2], f[2:-2], f[-2:])             # pieces are concatenated
        assert w.frames == 5
    data = open(fn, 'rb').read()
    tree = _walk(data)
    assert [t[0] for t in tree] == [b'hdrl', b'avih', b'strl', b'strh', b'strf', b'movi'] + [b'00dc'] * 5 + [b'idx1']
    assert [t[2] for t in tree if t[0] == b'00dc'] == [len(f) for f in frames]
    got = avi.read_avi(fn)
    assert got['frames'] == frames and (got['W'], got['H'], got['fps']) == (97, 41, (30000, 2002))
    assert got['audio_rate'] is None and len(got['audio']) == 0
    for (cc, off, size), f in zip(got['index'], frames):
        pos = got['movi'] + off
        assert cc == b'00dc' and data[pos:pos + 4] == b'00dc' and data[pos + 8:pos + 8 + size] == f
    avih = struct.unpack('<14I', data[32:88])
    assert avih[3] == 0x10 and avih[4] == 5 and avih[6] == 1 and avih[7] == max(map(len, frames))


@pytest.mark.parametrize('seconds', [0.1, 0.3337, 2.0], ids=['shorter', 'about_equal', 'longer'])
def test_audio_is_split_by_cumulative_floor_and_cut_to_the_picture(tmp_path, seconds):
    from a2m import avi
    sr, n = 11025, 5                                           # 5 frames = 0.33367 s = 3678 samples
    rng = np.random.default_rng(1)
    sound = rng.uniform(-1.2, 1.2, int(sr * seconds))
    pcm = avi.pcm16(sound)
    assert pcm.dtype == np.dtype('<i2') and pcm.max() == 32767 and pcm.min() == -32767
    assert np.array_equal(pcm, np.rint(np.clip(sound, -1, 1) * 32767).astype(np.int16))
    fn = str(tmp_path / 'a.avi')
    with avi.AVIWriter(fn, 16, 8, audio_rate=sr) as w:
        w.set_audio(pcm)
        for f in _frames(n, odd=False):
            w.write_frame(f)
        with pytest.raises(ValueError):
            w.set_audio(pcm)                                   # too late
    got = avi.read_avi(fn)
    total = min(len(pcm), n * sr * 2002 // 30000)
    assert got['audio_rate'] == sr and np.array_equal(got['audio'], pcm[:total])
    sizes = [size // 2 for cc, _, size in got['index'] if cc == b'01wb']
    bounds = [min(len(pcm), i * sr * 2002 // 30000) for i in range(n + 1)]
    assert sizes == list(np.diff(bounds)) and [cc for cc, _, _ in got['index']] == [b'00dc', b'01wb'] * n
    _walk(open(fn, 'rb').read())
    data = open(fn, 'rb').read()
    auds = data.index(b'auds')
    assert struct.unpack('<I', data[auds + 32:auds + 36])[0] == total        # dwLength in samples


def test_the_2_gib_guard(tmp_path):
    from a2m import avi
    fn = str(tmp_path / 'big.avi')
    w = avi.AVIWriter(fn, 16, 8)
    w.write_frame(b'\xff\xd8\xff\xd9')
    real = w._size
    frame = b'x' * 1000
    w._size = avi.LIMIT - (8 + 1000) - (8 + 16 * 2)            # the counter, stubbed: the frame just fits
    w.write_frame(frame)
    w._size = avi.LIMIT - (8 + 1000) - (8 + 16 * 3) + 1        # one byte too many with the index
    with pytest.raises(ValueError, match='2 GiB'):
        w.write_frame(frame)
    assert w.frames == 2
    w._size = real + 8 + 1000
    w.close()
    assert len(avi.read_avi(fn)['frames']) == 2
    with pytest.raises(ValueError):
        w.write_frame(frame)                                   # closed


def test_argument_checks(tmp_path):
    from a2m import avi
    for bad in (dict(path='x.mp4'), dict(W=0), dict(H=70000), dict(fps=(0, 1)), dict(audio_rate=0)):
        kw = dict(path=str(tmp_path / 'x.avi'), W=16, H=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            avi.AVIWriter(**kw)
    with avi.AVIWriter(str(tmp_path / 'x.avi'), 16, 8) as w:
        with pytest.raises(ValueError):
            w.set_audio(np.zeros(4, np.int16))                 # opened without audio_rate
    with pytest.raises(ValueError):
        avi.pcm16(np.zeros((2, 4)))


def _write_wav(path, pcm, rate, channels=1, width=2):
    with wave.open(str(path), 'wb') as w:
        w.setnchannels(channels)
        w.setsampwidth(width)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(pcm).tobytes())


def test_save_video_from_audio_video(tmp_path):
    from a2m import avi
    from a2m import video as V
    assert V.save_video_from_audio_video is avi.save_video_from_audio_video
    frames = _frames(6)
    silent = str(tmp_path / 'silent.avi')
    with avi.AVIWriter(silent, 40, 30, fps=(15, 1)) as w:
        for f in frames:
            w.write_frame(f)
    rng = np.random.default_rng(2)
    stereo = rng.integers(-32768, 32768, (16000, 2)).astype('<i2')           # 1 s; the video is 0.4 s
    _write_wav(tmp_path / 'speech.wav', stereo, 16000, channels=2)
    out = str(tmp_path / 'with_sound.avi')
    assert avi.save_video_from_audio_video(str(tmp_path / 'speech.wav'), silent, out) == 6
    got = avi.read_avi(out)
    assert got['frames'] == frames and got['fps'] == (15, 1) and got['audio_rate'] == 16000
    mono = np.rint(stereo.astype(np.float64).mean(1)).astype('<i2')
    assert np.array_equal(got['audio'], mono[:6 * 16000 // 15])
    _walk(open(out, 'rb').read())
    # a file that already has sound is accepted; its sound is replaced
    again = str(tmp_path / 'again.avi')
    _write_wav(tmp_path / 'short.wav', mono[:100], 8000)
    assert avi.save_video_from_audio_video(str(tmp_path / 'short.wav'), out, again) == 6
    got = avi.read_avi(again)
    assert got['audio_rate'] == 8000 and np.array_equal(got['audio'], mono[:100]) and got['frames'] == frames

    _write_wav(tmp_path / 'bytes.wav', np.zeros(10, np.uint8), 8000, width=1)
    (tmp_path / 'junk.avi').write_bytes(b'RIFF\x04\x00\x00\x00WAVE')
    (tmp_path / 'junk.wav').write_bytes(b'not a wave file')
    for a, v, o in (('bytes.wav', 'silent.avi', 'o.avi'), ('speech.wav', 'junk.avi', 'o.avi'),
                    ('junk.wav', 'silent.avi', 'o.avi'), ('speech.mp3', 'silent.avi', 'o.avi'),
                    ('speech.wav', 'silent.mp4', 'o.avi'), ('speech.wav', 'silent.avi', 'o.mp4')):
        with pytest.raises(ValueError, match='supported'):
            avi.save_video_from_audio_video(str(tmp_path / a), str(tmp_path / v), str(tmp_path / o))
