"""Streaming inference, the host side: the due rule of pats_audio.MelWindowStream against
inference.track_starts by brute force, the argument checks of the three stream entries of the
C-ABI, and AVIWriter.add_audio.  No GPU compute here."""
import ctypes

import numpy as np
import pytest

from conftest import REPO  # noqa: F401  (puts the package on sys.path)

HOP, N_FFT = 512, 2048
GEOMETRIES = [(0.49, 43, 1), (0.5, 44, 1), (0.52, 46, 1), (4.3, 382, 37)]   # time, window, stride over S


def _offline_starts(nf, overlap, time):
    from a2m.inference import track_starts
    try:
        return track_starts(nf, overlap, time, 15)[0]
    except ValueError:
        return np.zeros(0, np.int64)


@pytest.mark.parametrize('time,window,stride', GEOMETRIES)
def test_due_rule_against_track_starts(time, window, stride):
    from a2m.pats_audio import mel_window_geometry, mel_windows_due, num_frames
    w, interval, T = mel_window_geometry(time, 15)
    assert (w, interval) == (window, 6)
    rng = np.random.default_rng(3)
    appear_at_close = 0
    for overlap in (0, 1, T // 2):
        step = (T - overlap) * interval
        s_max = HOP * (window + 2 * step) + N_FFT          # three windows, and a little
        offline, last_nf = None, -1
        for S in range(1025, s_max + 1, stride):
            nf = num_frames(S, N_FFT, HOP, True)
            if nf != last_nf:
                offline, last_nf = _offline_starts(nf, overlap, time), nf
            d_open = mel_windows_due(S, False, window, interval, overlap)
            d_close = mel_windows_due(S, True, window, interval, overlap)
            # open: a prefix of the offline set; open + close: the offline set
            assert d_open <= d_close == len(offline), (S, overlap)
            assert np.array_equal(step * np.arange(d_close), offline)
            appear_at_close += d_close - d_open
            if d_open:
                # no due window needs a sample >= seen: its last frame ends at hop * id + n_fft / 2,
                # and frame 0's reflection reads up to sample n_fft / 2
                last = (d_open - 1) * step + interval * (T - 1)
                assert HOP * last + N_FFT // 2 - 1 < S and N_FFT // 2 < S, (S, overlap)
            # a split into two pushes emits nothing twice: the counts only grow
            a = int(rng.integers(0, S + 1))
            assert mel_windows_due(a, False, window, interval, overlap) <= d_open
    if window in (43, 44):
        assert appear_at_close > 0      # these geometries have windows that need end reflection
    else:
        assert appear_at_close == 0


def test_due_rule_last_sample_is_exact():
    """One sample short of the later of a window's two conditions it is not due; with it, it is.
    43 frames: the last frame's samples decide; 46 frames: the offline fit test does."""
    from a2m.pats_audio import mel_window_geometry, mel_windows_due
    for time in (0.49, 0.52):
        window, interval, T = mel_window_geometry(time, 15)
        need = max(HOP * interval * (T - 1) + N_FFT // 2, HOP * (window - 1))
        assert need == (22528 if time == 0.49 else 23040)
        assert mel_windows_due(need - 1, False, window, interval, 0) == 0
        assert mel_windows_due(need, False, window, interval, 0) == 1


# ------------------------------------------------------------------------------ C-ABI
PTR = 0x1000        # a non-null pointer for calls that must be refused before anything reads it


def _einval(rc):
    from a2m import _native as N
    assert rc == N.A2M_EINVAL, (rc, N.last_error())
    assert N.last_error()


def test_resample_stream_argument_checks():
    from a2m import _native as N
    f = N.lib.a2m_resample_stream_f32
    # (buf, base, len, n_total, sr_in, sr_out, zeros, plan, t_begin, n_out, out, stream)
    assert f(None, 0, 0, -1, 16000, 45600, 64, None, 0, 0, None, None) == 0          # zero size
    assert f(PTR, 0, 100, -1, 16000, 45600, 64, PTR, 7, 0, PTR, None) == 0
    _einval(f(None, 0, 4096, -1, 16000, 45600, 64, PTR, 0, 8, PTR, None))
    _einval(f(PTR, 0, 4096, -1, 16000, 45600, 64, None, 0, 8, PTR, None))
    _einval(f(PTR, 0, 4096, -1, 16000, 45600, 64, PTR, 0, 8, None, None))
    _einval(f(PTR, -1, 4096, -1, 16000, 45600, 64, PTR, 0, 8, PTR, None))
    _einval(f(PTR, 0, -1, -1, 16000, 45600, 64, PTR, 0, 8, PTR, None))
    _einval(f(PTR, 0, 4096, -1, 16000, 45600, 64, PTR, -1, 8, PTR, None))
    _einval(f(PTR, 0, 4096, -1, 16000, 45600, 64, PTR, 0, -8, PTR, None))
    _einval(f(PTR, 0, 4096, -1, 0, 45600, 64, PTR, 0, 8, PTR, None))
    # 16000 -> 45600: P/Q = 20/57, L = 64.  Output t reads samples [n_t - 63, n_t + 64].
    _einval(f(PTR, 0, 64, -1, 16000, 45600, 64, PTR, 0, 1, PTR, None))     # t = 0 needs sample 64
    assert 'buffer holds' in N.last_error()
    _einval(f(PTR, 64, 4096, -1, 16000, 45600, 64, PTR, 0, 1, PTR, None))  # sample 0 already dropped
    _einval(f(PTR, 0, 100, 200, 16000, 45600, 64, PTR, 285, 1, PTR, None))  # n_t = 100: needs 37..164, end at 200


def test_pats_audio_stream_argument_checks():
    from a2m import _native as N
    f = N.lib.a2m_pats_audio_stream_f32

    def call(buf=PTR, base=0, length=4096, n_total=-1, n_fft=2048, hop=512, win=2048, n_mels=128, power=2,
             plan=PTR, center=1, pad=0, eps=1e-10, ids=PTR, n_out=8, mean=None, std=None, out=PTR):
        return f(buf, base, length, n_total, n_fft, hop, win, n_mels, power, plan, center, pad, eps, ids, n_out,
                 mean, std, out, None)

    assert call(n_out=0) == 0
    assert call(buf=None, plan=None, ids=None, out=None, length=0, n_out=0) == 0
    for name in ('buf', 'plan', 'ids', 'out'):
        _einval(call(**{name: None}))
    _einval(call(base=-512))
    _einval(call(length=-1))
    _einval(call(n_out=-1))
    _einval(call(n_mels=0))
    _einval(call(mean=PTR))
    _einval(call(std=PTR))
    assert 'come together' in N.last_error()
    _einval(call(base=510))             # the frame loads are vector loads
    _einval(call(buf=PTR + 4))
    _einval(call(n_fft=2000))
    _einval(call(pad=2))
    _einval(call(eps=0.0))
    _einval(call(n_total=1024))         # reflection about an end needs more than n_fft / 2 samples


def test_track_blend_stream_argument_checks():
    from a2m import _native as N
    f = N.lib.a2m_track_blend_stream_f32
    # (win, m, T, Fd, overlap, tail, has_prev, flush, mean, std, out, stream)
    assert f(None, 0, 8, 104, 4, None, 0, 0, None, None, None, None) == 0
    assert f(None, 0, 8, 104, 4, PTR, 1, 0, None, None, None, None) == 0
    assert f(None, 0, 8, 104, 0, None, 1, 1, None, None, None, None) == 0    # a flush at overlap 0: nothing
    _einval(f(None, 1, 8, 104, 4, PTR, 0, 0, None, None, PTR, None))
    _einval(f(PTR, 1, 8, 104, 4, None, 0, 0, None, None, PTR, None))
    _einval(f(PTR, 1, 8, 104, 4, PTR, 0, 0, None, None, None, None))
    _einval(f(None, 0, 8, 104, 4, None, 1, 1, None, None, PTR, None))        # a flush reads the tail
    _einval(f(PTR, -1, 8, 104, 4, PTR, 0, 0, None, None, PTR, None))
    _einval(f(PTR, 1, 0, 104, 0, PTR, 0, 0, None, None, PTR, None))
    _einval(f(PTR, 1, 8, 0, 4, PTR, 0, 0, None, None, PTR, None))
    _einval(f(PTR, 1, 8, 104, -1, PTR, 0, 0, None, None, PTR, None))
    _einval(f(PTR, 1, 8, 104, 5, PTR, 0, 0, None, None, PTR, None))
    assert 'T/2' in N.last_error()
    _einval(f(PTR, 1, 8, 104, 4, PTR, 0, 0, PTR, None, PTR, None))
    _einval(f(PTR, 1, 8, 104, 4, PTR, 0, 0, None, PTR, PTR, None))
    _einval(f(None, 0, 8, 104, 4, PTR, 0, 1, None, None, PTR, None))         # a flush with no window before it


# ------------------------------------------------------------------------------ AVI
def _pcm(n):
    return (np.random.default_rng(11).integers(-30000, 30000, n)).astype('<i2')


def test_add_audio_in_pieces_equals_set_audio(tmp_path):
    from a2m.avi import AVIWriter, read_avi
    pcm = _pcm(9000)
    frames = [bytes([i]) * (40 + i) for i in range(7)]
    a, b = str(tmp_path / 'a.avi'), str(tmp_path / 'b.avi')
    with AVIWriter(a, 16, 8, audio_rate=16000) as w:
        w.set_audio(pcm)
        for fr in frames:
            w.write_frame(fr)
    with AVIWriter(b, 16, 8, audio_rate=16000) as w:
        w.add_audio(pcm[:2500])                     # ahead of frames 0, 1 (1067.7 samples a frame)
        w.write_frame(frames[0])
        w.write_frame(frames[1])
        w.add_audio(pcm[2500:2501])
        w.add_audio(pcm[2501:])
        for fr in frames[2:]:
            w.write_frame(fr)
    assert open(a, 'rb').read() == open(b, 'rb').read()
    back = read_avi(b)
    assert len(back['frames']) == 7 and np.array_equal(back['audio'], pcm[:len(back['audio'])])


def test_frame_ahead_of_its_samples_raises(tmp_path):
    from a2m.avi import AVIWriter
    pcm = _pcm(3000)
    with AVIWriter(str(tmp_path / 'c.avi'), 16, 8, audio_rate=16000) as w:
        w.add_audio(pcm[:1500])                     # frame 0 takes [0, 1067), frame 1 [1067, 2135)
        w.write_frame(b'x' * 10)
        with pytest.raises(ValueError, match='add_audio'):
            w.write_frame(b'y' * 10)
        assert w.frames == 1
        w.add_audio(pcm[1500:])
        w.write_frame(b'y' * 10)
        assert w.frames == 2 and w.samples == 2135
    with pytest.raises(ValueError):
        w.add_audio(pcm)                            # closed
    with pytest.raises(ValueError):
        AVIWriter(str(tmp_path / 'd.avi'), 16, 8).add_audio(pcm)   # no audio stream
