"""Streaming inference on the device: audio pushed in chunks gives the offline result bit for bit.

Every stage (pats_audio.ResampleStream, pats_audio.MelWindowStream, inference.TrackBlendStream,
inference.TrackStream, inference.VideoStream) is compared with its offline sibling over several
chunkings of one signal: one chunk, one sample at a time over the first 300 samples and then the
rest, a seeded random split, and boundaries at the indices where the code changes path.  Equal means
torch.equal / byte for byte; only the full generator is compared under the project's parity bound.
The waveform is pats_audio_ref.noisy_tone."""
import functools

import numpy as np
import pytest
import torch

import pats_audio_ref

pytestmark = pytest.mark.gpu

SR = 45600
# 512 * 40 + 137 samples are 41 feature frames: fewer than one window of any `time` below, so that
# length checks the empty stream.  512 * 139 + 137 is the shortest length of that form at which the
# last window (feature frame 96 = 2 * 48 = 4 * 24, both overlaps) of `time` 0.49 and 0.5 fits the
# recording (140 frames >= 96 + 44) while its last frame reaches past the end (sample
# 512 * (96 + 42) + 1024 > S): it appears only at close(), with end reflection.
S_SHORT, S_LONG = 512 * 40 + 137, 512 * 139 + 137


@functools.lru_cache(maxsize=None)
def tone(n, sr=SR):
    return pats_audio_ref.noisy_tone(n, sr)


def chunkings(S, critical, seed=0):
    """Lists of chunk lengths that sum to S."""
    rng = np.random.default_rng(seed)
    cuts = np.sort(rng.choice(np.arange(1, S), size=9, replace=False))
    crit = sorted({c for c in critical if 0 < c < S})
    out = {'one': [S],
           'samples': [1] * 300 + [S - 300],
           'random': np.diff(np.concatenate([[0], cuts, [S]])).tolist(),
           'critical': np.diff([0] + crit + [S]).tolist()}
    assert all(sum(v) == S and min(v) > 0 for v in out.values())
    return out


def pieces(wave, lengths, form):
    """The signal cut into chunks: form 0 device tensors, 1 numpy, 2 host tensors; and an empty push."""
    at = 0
    for i, n in enumerate(lengths):
        x = wave[at:at + n]
        at += n
        kind = (form + i) % 3
        yield torch.from_numpy(x).cuda() if kind == 0 else x if kind == 1 else torch.from_numpy(x)
        if i == 1:
            yield np.zeros(0, np.float32)


def run_stream(stream, wave, lengths, form=0):
    outs = [stream.push(x) for x in pieces(wave, lengths, form)]
    tail = stream.close()
    with pytest.raises(ValueError):
        stream.push(wave[:4])
    return outs, tail


# ------------------------------------------------------------------------------ resample
@pytest.mark.parametrize('rates', [(16000, 45600), (48000, 45600), (44100, 16000)])
def test_resample_stream_equals_resample(rates):
    from a2m import pats_audio as PA
    S = 5000
    wave = tone(S, rates[0])
    want = PA.resample(torch.from_numpy(wave).cuda(), rates[0], rates[1])
    L = PA.ResampleStream(rates[0], rates[1], max_chunk=1000).L
    for form, (name, lengths) in enumerate(chunkings(S, [2 * L - 1, 2 * L, 2 * L + 1]).items()):
        rs = PA.ResampleStream(rates[0], rates[1], max_chunk=1000)      # 5000 samples: the buffer compacts
        outs, tail = run_stream(rs, wave, lengths, form)
        seen = out = 0
        for x, n in zip(outs[:2], lengths[:2]):      # exactly the outputs whose taps arrived: n_t + L <= seen - 1
            seen, out = seen + n, out + x.numel()
            assert out == sum(1 for t in range(want.numel()) if t * rs.P // rs.Q + L <= seen - 1), name
        got = torch.cat(outs + [tail])
        assert got.shape == want.shape and torch.equal(got, want), name
        assert rs.samples_in == S and rs.samples_out == want.numel()


def test_resample_stream_equal_rates_pass_through():
    from a2m import pats_audio as PA
    wave = tone(3000)
    rs = PA.ResampleStream(SR, SR)
    outs, tail = run_stream(rs, wave, [1000, 1, 1999], form=1)
    assert tail.numel() == 0 and all(o.is_cuda for o in outs)
    assert torch.equal(torch.cat(outs), torch.from_numpy(wave).cuda())


# ------------------------------------------------------------------------------ mel windows
def _mel_reference(wave, time, overlap, mean, std, pad_mode):
    from a2m import inference as I, pats_audio as PA
    nf = PA.num_frames(len(wave), 2048, 512, True)
    try:
        starts, window, interval, T = I.track_starts(nf, overlap, time, 15)
    except ValueError:
        return None
    return PA.log_mel_512_windows(torch.from_numpy(wave).cuda(), SR, starts, window, interval, mean, std,
                                  pad_mode=pad_mode)


@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('half_overlap', [False, True])
@pytest.mark.parametrize('time', [0.49, 0.5, 0.52])
def test_mel_window_stream_equals_offline_windows(time, half_overlap, norm, pad_mode='reflect'):
    from a2m import pats_audio as PA
    window, interval, T = PA.mel_window_geometry(time, 15)
    overlap = T // 2 if half_overlap else 0
    rng = np.random.default_rng(2)
    mean = torch.from_numpy(rng.normal(-3, 1, 128).astype(np.float32)).cuda() if norm else None
    std = torch.from_numpy(rng.uniform(0.5, 3, 128).astype(np.float32)).cuda() if norm else None
    kw = dict(overlap=overlap, time=time, mean=mean, std=std, pad_mode=pad_mode, max_chunk=4096)
    # 41 feature frames hold no window: the stream gives none, the offline path refuses
    assert _mel_reference(tone(S_SHORT), time, overlap, mean, std, pad_mode) is None
    outs, tail = run_stream(PA.MelWindowStream(SR, **kw), tone(S_SHORT), [1024, 1, S_SHORT - 1025])
    assert all(o.shape == (0, T, 128) for o in outs + [tail])

    wave = tone(S_LONG)
    want = _mel_reference(wave, time, overlap, mean, std, pad_mode)
    assert want.shape[0] == {0.49: (3, 5), 0.5: (3, 5), 0.52: (2, 4)}[time][half_overlap]
    assert not torch.isnan(want).any()
    need = max(512 * interval * (T - 1) + 1024, 512 * (window - 1))      # window 0 comes due here
    assert need % 512 == 0
    for form, (name, lengths) in enumerate(chunkings(S_LONG, [1024, 1025, need - 1, need, need + 1]).items()):
        ms = PA.MelWindowStream(SR, **kw)
        outs, tail = run_stream(ms, wave, lengths, form)
        assert tail.shape[0] == (0 if time == 0.52 else 1), name          # 43 / 44 frames: end reflection
        if name == 'critical':   # pushes: 1024, 1, (empty), need - 1026, 1, 1, rest
            assert [o.shape[0] for o in outs[:6]] == [0, 0, 0, 0, 1, 0]
        got = torch.cat(outs + [tail])
        assert got.shape == want.shape and torch.equal(got, want), name
        assert ms.samples_in == S_LONG and ms.windows_out == want.shape[0]


def test_mel_window_stream_constant_padding():
    test_mel_window_stream_equals_offline_windows(0.5, True, True, pad_mode='constant')


# ------------------------------------------------------------------------------ blend
@pytest.mark.parametrize('norm', [False, True])
@pytest.mark.parametrize('Fd', [3, 104])
@pytest.mark.parametrize('overlap', [0, 1, 4])
def test_track_blend_stream_equals_blend_track(overlap, Fd, norm):
    from a2m import inference as I
    T = 8
    rng = np.random.default_rng(overlap * 7 + Fd)
    mean = torch.from_numpy(rng.normal(0, 50, Fd).astype(np.float32)).cuda() if norm else None
    std = torch.from_numpy(rng.uniform(0.5, 30, Fd).astype(np.float32)).cuda() if norm else None
    for n in (1, 2, 5):
        win = torch.from_numpy(rng.standard_normal((n, T, Fd)).astype(np.float32)).cuda()
        want = I.blend_track(win, overlap, mean, std)
        for at_a_time in (1, 2, n):
            bs = I.TrackBlendStream(T, Fd, overlap, mean, std)
            outs = [bs.push(win[:0])]
            outs += [bs.push(win[i:i + at_a_time]) for i in range(0, n, at_a_time)]
            assert [o.shape[0] for o in outs[1:]] == [min(at_a_time, n - i) * (T - overlap)
                                                     for i in range(0, n, at_a_time)]
            outs.append(bs.close())
            assert outs[-1].shape == (overlap, Fd)
            got = torch.cat(outs)
            assert got.shape == want.shape and torch.equal(got, want), (n, at_a_time)
            with pytest.raises(ValueError):
                bs.push(win[:1])
    with pytest.raises(ValueError):
        I.TrackBlendStream(T, Fd, overlap, mean, std).close()               # nothing to flush
    with pytest.raises(ValueError):
        I.TrackBlendStream(T, Fd, T // 2 + 1)


# ------------------------------------------------------------------------------ track
class Stub:
    """A generator that is a pure elementwise function of its window."""
    body_feats, hand_feats = 20, 84

    def __call__(self, audio):
        return audio[..., :104] * 0.5, None


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('resample_from', [None, 16000])
def test_track_stream_with_a_stub_generator(resample_from, batch):
    from a2m import inference as I
    sr = resample_from or SR
    S = S_LONG if resample_from is None else 25000          # 25000 at 16 kHz: 71250 samples, 140 frames
    wave = tone(S, sr)
    rng = np.random.default_rng(4)
    mean = torch.from_numpy(rng.normal(0, 50, 104).astype(np.float32)).cuda()
    std = torch.from_numpy(rng.uniform(0.5, 30, 104).astype(np.float32)).cuda()
    kw = dict(overlap=3, batch=batch, time=0.5, pose_mean=mean, pose_std=std,
              resample_to=None if resample_from is None else SR)
    want = I.generate_track(Stub(), torch.from_numpy(wave).cuda(), sr, **kw)
    n_win = (140 - 44) // (5 * 6) + 1
    assert want.shape == ((n_win - 1) * 5 + 8, 104)
    for form, (name, lengths) in enumerate(chunkings(S, [1024, 1025, 22527, 22528, 22529], seed=1).items()):
        ts = I.TrackStream(Stub(), sr, max_chunk=4096, **kw)
        outs, tail = run_stream(ts, wave, lengths, form)
        got = torch.cat(outs + [tail])
        assert got.shape == want.shape and torch.equal(got, want), name
        assert (ts.samples_in, ts.windows_out, ts.frames_out) == (S, n_win, want.shape[0]), name


def test_track_stream_too_short_raises_at_close():
    from a2m import inference as I
    wave = tone(S_SHORT)
    with pytest.raises(ValueError, match='one window needs 44'):
        I.generate_track(Stub(), torch.from_numpy(wave).cuda(), SR, overlap=3, time=0.5)
    ts = I.TrackStream(Stub(), SR, overlap=3, time=0.5)
    assert ts.push(wave).shape == (0, 104)
    with pytest.raises(ValueError, match='one window needs 44'):
        ts.close()


def test_track_stream_with_the_generator(g_state):
    """Default geometry, three windows at overlap 16, batch 1 on both sides: the same shapes through
    the same routes, so the normalised poses are expected to be equal; the bound is the project's
    parity bound, there so that an unordered reduction in the eval forward would not fail a
    streaming test.  Observed on an MI355X: max abs difference 0.0 (recorded in DESIGN.md)."""
    from a2m import inference as I
    from a2m.real_motion_model import SelfAttention_G
    g = SelfAttention_G(p=0.0)
    g.load_state_dict(g_state, strict=False)
    g = g.to('cuda').eval()
    S = 512 * 958
    wave = tone(S)
    want = I.generate_track(g, torch.from_numpy(wave).cuda(), SR, overlap=16, batch=1)
    assert want.shape == (2 * 48 + 64, 104)
    ts = I.TrackStream(g, SR, overlap=16, batch=1)
    lengths = [16384] * (S // 16384) + [S % 16384]
    outs, tail = run_stream(ts, wave, lengths, form=1)
    got = torch.cat(outs + [tail])
    assert got.shape == want.shape
    diff = (got - want).abs().max().item()
    print(f'track stream vs generate_track: max abs difference {diff:.3e}')
    assert diff < 1e-4
    assert (ts.samples_in, ts.windows_out, ts.frames_out) == (S, 3, 160)


# ------------------------------------------------------------------------------ video
def test_video_stream_writes_the_offline_file(tmp_path):
    from a2m import inference as I
    from a2m.avi import read_avi

    class Drawn(Stub):          # still elementwise; moves the mel values onto the canvas
        def __call__(self, audio):
            return audio[..., :104] * 4.0 + 40.0, None

    wave = tone(S_LONG)
    a, b = str(tmp_path / 'offline.avi'), str(tmp_path / 'stream.avi')
    kw = dict(overlap=3, track_kwargs=dict(time=0.5), img_size=(96, 64), scale=1.0, quality=80, chunk=7)
    frames = I.generate_video(Drawn(), torch.from_numpy(wave).cuda(), SR, a, **kw)
    vs = I.VideoStream(Drawn(), SR, b, **kw)
    for x in pieces(wave, chunkings(S_LONG, [22527, 22528, 22529])['random'], 0):
        vs.push(x)
    assert vs.close() == frames == 3 * 5 + 8
    assert open(a, 'rb').read() == open(b, 'rb').read()
    ra, rb = read_avi(a), read_avi(b)
    assert len(rb['frames']) == len(ra['frames']) == frames
    assert np.array_equal(ra['audio'], rb['audio']) and len(rb['audio']) == frames * SR * 2002 // 30000


# ------------------------------------------------------------------------------ allocation
def test_no_device_allocation_after_warm_up():
    from a2m import inference as I, pats_audio as PA
    wave = torch.from_numpy(tone(4096 * 10)).cuda()
    for make in (lambda: PA.MelWindowStream(SR, overlap=3, time=0.5, max_chunk=4096),
                 lambda: PA.ResampleStream(SR, 16000, max_chunk=4096),
                 lambda: I.TrackStream(Stub(), SR, overlap=3, time=0.5, max_chunk=4096)):
        stream, seen, got = make(), {}, 0
        for i in range(10):
            out = stream.push(wave[4096 * i:4096 * (i + 1)])
            got += out.shape[0]
            del out
            seen[i + 1] = torch.cuda.memory_allocated()
        assert got > 0                       # windows / samples did come out in between
        assert seen[10] == seen[3], seen
