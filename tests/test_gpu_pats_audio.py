"""a2m.pats_audio on the GPU against the float64 restatement (pats_audio_ref.py): log_mel_512
over the edge cases of its centred framing, log_mel_400, the windowed entry that computes only
the frames a window gather reads, and waveform -> poses end to end.

The waveform is noise over a 440 Hz tone: every band of both features holds energy far above
fp32 FFT noise, the values span about -5 .. 8, and a float32 CPU restatement differs from the
float64 one by 5.5e-7 in rel_err, so the suite's TOL = 1e-4 applies unchanged."""
import numpy as np
import pytest
import torch

import pats_audio_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda'
_cache = {}


def _wave(n, sr=16000):
    if (n, sr) not in _cache:
        _cache[n, sr] = ref.noisy_tone(n, sr)
    return _cache[n, sr].copy()


def _ref512(n, sr=16000, **kw):
    key = ('512', n, sr) + tuple(sorted(kw.items()))
    if key not in _cache:
        r = ref.log_mel_512(_wave(n, sr), sr, **kw)
        r.setflags(write=False)
        _cache[key] = r
    return _cache[key]


def _check(got, want):
    got = got.cpu().numpy() if torch.is_tensor(got) else got
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.isfinite(got).all()
    e = rel_err(got, want)
    print(f'rel_err {e:.3e} over {want.shape}, ref range [{want.min():.2f}, {want.max():.2f}]')
    assert e < TOL


# ------------------------------------------------------------------------------ log_mel_512
@pytest.mark.parametrize('n,frames', [(1025, 3), (1500, 3), (3587, 8), (30000, 59)])
def test_log_mel_512_lengths(n, frames):
    """Minimum length, every frame touching a pad, S no multiple of the hop, a frame count that
    is no multiple of the 8 waves of a workgroup."""
    from a2m.pats_audio import log_mel_512
    got = log_mel_512(torch.from_numpy(_wave(n)).to(DEV), 16000)
    assert got.shape == (frames, 128)
    _check(got, _ref512(n))


@pytest.mark.parametrize('n', [1025, 3587])
@pytest.mark.parametrize('sr', [22050, 44100])
def test_log_mel_512_sample_rates(sr, n):
    """Other filterbanks: the rows get wider with the sample rate (64 taps at 44.1 kHz)."""
    from a2m.pats_audio import log_mel_512
    _check(log_mel_512(torch.from_numpy(_wave(n, sr)).to(DEV), sr), _ref512(n, sr))


def test_log_mel_512_80_mels():
    from a2m.pats_audio import log_mel_512
    got = log_mel_512(torch.from_numpy(_wave(3587)).to(DEV), 16000, n_mels=80)
    assert got.shape == (8, 80)
    _check(got, _ref512(3587, n_mels=80))


@pytest.mark.parametrize('n', [1500, 3587])
def test_log_mel_512_constant_padding(n):
    from a2m.pats_audio import log_mel_512
    _check(log_mel_512(torch.from_numpy(_wave(n)).to(DEV), 16000, pad_mode='constant'),
           _ref512(n, pad_mode='constant'))
    short = log_mel_512(torch.from_numpy(_wave(1025)[:700].copy()).to(DEV), 16000, pad_mode='constant')
    _check(short, ref.log_mel_512(_wave(1025)[:700], 16000, pad_mode='constant'))


def test_log_mel_512_numpy_in_numpy_out():
    from a2m.pats_audio import log_mel_512
    got = log_mel_512(_wave(3587), 16000)
    assert isinstance(got, np.ndarray)
    _check(got, _ref512(3587))


def test_log_mel_512_strided_rows():
    """[3, S] rows that are a slice of a wider buffer; every clip has its own edges."""
    from a2m.pats_audio import log_mel_512
    n = 3587
    full = _wave(3 * 4000 + 100)
    buf = torch.from_numpy(full[:3 * 4000].reshape(3, 4000).copy()).to(DEV)
    view = buf[:, 100:100 + n]
    assert not view.is_contiguous()
    got = log_mel_512(view, 16000)
    assert got.shape == (3, 8, 128)
    want = np.stack([ref.log_mel_512(full[c * 4000 + 100:c * 4000 + 100 + n], 16000) for c in range(3)])
    _check(got, want)


def test_silence_hits_the_zero_mask():
    """All-zero audio: every value is exactly the float32 nearest to log(float32(eps)), for
    both features."""
    from a2m.pats_audio import log_mel_400, log_mel_512
    z = torch.zeros(3587, device=DEV)
    a = log_mel_512(z, 16000).cpu().numpy()
    b = log_mel_400(z).cpu().numpy()
    want_a = np.log(np.float64(np.float32(1e-10))).astype(np.float32)
    want_b = np.log(np.float64(np.float32(1e-6))).astype(np.float32)
    assert a.shape == (8, 128) and (a == want_a).all()
    assert b.shape == (20, 64) and (b == want_b).all()
    # a different eps moves it: the value is the mask's, not a floor under the spectrum
    c = log_mel_512(z, 16000, eps=1e-3).cpu().numpy()
    assert (c == np.log(np.float64(np.float32(1e-3))).astype(np.float32)).all()


# ------------------------------------------------------------------------------ log_mel_400
@pytest.mark.parametrize('n,frames', [(512, 1), (1000, 4), (1637, 8), (30000, 185)])
def test_log_mel_400(n, frames):
    from a2m.pats_audio import log_mel_400
    got = log_mel_400(torch.from_numpy(_wave(n)).to(DEV))
    assert got.shape == (frames, 64)
    _check(got, ref.log_mel_400(_wave(n)))


def test_log_mel_400_too_short_is_empty():
    from a2m.pats_audio import log_mel_400
    got = log_mel_400(torch.from_numpy(_wave(512)[:511].copy()).to(DEV))
    assert got.shape == (0, 64)
    assert log_mel_400(_wave(512)[:511]).shape == (0, 64)


# ---------------------------------------------------------------------- log_mel_512_windows
def test_windows_equal_gather_of_full_feature():
    from a2m.pats_audio import log_mel_512, log_mel_512_windows
    from a2m.windowing import gather_windows
    wave = torch.from_numpy(_wave(30000)).to(DEV)
    full = log_mel_512(wave, 16000)                       # 59 frames
    starts = np.array([40, 0, 47, 13, 0, 13], np.int64)   # unsorted, repeated, first and last window
    got = log_mel_512_windows(wave, 16000, starts, window=12, interval=5)
    want = gather_windows(full, starts, 12, 5)
    assert got.shape == want.shape == (6, 3, 128)
    assert torch.equal(got, want)
    _check(got[1], _ref512(30000)[0:12:5])
    mean = torch.linspace(-1, 1, 128, device=DEV)
    std = torch.linspace(0.5, 2, 128, device=DEV)
    std[5] = 0.0                                          # the loader's std < 1e-7 -> 1
    assert torch.equal(log_mel_512_windows(wave, 16000, starts, 12, 5, mean, std),
                       gather_windows(full, starts, 12, 5, mean, std))


def test_windows_loader_geometry_two_windows():
    """window 382, interval 6 (the generator's T = 64) on a clip long enough for two."""
    from a2m.pats_audio import log_mel_512, log_mel_512_windows
    from a2m.windowing import gather_windows, window_index
    n = 512 * 770
    wave = torch.from_numpy(_wave(n)).to(DEV)
    full = log_mel_512(wave, 16000)
    starts, window, interval = window_index(full.shape[0], 'audio/log_mel_512', 15)
    assert (window, interval) == (382, 6) and len(starts) == 2
    got = log_mel_512_windows(wave, 16000, starts)
    assert got.shape == (2, 64, 128)
    assert torch.equal(got, gather_windows(full, starts, window, interval))


def test_windows_per_window_clips():
    from a2m.pats_audio import log_mel_512, log_mel_512_windows
    waves = torch.from_numpy(np.stack([_wave(30000), _wave(30000)[::-1].copy()])).to(DEV)
    full = log_mel_512(waves, 16000)
    got = log_mel_512_windows(waves, 16000, [3, 40, 3], 12, 5, clips=[1, 0, 1])
    for i, (s, c) in enumerate(((3, 1), (40, 0), (3, 1))):
        assert torch.equal(got[i], full[c, s:s + 12:5])


def test_windows_out_of_range_raises():
    from a2m.pats_audio import log_mel_512_windows
    wave = torch.from_numpy(_wave(30000)).to(DEV)
    for starts in ([48], [-1], torch.tensor([0, 48], device=DEV)):
        with pytest.raises(ValueError, match='window out of range'):
            log_mel_512_windows(wave, 16000, starts, window=12, interval=5)


def test_windows_capture_into_a_graph():
    from a2m.pats_audio import log_mel_512_windows
    wave = torch.from_numpy(_wave(30000)).to(DEV)
    starts = torch.tensor([40, 0, 13], device=DEV)
    eager = log_mel_512_windows(wave, 16000, starts, 12, 5)       # also builds the plan
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        log_mel_512_windows(wave, 16000, starts, 12, 5, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


# ------------------------------------------------------------------------------ end to end
def test_wave_to_poses_end_to_end(g_state):
    """generate_from_wave == the restatement's features, windowed on the host, through the
    generator (as test_mel_plus_generator_end_to_end, at its 1e-4)."""
    from a2m.inference import generate, generate_from_wave
    from a2m.real_motion_model import SelfAttention_G
    from a2m.windowing import window_index
    m = SelfAttention_G(p=0.0)
    m.load_state_dict(g_state, strict=False)
    m = m.to(DEV).eval()
    n = 512 * 770
    feat = _ref512(n)
    starts, window, interval = window_index(feat.shape[0], 'audio/log_mel_512', 15)
    mean, std = feat.mean(0).astype(np.float32), feat.std(0).astype(np.float32)
    windows = np.stack([feat[s:s + window:interval] for s in starts])
    audio = ((windows - mean) / std).astype(np.float32)
    pm = torch.linspace(-50, 50, 104)
    ps = torch.linspace(1, 20, 104)
    want = generate(m, torch.from_numpy(audio).to(DEV), pm, ps)
    got = generate_from_wave(m, torch.from_numpy(_wave(n)).to(DEV), 16000,
                             audio_mean=torch.from_numpy(mean).to(DEV),
                             audio_std=torch.from_numpy(std).to(DEV), pose_mean=pm, pose_std=ps)
    assert got.shape == (2, 64, 104)
    e = rel_err(got.cpu(), want.cpu())
    print(f'pose rel_err {e:.3e}')
    assert e < TOL
