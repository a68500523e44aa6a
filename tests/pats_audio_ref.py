"""Float64 numpy restatement of the PATS audio features (pats/data_loading/audio.py:58-120),
i.e. of librosa.feature.melspectrogram with the defaults the reference was written against,
from the published formulas only (librosa itself is not a dependency):

  slaney_mel_basis(sr, n_fft, n_mels, fmin, fmax, norm)   librosa.filters.mel(htk=False)
  log_mel_512(y, sr, eps, pad_mode, n_mels)               centred, reflected edges, power, 128 mels
  log_mel_400(y, eps)                                     16 kHz, 400-in-512 window, magnitude, 64 mels

Shared by the CPU and GPU tests of a2m.pats_audio; the tests treat its outputs as read-only.
"""
import numpy as np

_F_SP = 200.0 / 3
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP           # 15
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    return np.where(f >= _MIN_LOG_HZ,
                    _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def slaney_mel_basis(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, norm=True):
    """[n_mels, 1 + n_fft/2] float64 triangles linear in Hz; norm: each row times 2 / bandwidth."""
    fmax = sr / 2.0 if fmax is None else fmax
    fftfreqs = np.linspace(0.0, sr / 2.0, 1 + n_fft // 2)
    mel_f = mel_to_hz(np.linspace(hz_to_mel(fmin), hz_to_mel(fmax), n_mels + 2))
    w = np.zeros((n_mels, fftfreqs.size))
    for i in range(n_mels):
        lower = (fftfreqs - mel_f[i]) / (mel_f[i + 1] - mel_f[i])
        upper = (mel_f[i + 2] - fftfreqs) / (mel_f[i + 2] - mel_f[i + 1])
        w[i] = np.maximum(0.0, np.minimum(lower, upper))
        if norm:
            w[i] *= 2.0 / (mel_f[i + 2] - mel_f[i])
    return w


def _hann(n):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)


def _frames(y, n_fft, hop):
    n = 1 + (y.size - n_fft) // hop if y.size >= n_fft else 0
    idx = hop * np.arange(n)[:, None] + np.arange(n_fft)[None, :]
    return y[idx] if n else np.zeros((0, n_fft))


def _mask_log(spec, eps):
    return np.log(np.where(spec == 0, eps, spec))


def log_mel_512(y, sr, eps=1e-10, pad_mode='reflect', n_mels=128):
    y = np.asarray(y, dtype=np.float64)
    n_fft, hop = 2048, 512
    if pad_mode == 'reflect' and y.size <= n_fft // 2:
        raise ValueError('reflect padding needs more than n_fft / 2 samples')
    yp = np.pad(y, n_fft // 2, mode=pad_mode)
    spec = np.abs(np.fft.rfft(_frames(yp, n_fft, hop) * _hann(n_fft), axis=1)) ** 2
    return _mask_log(spec @ slaney_mel_basis(sr, n_fft, n_mels).astype(np.float32).astype(np.float64).T, eps)


def log_mel_400(y, eps=1e-6):
    y = np.asarray(y, dtype=np.float64)
    sr, n_fft, hop, win = 16000, 512, 160, 400
    window = np.zeros(n_fft)
    window[(n_fft - win) // 2:(n_fft - win) // 2 + win] = _hann(win)
    spec = np.abs(np.fft.rfft(_frames(y, n_fft, hop) * window, axis=1))
    basis = slaney_mel_basis(sr, n_fft, 64, 125.0, 7500.0, norm=False)
    return _mask_log(spec @ basis.astype(np.float32).astype(np.float64).T, eps)


def noisy_tone(n_samples, sr):
    """The tests' waveform: noise over a 440 Hz tone (every band far above fp32 FFT noise)."""
    t = np.arange(n_samples) / float(sr)
    return (0.1 * np.random.default_rng(7).standard_normal(n_samples)
            + 0.5 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
