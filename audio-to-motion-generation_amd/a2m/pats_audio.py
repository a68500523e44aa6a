"""PATS audio features from a waveform on the HIP path (pats/data_loading/audio.py:58-120).

  log_mel_512(y, sr, eps=1e-10, pad_mode='reflect', n_mels=128, out=None)
      librosa.feature.melspectrogram(y, sr, n_fft=2048, hop_length=512): frames centred with
      reflected edges ('constant' = zeros, newer librosa's default), periodic Hann, power
      spectrum, Slaney filterbank 0..sr/2 with area normalisation, exact zeros -> eps, ln,
      [frames, n_mels] with frames = 1 + S // 512.  The generator's audio/log_mel_512 input.
  log_mel_400(y, sr=16000, eps=1e-6, out=None)
      n_fft 512, hop 160, a 400-sample Hann centred in the frame, no padding, magnitude
      spectrum, 64 Slaney mels 125..7500 Hz without normalisation; frames = 1 + (S - 512) // 160.
      Works on 16 kHz audio only: any other sr raises ValueError (log_mel_400_resampled is the
      entry that resamples first, as the reference does).
  resample(y, orig_sr, target_sr, res_type='kaiser_best', out=None)
      librosa.core.resample as the reference calls it (audio.py:88): band-limited interpolation
      with a Kaiser-windowed sinc, resampy's 'kaiser_best' (64 zero crossings) or 'kaiser_fast'
      (16) parameters, the continuous filter evaluated exactly; ceil(S * target_sr / orig_sr)
      samples.  Equal rates return y itself.
  log_mel_400_resampled(y, sr, eps=1e-6, res_type='kaiser_best')
      == log_mel_400(resample(y, sr, 16000)): the reference's audio/log_mel_400 (audio.py:86-120).
  log_mel_512_windows(wave, sr, starts, window=382, interval=6, mean=None, std=None, ...)
      == gather_windows(log_mel_512(wave, sr), starts, window, interval, mean, std), computing
      only the frames the gather reads (every `interval`-th of each window).

`y` may be a 1-D numpy array (returns numpy [F, M], as the reference does) or a device tensor
[S] / [C, S] with contiguous samples (rows may be strided; returns [F, M] / [C, F, M]).
Computation and output are fp32 on the GPU (reference: float64 numpy); DESIGN.md section 4, PATS
audio features, has the semantics and the numbers.  There is no CPU path.  resample takes and
returns the same forms ([S] numpy -> numpy; [S] / [C, S] device -> [S'] / [C, S']).
"""
import ctypes

import numpy as np
import torch

from . import _native as N
from . import functional as F

PAD_MODES = {'reflect': 0, 'constant': 1}


class PatsAudioPlan:
    """Device-resident window / twiddle / Slaney-filterbank plan of one feature configuration."""
    _cache = {}

    def __init__(self, sample_rate, n_fft, hop, win_length, n_mels, fmin, fmax, slaney_norm, power,
                 device=None):
        self.n_fft, self.hop, self.win_length, self.n_mels, self.power = n_fft, hop, win_length, n_mels, power
        args = (sample_rate, n_fft, hop, win_length, n_mels, fmin, fmax, int(slaney_norm), power)
        nbytes = N.lib.a2m_pats_audio_plan_bytes(*args)
        self.host = torch.zeros(max(nbytes, 16), dtype=torch.uint8)
        N.check(N.lib.a2m_pats_audio_plan_build(*args, ctypes.c_void_p(self.host.data_ptr()),
                                                self.host.numel()), value_error=True)
        self.dev = self.host.to(device) if device is not None else None

    @classmethod
    def get(cls, device, *cfg):
        key = cfg + (str(torch.device(device)),)
        if key not in cls._cache:
            cls._cache[key] = cls(*cfg, device=device)
        return cls._cache[key]

    def filterbank(self):
        """The plan's mel basis as numpy [n_mels, 1 + n_fft/2] float32 (librosa.filters.mel)."""
        basis = np.zeros((self.n_mels, self.n_fft // 2 + 1), np.float32)
        N.check(N.lib.a2m_pats_audio_plan_filterbank(ctypes.c_void_p(self.host.data_ptr()),
                                                     self.host.numel(), basis.ctypes.data))
        return basis


def _cfg_512(sr, n_mels):
    return (int(sr), 2048, 512, 2048, int(n_mels), 0.0, sr / 2.0, 1, 2)


def _cfg_400(sr):
    if int(sr) != 16000:
        raise ValueError(f'log_mel_400 works on 16 kHz audio: resampling from sr={sr} is not '
                         'implemented, resample the waveform first')
    return (16000, 512, 160, 400, 64, 125.0, 7500.0, 0, 1)


def mel_basis_512(sr, n_mels=128):
    return PatsAudioPlan(*_cfg_512(sr, n_mels)).filterbank()


def mel_basis_400(sr=16000):
    return PatsAudioPlan(*_cfg_400(sr)).filterbank()


def num_frames(n_samples, n_fft, hop, center):
    return int(N.lib.a2m_pats_audio_num_frames(n_samples, n_fft, hop, int(center)))


def _pad_mode(pad_mode, n_samples, n_fft):
    if pad_mode not in PAD_MODES:
        raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
    if pad_mode == 'reflect' and n_samples <= n_fft // 2:
        raise ValueError(f'reflect padding needs more than n_fft / 2 = {n_fft // 2} samples, '
                         f'got {n_samples}')
    return PAD_MODES[pad_mode]


def _launch(wave, plan, center, pad, eps, frame_ids, n_out, mean, std, out):
    C, S = wave.shape
    N.check(N.lib.a2m_pats_audio_f32(F._p(wave), C, wave.stride(0), S, plan.n_fft, plan.hop,
                                     plan.win_length, plan.n_mels, plan.power, F._p(plan.dev),
                                     int(center), pad, float(eps), F._p(frame_ids), n_out, F._p(mean),
                                     F._p(std), F._p(out), F._stream()), value_error=True)
    return out


def _feature(y, cfg, center, pad_mode, eps, out):
    as_numpy = not torch.is_tensor(y)
    if as_numpy:
        y = torch.as_tensor(np.asarray(y, dtype=np.float32))
    if y.dim() not in (1, 2):
        raise ValueError(f'waveform must be [S] or [C, S], got {tuple(y.shape)}')
    pad = _pad_mode(pad_mode, y.shape[-1], cfg[1]) if center else 0   # before anything touches the GPU
    wave = y.to('cuda') if as_numpy else y
    F._check_dev(wave, out)
    squeeze = wave.dim() == 1
    w2 = wave.reshape(1, -1) if squeeze else wave
    if w2.stride(1) != 1 and w2.shape[1] > 1:
        w2 = w2.contiguous()
    plan = PatsAudioPlan.get(w2.device, *cfg)
    C, S = w2.shape
    nf = num_frames(S, plan.n_fft, plan.hop, center)
    if out is None:
        out = torch.empty(C, nf, plan.n_mels, device=w2.device, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.numel() == C * nf * plan.n_mels
    _launch(w2, plan, center, pad, eps, None, C * nf, None, None, out)
    res = out.reshape(nf, plan.n_mels) if squeeze else out.reshape(C, nf, plan.n_mels)
    return res.cpu().numpy() if as_numpy else res


def log_mel_512(y, sr, eps=1e-10, pad_mode='reflect', n_mels=128, out=None):
    return _feature(y, _cfg_512(sr, n_mels), True, pad_mode, eps, out)


def log_mel_400(y, sr=16000, eps=1e-6, out=None):
    return _feature(y, _cfg_400(sr), False, 'constant', eps, out)


# ------------------------------------------------------------------------------ resampling
# res_type -> (zero crossings, Kaiser beta, roll-off): resampy's published filter designs
RES_TYPES = {'kaiser_best': (64, 14.769656459379492, 0.9475937167399596),
             'kaiser_fast': (16, 8.555504641634386, 0.85)}


class ResamplePlan:
    """Device-resident tap bank of one (orig_sr, target_sr, filter) configuration."""
    _cache = {}

    def __init__(self, sr_in, sr_out, num_zeros, beta, rolloff, device=None):
        self.sr_in, self.sr_out, self.num_zeros = sr_in, sr_out, num_zeros
        args = (sr_in, sr_out, num_zeros, beta, rolloff)
        nbytes = N.lib.a2m_resample_plan_bytes(*args)
        self.host = torch.zeros(max(nbytes, 64), dtype=torch.uint8)
        N.check(N.lib.a2m_resample_plan_build(*args, ctypes.c_void_p(self.host.data_ptr()),
                                              self.host.numel()), value_error=True)
        self.dev = self.host.to(device) if device is not None else None

    @classmethod
    def get(cls, device, *cfg):
        key = cfg + (str(torch.device(device)),)
        if key not in cls._cache:
            cls._cache[key] = cls(*cfg, device=device)
        return cls._cache[key]

    def bank(self):
        """(P, Q, L, taps): the reduced ratio, the half width and the dense float32 bank [Q, 2L],
        row p holding h_p[k] for k = -L+1 .. L."""
        P, Q, L = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        hp, nb = ctypes.c_void_p(self.host.data_ptr()), self.host.numel()
        N.check(N.lib.a2m_resample_plan_bank(hp, nb, ctypes.byref(P), ctypes.byref(Q), ctypes.byref(L), None))
        taps = np.zeros((Q.value, 2 * L.value), np.float32)
        N.check(N.lib.a2m_resample_plan_bank(hp, nb, None, None, None, taps.ctypes.data))
        return P.value, Q.value, L.value, taps


def _rate(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != int(v) \
            or not 1 <= int(v) < 2 ** 31:
        raise ValueError(f'{name} must be a positive integer sample rate, got {v!r}')
    return int(v)


def _resample_cfg(orig_sr, target_sr, res_type):
    if res_type not in RES_TYPES:
        raise ValueError(f'res_type must be one of {sorted(RES_TYPES)}, got {res_type!r}')
    return (_rate('orig_sr', orig_sr), _rate('target_sr', target_sr)) + RES_TYPES[res_type]


def resample_num_samples(n_samples, orig_sr, target_sr):
    return int(N.lib.a2m_resample_num_samples(n_samples, orig_sr, target_sr))


def resample(y, orig_sr, target_sr, res_type='kaiser_best', out=None):
    cfg = _resample_cfg(orig_sr, target_sr, res_type)
    if cfg[0] == cfg[1]:
        return y
    as_numpy = not torch.is_tensor(y)
    if as_numpy:
        y = torch.as_tensor(np.asarray(y, dtype=np.float32))
    if y.dim() not in (1, 2):
        raise ValueError(f'waveform must be [S] or [C, S], got {tuple(y.shape)}')
    if N.lib.a2m_resample_plan_bytes(*cfg) == 0:
        ResamplePlan(*cfg)   # a refused configuration raises before anything touches the GPU
    wave = y.to('cuda') if as_numpy else y
    F._check_dev(wave, out)
    squeeze = wave.dim() == 1
    w2 = wave.reshape(1, -1) if squeeze else wave
    if w2.stride(1) != 1 and w2.shape[1] > 1:
        w2 = w2.contiguous()
    plan = ResamplePlan.get(w2.device, *cfg)
    C, S = w2.shape
    n_out = resample_num_samples(S, cfg[0], cfg[1])
    if out is None:
        out = torch.empty(C, n_out, device=w2.device, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.numel() == C * n_out
    N.check(N.lib.a2m_resample_f32(F._p(w2), C, w2.stride(0), S, cfg[0], cfg[1], cfg[2], F._p(plan.dev),
                                   F._p(out), n_out, n_out, F._stream()), value_error=True)
    res = out.reshape(n_out) if squeeze else out.reshape(C, n_out)
    return res.cpu().numpy() if as_numpy else res


def log_mel_400_resampled(y, sr, eps=1e-6, res_type='kaiser_best'):
    return log_mel_400(resample(y, sr, 16000, res_type), 16000, eps)


_offsets = {}


def _frame_offsets(nj, interval, device):
    key = (nj, interval, str(device))
    if key not in _offsets:
        _offsets[key] = interval * torch.arange(nj, device=device, dtype=torch.int64)
    return _offsets[key]


def log_mel_512_windows(wave, sr, starts, window=382, interval=6, mean=None, std=None, eps=1e-10,
                        pad_mode='reflect', n_mels=128, clips=None, out=None):
    """wave [S] or [C, S] (device), starts: feature-frame index of each window's first frame ->
    [n, ceil(window / interval), n_mels].  With [C, S], clips[i] is window i's clip (default 0).
    Host `starts` are range-checked on the host; device `starts` are checked too unless the
    stream is capturing (the check reads them back): the range is then the caller's to keep, and
    a frame outside the wave gives a row of NaN, never an out-of-bounds read."""
    F._check_dev(wave, mean, std, out)
    w2 = wave.reshape(1, -1) if wave.dim() == 1 else wave
    if w2.dim() != 2:
        raise ValueError(f'waveform must be [S] or [C, S], got {tuple(wave.shape)}')
    if w2.stride(1) != 1 and w2.shape[1] > 1:
        w2 = w2.contiguous()
    dev = w2.device
    plan = PatsAudioPlan.get(dev, *_cfg_512(sr, n_mels))
    C, S = w2.shape
    pad = _pad_mode(pad_mode, S, plan.n_fft)
    nf = num_frames(S, plan.n_fft, plan.hop, True)
    capturing = torch.cuda.is_current_stream_capturing()
    if torch.is_tensor(starts) and starts.is_cuda:
        st = starts.to(dev, torch.int64).reshape(-1)
        lo_hi = None if capturing or not st.numel() else (int(st.min()), int(st.max()))
    else:
        st_h = np.asarray(starts.cpu() if torch.is_tensor(starts) else starts, np.int64).reshape(-1)
        lo_hi = (int(st_h.min()), int(st_h.max())) if st_h.size else None
        st = torch.from_numpy(st_h).to(dev)
    if lo_hi is not None and (lo_hi[0] < 0 or lo_hi[1] + window > nf):
        raise ValueError('window out of range')
    nj = (window + interval - 1) // interval
    if clips is not None:
        cl = clips.to(dev, torch.int64) if torch.is_tensor(clips) else \
            torch.from_numpy(np.asarray(clips, np.int64)).to(dev)
        if not capturing and cl.numel() and (int(cl.min()) < 0 or int(cl.max()) >= C):
            raise ValueError('clip index out of range')
        st = st + nf * cl.reshape(-1)
    ids = (st[:, None] + _frame_offsets(nj, interval, dev)[None, :]).contiguous()   # one small kernel
    n = st.numel()
    if out is None:
        out = torch.empty(n, nj, plan.n_mels, device=dev, dtype=torch.float32)
    else:
        assert out.is_contiguous() and out.numel() == n * nj * plan.n_mels
    if mean is not None:
        mean, std = mean.contiguous(), std.contiguous()
    _launch(w2, plan, True, pad, eps, ids, n * nj, mean, std, out)
    return out
