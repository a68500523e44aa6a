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
  ResampleStream(orig_sr, target_sr, ...) / MelWindowStream(sr, overlap, time, ...)
      resample and log_mel_512_windows (over inference.track_starts) for a signal that arrives in
      pieces: push(samples), close(); the pieces concatenate to the offline result bit for bit.

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


# ------------------------------------------------------------------------------ streaming
# The stateful forms of resample and log_mel_512_windows for audio that arrives in pieces
# (Streaming inference).  Each stage keeps a linear sliding device buffer that holds
# samples [base, base + len) of the signal, allocated once: capacity 2 * (largest live span) +
# max_chunk, so that when a chunk no longer fits, the live samples move to the front in one
# non-overlapping device copy.  What a push returns follows from sample counts on the host; nothing
# is read back from the device.
def _as_chunk(samples, device):
    """[s] samples (device tensor, host tensor or numpy) -> a float32 tensor; host data stays on
    the host (the copy into the buffer is the transfer)."""
    if torch.is_tensor(samples):
        x = samples.detach()
        if x.is_cuda and x.device != device:
            raise ValueError(f'samples are on {x.device}, the stream on {device}')
    else:
        x = torch.as_tensor(np.asarray(samples, dtype=np.float32))
    if x.dim() != 1:
        raise ValueError(f'a chunk is [s] samples of one channel, got {tuple(x.shape)}')
    return x if x.dtype == torch.float32 else x.float()


class _SlidingBuffer:
    """Samples [base, base + len) of an unbounded signal in one device allocation."""

    def __init__(self, live_max, max_chunk, device, align=1):
        if max_chunk < 1:
            raise ValueError('max_chunk must be >= 1')
        self.live_max, self.max_chunk, self.align = int(live_max), int(max_chunk), int(align)
        # `align` more: the kept span starts at a multiple of it, at most align - 1 below the need
        self.cap = 2 * (self.live_max + self.align) + self.max_chunk
        self.buf = torch.zeros(self.cap, device=device, dtype=torch.float32)
        self.base, self.len = 0, 0

    @property
    def seen(self):
        return self.base + self.len

    def append(self, chunk, keep_from):
        """Add chunk (<= max_chunk samples); samples below keep_from are no longer needed."""
        s = chunk.shape[0]
        assert s <= self.max_chunk
        if self.len + s > self.cap:
            lo = max(self.base, keep_from // self.align * self.align)
            live = self.seen - lo
            a = lo - self.base
            assert live <= a and live + s <= self.cap, (live, a, s, self.cap)   # sized so by construction
            if live:
                self.buf[:live].copy_(self.buf[a:a + live])
            self.base, self.len = lo, live
        if s:
            self.buf[self.len:self.len + s].copy_(chunk, non_blocking=True)
        self.len += s


class ResampleStream:
    """resample() for a signal that arrives in pieces: the concatenation of every push() and of
    close() equals resample(whole signal) bit for bit, whatever the chunking.

    push(samples [s]) -> [r] (device): exactly the outputs whose whole tap support has arrived
    (n_t + L <= seen - 1); close() -> [r]: the rest, up to ceil(S * target_sr / orig_sr), with zeros
    past the end.  Equal rates pass the samples through.  A push larger than max_chunk is split
    internally; after close(), push raises."""

    def __init__(self, orig_sr, target_sr, res_type='kaiser_best', max_chunk=16384, device='cuda'):
        self.cfg = _resample_cfg(orig_sr, target_sr, res_type)
        self.device = torch.device(device if str(device) != 'cuda' else f'cuda:{torch.cuda.current_device()}')
        self.samples_in, self.samples_out, self.closed = 0, 0, False
        self.passthrough = self.cfg[0] == self.cfg[1]
        self.max_chunk = int(max_chunk)
        if self.max_chunk < 1:
            raise ValueError('max_chunk must be >= 1')
        if self.passthrough:
            return
        self.plan = ResamplePlan.get(self.device, *self.cfg)
        self.P, self.Q, self.L, _ = self.plan.bank()
        # after a push every ready output is out, so the next one's support [n_t - L + 1, n_t + L]
        # is not complete: fewer than 2 L samples are live
        self.sb = _SlidingBuffer(2 * self.L + 1, self.max_chunk, self.device)

    def ready(self, seen, closed=False):
        """Outputs [0, ready) are computable from `seen` samples (host arithmetic only)."""
        if closed:
            return resample_num_samples(seen, self.cfg[0], self.cfg[1])
        x = seen - 1 - self.L          # n_t = t P div Q <= x
        return 0 if x < 0 else ((x + 1) * self.Q - 1) // self.P + 1

    def _keep_from(self):
        return max(0, self.samples_out * self.P // self.Q - self.L + 1)

    def _launch(self, out, t_begin, n_out, n_total):
        sb = self.sb
        N.check(N.lib.a2m_resample_stream_f32(F._p(sb.buf), sb.base, sb.len, n_total, self.cfg[0], self.cfg[1],
                                              self.cfg[2], F._p(self.plan.dev), t_begin, n_out, F._p(out),
                                              F._stream()), value_error=True)

    def push(self, samples):
        if self.closed:
            raise ValueError('the stream is closed')
        x = _as_chunk(samples, self.device)
        if self.passthrough:
            self.samples_in += x.shape[0]
            self.samples_out += x.shape[0]
            return x.to(self.device)
        total = self.ready(self.samples_in + x.shape[0]) - self.samples_out
        out = torch.empty(total, device=self.device, dtype=torch.float32)
        done = 0
        with torch.cuda.device(self.device):
            for i in range(0, x.shape[0], self.max_chunk):
                chunk = x[i:i + self.max_chunk]
                self.sb.append(chunk, self._keep_from())
                self.samples_in += chunk.shape[0]
                n = self.ready(self.samples_in) - self.samples_out
                self._launch(out[done:done + n], self.samples_out, n, -1)
                self.samples_out += n
                done += n
        return out

    def close(self):
        if self.closed:
            raise ValueError('the stream is closed')
        self.closed = True
        if self.passthrough:
            return torch.empty(0, device=self.device, dtype=torch.float32)
        n = self.ready(self.samples_in, True) - self.samples_out
        out = torch.empty(n, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._launch(out, self.samples_out, n, self.samples_in)
        self.samples_out += n
        return out


def mel_window_geometry(time=4.3, fs_new=15):
    """(window, interval, T) of the audio/log_mel_512 windows, as inference.track_starts."""
    from .windowing import window_index
    _, window, interval = window_index(0, 'audio/log_mel_512', fs_new, time)
    return window, interval, (window + interval - 1) // interval


def mel_windows_due(seen, closed, window, interval, overlap, n_fft=2048, hop=512):
    """How many windows [0, due) of a stream are computable once `seen` samples have arrived: the
    pure host rule of MelWindowStream.  Window k starts at feature frame s_k = k (T - overlap)
    interval and reads frames s_k + interval j, j < T.  While the stream is open it is due when
    the frames seen so far hold it, num_frames(seen) >= s_k + window (the offline fit test, so no
    window is emitted that the whole recording would not have), and its last frame is complete,
    seen >= hop (s_k + interval (T - 1)) + n_fft / 2.  At close every window that fits the final
    length is due; the frames that then reach past the end are reflected about it."""
    T = (window + interval - 1) // interval
    step = (T - overlap) * interval
    nf = num_frames(seen, n_fft, hop, True) if seen > 0 else 0
    fit = (nf - window) // step + 1 if nf >= window else 0
    if closed:
        return fit
    room = seen - n_fft // 2 - hop * interval * (T - 1)
    return min(fit, room // (hop * step) + 1) if room >= 0 else 0


class MelWindowStream:
    """log_mel_512_windows over inference.track_starts for a signal that arrives in pieces: the
    concatenation of every push() and of close() equals
    log_mel_512_windows(whole, sr, track_starts(num_frames(S), overlap, time, fs_new)[0], ...) bit
    for bit, whatever the chunking.

    push(samples [s]) -> [m, T, n_mels] (device), the windows that became due (mel_windows_due);
    close() -> [m, T, n_mels], the windows that fit only the final length, with end reflection.
    Mel rows shared by overlapping windows are recomputed.  After close(), push raises."""
    N_FFT, HOP = 2048, 512

    def __init__(self, sr, overlap=16, time=4.3, fs_new=15, mean=None, std=None, eps=1e-10,
                 pad_mode='reflect', n_mels=128, max_chunk=16384, device='cuda'):
        self.device = torch.device(device if str(device) != 'cuda' else f'cuda:{torch.cuda.current_device()}')
        self.window, self.interval, self.T = mel_window_geometry(time, fs_new)
        if not 0 <= overlap <= self.T // 2:
            raise ValueError(f'overlap {overlap} outside [0, T/2 = {self.T // 2}]')
        if pad_mode not in PAD_MODES:
            raise ValueError(f"pad_mode must be 'reflect' or 'constant', got {pad_mode!r}")
        if (mean is None) != (std is None):
            raise ValueError('mean and std come together')
        self.overlap, self.eps, self.pad_mode, self.pad = int(overlap), float(eps), pad_mode, PAD_MODES[pad_mode]
        self.step = (self.T - self.overlap) * self.interval
        self.plan = PatsAudioPlan.get(self.device, *_cfg_512(sr, n_mels))
        self.mean = None if mean is None else mean.to(self.device, torch.float32).contiguous()
        self.std = None if std is None else std.to(self.device, torch.float32).contiguous()
        self.max_chunk = int(max_chunk)
        hop, half = self.HOP, self.N_FFT // 2
        # the next window is not yet due: fewer samples than the later of its two conditions asks
        # for are live, counted from its first sample hop s_k - n_fft / 2
        live = max(hop * self.interval * (self.T - 1) + 2 * half, hop * self.window + half) + hop
        # the buffer is only ever compacted by multiples of the hop: the kernel's frame loads are
        # vector loads from base-relative offsets (a2m_pats_audio_stream_f32)
        self.sb = _SlidingBuffer(live, self.max_chunk, self.device, align=hop)
        self.per_call = self.max_chunk // (hop * self.step) + 3      # windows one chunk can make due
        k = torch.arange(self.per_call, device=self.device, dtype=torch.int64)
        j = torch.arange(self.T, device=self.device, dtype=torch.int64)
        self._rel = (k[:, None] * self.step + j[None, :] * self.interval).contiguous()
        self._ids = torch.empty_like(self._rel)
        self.samples_in, self.windows_out, self.closed = 0, 0, False

    def due(self, seen, closed=False):
        return mel_windows_due(seen, closed, self.window, self.interval, self.overlap, self.N_FFT, self.HOP)

    def _keep_from(self):
        return max(0, self.HOP * self.windows_out * self.step - self.N_FFT // 2)

    def _emit(self, out, n, n_total):
        """Windows [windows_out, windows_out + n) into out [n, T, n_mels]."""
        sb, p = self.sb, self.plan
        for i in range(0, n, self.per_call):
            m = min(self.per_call, n - i)
            torch.add(self._rel[:m], (self.windows_out + i) * self.step, out=self._ids[:m])
            N.check(N.lib.a2m_pats_audio_stream_f32(F._p(sb.buf), sb.base, sb.len, n_total, p.n_fft, p.hop,
                                                    p.win_length, p.n_mels, p.power, F._p(p.dev), 1, self.pad,
                                                    self.eps, F._p(self._ids), m * self.T, F._p(self.mean),
                                                    F._p(self.std), F._p(out[i:i + m]), F._stream()),
                    value_error=True)
        self.windows_out += n

    def push(self, samples):
        if self.closed:
            raise ValueError('the stream is closed')
        x = _as_chunk(samples, self.device)
        total = self.due(self.samples_in + x.shape[0]) - self.windows_out
        out = torch.empty(total, self.T, self.plan.n_mels, device=self.device, dtype=torch.float32)
        done = 0
        with torch.cuda.device(self.device):
            for i in range(0, x.shape[0], self.max_chunk):
                chunk = x[i:i + self.max_chunk]
                self.sb.append(chunk, self._keep_from())
                self.samples_in += chunk.shape[0]
                n = self.due(self.samples_in) - self.windows_out
                self._emit(out[done:done + n], n, -1)
                done += n
        return out

    def close(self):
        if self.closed:
            raise ValueError('the stream is closed')
        self.closed = True
        n = self.due(self.samples_in, True) - self.windows_out
        out = torch.empty(n, self.T, self.plan.n_mels, device=self.device, dtype=torch.float32)
        if n:
            _pad_mode(self.pad_mode, self.samples_in, self.N_FFT)
            with torch.cuda.device(self.device):
                self._emit(out, n, self.samples_in)
        return out
