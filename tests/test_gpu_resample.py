"""a2m.pats_audio.resample on the GPU against the float64 restatement (resample_ref.py): rate
pairs and both filters, the clip edges, input / output forms, a captured launch, and the two
entries built on it (log_mel_400_resampled, generate_from_wave(resample_to=...)).

The waveform is pats_audio_ref.noisy_tone.  A float32 restatement of the same sums differs from
the float64 one by 1.5e-7 .. 2.7e-7 in rel_err (test_resample_cpu.py prints it), so the suite's
TOL = 1e-4 applies unchanged."""
import numpy as np
import pytest
import torch

import pats_audio_ref
import resample_ref as ref
from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda'
_cache = {}


def _wave(n, sr):
    if (n, sr) not in _cache:
        _cache[n, sr] = pats_audio_ref.noisy_tone(n, sr)
    return _cache[n, sr].copy()


def _ref(n, sr_in, sr_out, res_type='kaiser_best'):
    key = ('ref', n, sr_in, sr_out, res_type)
    if key not in _cache:
        r = ref.resample(_wave(n, sr_in), sr_in, sr_out, res_type)
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


@pytest.mark.parametrize('sr_in,sr_out,n,res_type', [
    (44100, 16000, 3000, 'kaiser_best'), (44100, 16000, 3000, 'kaiser_fast'),
    (16000, 44100, 1200, 'kaiser_best'), (16000, 44100, 1200, 'kaiser_fast'),
    (48000, 44100, 2500, 'kaiser_best'), (45600, 16000, 3000, 'kaiser_best'),
    (16000, 8000, 1500, 'kaiser_best')])
def test_pairs_and_filters(sr_in, sr_out, n, res_type):
    from a2m.pats_audio import resample
    got = resample(torch.from_numpy(_wave(n, sr_in)).to(DEV), sr_in, sr_out, res_type)
    assert got.shape == (ref.num_samples(n, sr_in, sr_out),)
    _check(got, _ref(n, sr_in, sr_out, res_type))


@pytest.mark.parametrize('n,n_out', [(1, 1), (50, 19), (353, 129), (12000, 4354)])
def test_edges(n, n_out):
    """One sample; every output seeing both zero extensions; one sample short of the filter's
    width; more than one workgroup tile and no multiple of it."""
    from a2m.pats_audio import resample
    got = resample(torch.from_numpy(_wave(n, 44100)).to(DEV), 44100, 16000)
    assert got.shape == (n_out,)
    _check(got, _ref(n, 44100, 16000))


@pytest.mark.parametrize('sr_in,sr_out,n,res_type', [(48000, 4000, 30000, 'kaiser_best'),
                                                     (48000, 100, 20000, 'kaiser_fast')])
def test_steep_ratios(sr_in, sr_out, n, res_type):
    """12:1 fills most of the LDS a tile may take (13.8k samples); at 480:1 the span of a tile
    does not fit, and the launch takes the unstaged kernel."""
    from a2m.pats_audio import resample
    got = resample(torch.from_numpy(_wave(n, sr_in)).to(DEV), sr_in, sr_out, res_type)
    _check(got, _ref(n, sr_in, sr_out, res_type))


def test_strided_rows():
    """[3, S] rows that are a slice of a wider buffer; every clip has its own edges."""
    from a2m.pats_audio import resample
    n = 3000
    full = _wave(3 * 4000 + 100, 44100)
    buf = torch.from_numpy(full[:3 * 4000].reshape(3, 4000).copy()).to(DEV)
    view = buf[:, 100:100 + n]
    assert not view.is_contiguous()
    got = resample(view, 44100, 16000)
    assert got.shape == (3, 1089)
    want = np.stack([ref.resample(full[c * 4000 + 100:c * 4000 + 100 + n], 44100, 16000) for c in range(3)])
    _check(got, want)


def test_numpy_in_numpy_out():
    from a2m.pats_audio import resample
    got = resample(_wave(3000, 44100), 44100, 16000)
    assert isinstance(got, np.ndarray)
    _check(got, _ref(3000, 44100, 16000))


def test_out_is_honoured():
    from a2m.pats_audio import resample
    wave = torch.from_numpy(_wave(3000, 44100)).to(DEV)
    out = torch.full((1089,), float('nan'), device=DEV)
    got = resample(wave, 44100, 16000, out=out)
    assert got.data_ptr() == out.data_ptr()
    _check(out, _ref(3000, 44100, 16000))


def test_equal_rates_return_the_input():
    from a2m.pats_audio import resample
    wave = torch.from_numpy(_wave(3000, 44100)).to(DEV)
    assert resample(wave, 44100, 44100) is wave


def test_silence_gives_exact_zeros():
    from a2m.pats_audio import resample
    got = resample(torch.zeros(2, 3000, device=DEV), 44100, 16000)
    assert got.shape == (2, 1089) and (got == 0).all()


def test_empty_input_gives_empty_output():
    from a2m.pats_audio import resample
    assert resample(torch.zeros(0, device=DEV), 44100, 16000).shape == (0,)
    assert resample(torch.zeros(3, 0, device=DEV), 44100, 16000).shape == (3, 0)
    assert resample(np.zeros(0, np.float32), 44100, 16000).shape == (0,)


def test_capture_into_a_graph():
    from a2m.pats_audio import resample
    wave = torch.from_numpy(_wave(12000, 44100)).to(DEV)
    eager = resample(wave, 44100, 16000)                  # also builds the plan
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        resample(wave, 44100, 16000, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_log_mel_400_resampled():
    from a2m.pats_audio import log_mel_400_resampled
    n = 12000                                             # 4354 samples at 16 kHz: 25 frames
    got = log_mel_400_resampled(torch.from_numpy(_wave(n, 44100)).to(DEV), 44100)
    assert got.shape == (25, 64)
    _check(got, pats_audio_ref.log_mel_400(_ref(n, 44100, 16000)))


def test_generate_from_wave_resamples_first(g_state):
    """resample_to=R == resampling by hand and passing sr=R, bitwise; without the keyword the
    call is today's: the features of the wave as it is, through log_mel_512_windows."""
    from a2m.inference import generate, generate_from_wave
    from a2m.pats_audio import log_mel_512_windows, num_frames, resample
    from a2m.real_motion_model import SelfAttention_G
    from a2m.windowing import window_index
    m = SelfAttention_G(p=0.0)
    m.load_state_dict(g_state, strict=False)
    m = m.to(DEV).eval()
    sr, R = 16000, 45600
    n = 70000                                             # 199500 samples at R: 390 frames, one window
    wave = torch.from_numpy(_wave(n, sr)).to(DEV)
    pm, ps = torch.linspace(-50, 50, 104), torch.linspace(1, 20, 104)
    got = generate_from_wave(m, wave, sr, pose_mean=pm, pose_std=ps, resample_to=R)
    by_hand = resample(wave, sr, R)
    assert by_hand.shape == (199500,)
    want = generate_from_wave(m, by_hand, R, pose_mean=pm, pose_std=ps)
    assert got.shape == (1, 64, 104) and torch.equal(got, want)
    # resample_to=None: the parent's body, spelled out
    long = torch.from_numpy(_wave(512 * 400, sr)).to(DEV)
    starts, window, interval = window_index(num_frames(long.shape[-1], 2048, 512, True), 'audio/log_mel_512', 15, 4.3)
    parent = generate(m, log_mel_512_windows(long, sr, starts, window, interval, None, None), pm, ps)
    assert torch.equal(generate_from_wave(m, long, sr, pose_mean=pm, pose_std=ps), parent)
    assert torch.equal(generate_from_wave(m, long, sr, pose_mean=pm, pose_std=ps, resample_to=None), parent)
