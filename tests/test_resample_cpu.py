"""Host side of a2m.pats_audio.resample (no GPU): the output length, the plan builder's tap bank
against the float64 restatement in resample_ref.py, the restatement itself on pure tones (what a
band-limited resampler must do: pass the band, stop what would alias), and the argument errors."""
import ctypes

import numpy as np
import pytest

import resample_ref as ref

PAIRS = [(44100, 16000), (16000, 44100), (48000, 44100)]
BANKS = [(a, b, f) for a, b in PAIRS for f in ('kaiser_best', 'kaiser_fast')] + \
        [(45600, 16000, 'kaiser_best'), (16000, 8000, 'kaiser_best')]
_banks = {}


def _bank(sr_in, sr_out, res_type):
    from a2m import pats_audio
    key = (sr_in, sr_out, res_type)
    if key not in _banks:
        got = pats_audio.ResamplePlan(sr_in, sr_out, *pats_audio.RES_TYPES[res_type]).bank()
        want = ref.bank(sr_in, sr_out, res_type)
        want.setflags(write=False)
        _banks[key] = (got, want)
    return _banks[key]


def test_filter_parameters_are_the_published_ones():
    from a2m import pats_audio
    assert pats_audio.RES_TYPES == ref.FILTERS


def test_num_samples_sweep():
    from a2m import _native as N
    from a2m import pats_audio
    rates = [(441, 160), (160, 441), (44100, 16000), (16000, 44100), (48000, 44100), (16000, 16000),
             (45600, 16000), (16000, 8000), (22051, 16000), (1, 7), (7, 1)]
    for sr_in, sr_out in rates:
        for n in [0, 1, 2, 3, 159, 160, 161, 440, 441, 442, 3000, 12000, 190924, 2880000, 10 ** 12 + 7]:
            assert N.lib.a2m_resample_num_samples(n, sr_in, sr_out) == -(-n * sr_out // sr_in), (n, sr_in, sr_out)
    assert pats_audio.resample_num_samples(12000, 44100, 16000) == 4354
    for bad in [(-1, 441, 160), (5, 0, 160), (5, 441, 0), (5, -441, 160)]:
        assert N.lib.a2m_resample_num_samples(*bad) == 0


@pytest.mark.parametrize('sr_in,sr_out,res_type', BANKS)
def test_plan_bank_matches_restatement(sr_in, sr_out, res_type):
    (P, Q, L, got), want = _bank(sr_in, sr_out, res_type)
    assert (P, Q) == ref.ratio(sr_in, sr_out) and L == ref.half_width(sr_in, sr_out, ref.FILTERS[res_type][0])
    assert got.dtype == np.float32 and got.shape == want.shape == (Q, 2 * L)
    # float32 rounding of float64 values that may differ in their last bits (as the filterbank tests)
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-12)
    assert ((got != 0) == (want.astype(np.float32) != 0)).all()
    # the window's edge: a tap is zero exactly where |p - k Q| >= Z max(P, Q)
    num = np.arange(Q)[:, None] - np.arange(-L + 1, L + 1)[None, :] * Q
    outside = np.abs(num) >= ref.FILTERS[res_type][0] * max(P, Q)
    assert outside.any() and (got[outside] == 0).all()


def test_bank_sizes():
    """The banks DESIGN.md quotes: [Q][2L]."""
    for (a, b), shape in zip(PAIRS + [(45600, 16000)], [(160, 354), (441, 128), (147, 140), (20, 366)]):
        assert _bank(a, b, 'kaiser_best')[1].shape == shape


@pytest.mark.parametrize('sr_in,sr_out', PAIRS + [(45600, 16000), (16000, 8000)])
def test_every_phase_has_unit_dc_gain(sr_in, sr_out):
    (_, _, _, got), want = _bank(sr_in, sr_out, 'kaiser_best')
    assert np.abs(want.sum(1) - 1).max() < 1e-6
    assert np.abs(got.astype(np.float64).sum(1) - 1).max() < 1e-6


@pytest.mark.parametrize('sr_in,sr_out', [(44100, 16000), (16000, 44100)])
def test_restatement_reproduces_in_band_tones(sr_in, sr_out):
    n = sr_in // 4
    for hz in (1000.0, 0.40 * min(sr_in, sr_out)):
        y = ref.resample(ref.tone(n, sr_in, hz), sr_in, sr_out)
        assert y.size == ref.num_samples(n, sr_in, sr_out)
        want = ref.tone(y.size, sr_out, hz)
        e = np.abs(y - want)[600:-600].max()
        print(f'{sr_in} -> {sr_out}, {hz:.0f} Hz: interior error {e:.2e}')
        assert e < 1e-6


def test_restatement_stops_what_would_alias():
    sr_in, sr_out = 44100, 16000
    y = ref.resample(ref.tone(sr_in // 4, sr_in, 0.6 * sr_out), sr_in, sr_out)
    e = np.abs(y)[600:-600].max()
    print(f'0.6 sr_out tone: interior residue {e:.2e}')
    assert e < 1e-6


def test_restatement_float32_sums_stay_close():
    """The GPU tests' tolerance rests on this: the same sums in float32 differ from the float64
    ones by a few 1e-7 in rel_err."""
    from conftest import rel_err
    import pats_audio_ref
    x = pats_audio_ref.noisy_tone(3000, 44100)
    e = rel_err(ref.resample(x, 44100, 16000, dtype=np.float32), ref.resample(x, 44100, 16000))
    print(f'float32 restatement rel_err {e:.2e}')
    assert e < 1e-6


def test_bad_res_type():
    from a2m import pats_audio
    with pytest.raises(ValueError, match='res_type'):
        pats_audio.resample(np.zeros(100, np.float32), 44100, 16000, res_type='sinc_best')
    with pytest.raises(ValueError, match='res_type'):
        pats_audio.log_mel_400_resampled(np.zeros(100, np.float32), 44100, res_type='fft')


@pytest.mark.parametrize('rates', [(0, 16000), (44100, 0), (-44100, 16000), (44100, -1), (44100.5, 16000),
                                   (44100, '16000'), (2 ** 31, 16000)])
def test_bad_rates(rates):
    from a2m import pats_audio
    with pytest.raises(ValueError, match='sample rate'):
        pats_audio.resample(np.zeros(100, np.float32), *rates)


def test_bad_rates_at_the_abi():
    from a2m import _native as N
    buf = (ctypes.c_uint8 * 64)()
    for sr_in, sr_out in [(0, 16000), (16000, 0), (-1, 16000)]:
        assert N.lib.a2m_resample_plan_bytes(sr_in, sr_out, 64, 14.0, 0.9) == 0
        assert N.lib.a2m_resample_plan_build(sr_in, sr_out, 64, 14.0, 0.9, buf, 64) == N.A2M_EINVAL
        assert 'rates' in N.last_error()
    for z, beta, rho, word in [(0, 14.0, 0.9, 'num_zeros'), (64, -1.0, 0.9, 'beta'), (64, 14.0, 0.0, 'rolloff'),
                               (64, 14.0, 1.5, 'rolloff'), (64, float('nan'), 0.9, 'beta')]:
        assert N.lib.a2m_resample_plan_bytes(44100, 16000, z, beta, rho) == 0
        assert N.lib.a2m_resample_plan_build(44100, 16000, z, beta, rho, buf, 64) == N.A2M_EINVAL
        assert word in N.last_error()
    assert N.lib.a2m_resample_plan_bytes(44100, 16000, 64, 14.0, 1.0) > 0     # rolloff 1 is allowed
    nb = N.lib.a2m_resample_plan_bytes(16000, 8000, 16, 8.0, 0.85)
    assert N.lib.a2m_resample_plan_build(16000, 8000, 16, 8.0, 0.85, buf, 64) == N.A2M_EWS and nb > 64


def test_nearly_coprime_rates_are_refused():
    """22051 -> 16000 does not reduce: 16000 phases x 178 taps."""
    from a2m import _native as N
    from a2m import pats_audio
    with pytest.raises(ValueError, match='22051/16000'):
        pats_audio.ResamplePlan(22051, 16000, *pats_audio.RES_TYPES['kaiser_best'])
    with pytest.raises(ValueError, match='22051/16000'):
        pats_audio.resample(np.zeros(100, np.float32), 22051, 16000)
    assert N.lib.a2m_resample_plan_bytes(22051, 16000, *pats_audio.RES_TYPES['kaiser_best']) == 0


def test_launch_argument_errors():
    from a2m import _native as N
    one = ctypes.c_void_p(64)   # never dereferenced: every call below is refused on the host
    f = N.lib.a2m_resample_f32
    assert f(None, 1, 3000, 3000, 44100, 16000, 64, None, None, 1089, 1089, None) == N.A2M_EINVAL
    assert 'null' in N.last_error()
    for args in [(None, 1, 3000, 3000, 44100, 16000, 64, one, one, 1089, 1089, None),
                 (one, 1, 3000, 3000, 44100, 16000, 64, None, one, 1089, 1089, None),
                 (one, 1, 3000, 3000, 44100, 16000, 64, one, None, 1089, 1089, None)]:
        assert f(*args) == N.A2M_EINVAL and 'null' in N.last_error()
    assert f(one, -1, 3000, 3000, 44100, 16000, 64, one, one, 1089, 1089, None) == N.A2M_EINVAL
    assert f(one, 1, 3000, -3000, 44100, 16000, 64, one, one, 1089, 0, None) == N.A2M_EINVAL
    assert f(one, 1, 3000, 3000, 44100, 16000, 64, one, one, 1089, 1088, None) == N.A2M_EINVAL
    assert 'n_out' in N.last_error()
    assert f(one, 1, 3000, 3000, 0, 16000, 64, one, one, 1089, 1089, None) == N.A2M_EINVAL
    big = 2 ** 62 // 160 + 1                                                   # n_samples * Q > 2^62
    assert f(one, 1, big, big, 44100, 16000, 64, one, one, 1, 1, None) == N.A2M_EINVAL
    assert '62 bits' in N.last_error()
    # nothing to do is not an error, whatever the pointers
    assert f(None, 0, 3000, 3000, 44100, 16000, 64, None, None, 1089, 1089, None) == 0
    assert f(None, 1, 0, 0, 44100, 16000, 64, None, None, 0, 0, None) == 0


def test_plan_bank_rejects_a_truncated_plan():
    from a2m import _native as N
    from a2m import pats_audio
    plan = pats_audio.ResamplePlan(16000, 8000, *pats_audio.RES_TYPES['kaiser_fast'])
    hp = ctypes.c_void_p(plan.host.data_ptr())
    P = ctypes.c_int32()
    assert N.lib.a2m_resample_plan_bank(hp, 8, ctypes.byref(P), None, None, None) == N.A2M_EINVAL
    assert N.lib.a2m_resample_plan_bank(hp, plan.host.numel() - 4, ctypes.byref(P), None, None, None) == N.A2M_EINVAL
    assert N.lib.a2m_resample_plan_bank(hp, plan.host.numel(), ctypes.byref(P), None, None, None) == 0
    assert P.value == 2


def test_equal_rates_return_the_input():
    from a2m import pats_audio
    y = np.zeros(100, np.float32)
    assert pats_audio.resample(y, 16000, 16000) is y
    assert pats_audio.resample(y, 16000.0, 16000) is y


def test_generate_from_wave_takes_the_new_keywords_by_name():
    import inspect
    from a2m.inference import generate_from_wave
    sig = inspect.signature(generate_from_wave)
    names = list(sig.parameters)
    assert sig.parameters['resample_to'].default is None
    assert sig.parameters['res_type'].default == 'kaiser_best'
    assert names.index('resample_to') < names.index('res_type') < names.index('mel_kwargs')
