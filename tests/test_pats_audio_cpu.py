"""Host side of a2m.pats_audio (no GPU): the plan builder's Slaney filterbank against the
float64 restatement in pats_audio_ref.py, the restatement itself against librosa's published
filters.mel example, the frame counts and the argument errors."""
import ctypes

import numpy as np
import pytest

import pats_audio_ref as ref


def test_restatement_matches_librosa_published_example():
    """librosa's docs print filters.mel(sr=22050, n_fft=2048) row 0 as 0, 0.016, 0.032, ...;
    by hand w[0, 1] = (10.767 / 25.79) * 2 / 51.59 = 0.0162."""
    w = ref.slaney_mel_basis(22050, 2048)
    assert w.shape == (128, 1025)
    np.testing.assert_allclose(w[0, :3], [0.0, 0.016, 0.032], atol=5e-4)
    assert abs(w[0, 1] - 0.0162) < 5e-4
    assert w[-1, -1] == 0.0 and (w >= 0).all()


@pytest.mark.parametrize('sr,n_mels', [(16000, 128), (22050, 128), (44100, 128), (16000, 80)])
def test_plan_filterbank_512(sr, n_mels):
    from a2m import pats_audio
    got = pats_audio.mel_basis_512(sr, n_mels)
    want = ref.slaney_mel_basis(sr, 2048, n_mels)
    assert got.dtype == np.float32 and got.shape == want.shape
    # float32 rounding of float64 values that may differ in their last bits
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-12)
    assert ((got != 0) == (want.astype(np.float32) != 0)).all()


def test_plan_filterbank_400():
    from a2m import pats_audio
    got = pats_audio.mel_basis_400()
    want = ref.slaney_mel_basis(16000, 512, 64, 125.0, 7500.0, norm=False)
    assert got.shape == (64, 257)
    np.testing.assert_allclose(got, want, rtol=2e-7, atol=1e-12)
    assert got.max() <= 1.0   # norm=None: plain triangles


@pytest.mark.parametrize('n,frames', [(1025, 3), (3587, 8), (30000, 59)])
def test_frame_count_centred(n, frames):
    from a2m import pats_audio
    assert pats_audio.num_frames(n, 2048, 512, True) == frames == 1 + n // 512


@pytest.mark.parametrize('n,frames', [(511, 0), (512, 1), (1637, 8)])
def test_frame_count_400(n, frames):
    from a2m import pats_audio
    assert pats_audio.num_frames(n, 512, 160, False) == frames


@pytest.mark.parametrize('n', [1, 1000, 1024])
def test_reflect_needs_more_than_half_a_frame(n):
    from a2m import pats_audio
    with pytest.raises(ValueError, match='reflect'):
        pats_audio.log_mel_512(np.zeros(n, np.float32), 16000)


def test_reflect_rejected_by_the_launch_too():
    from a2m import _native as N
    rc = N.lib.a2m_pats_audio_f32(None, 1, 1024, 1024, 2048, 512, 2048, 128, 2, None, 1, 0, 1e-10,
                                  None, 3, None, None, None, None)
    assert rc == N.A2M_EINVAL and 'reflect' in N.last_error()


def test_bad_pad_mode():
    from a2m import pats_audio
    with pytest.raises(ValueError, match='pad_mode'):
        pats_audio.log_mel_512(np.zeros(4096, np.float32), 16000, pad_mode='edge')


def test_fmax_above_nyquist():
    from a2m import pats_audio
    with pytest.raises(ValueError, match='Nyquist'):
        pats_audio.PatsAudioPlan(16000, 2048, 512, 2048, 128, 0.0, 8000.5, 1, 2)
    from a2m import _native as N
    assert N.lib.a2m_pats_audio_plan_bytes(16000, 2048, 512, 2048, 128, 0.0, 8000.5, 1, 2) == 0


def test_log_mel_400_does_not_resample():
    from a2m import pats_audio
    with pytest.raises(ValueError, match='resampl'):
        pats_audio.log_mel_400(np.zeros(4096, np.float32), sr=44100)


def test_plan_rejects_bad_geometry():
    from a2m import pats_audio
    for cfg in ((16000, 1000, 160, 400, 64, 125.0, 7500.0, 0, 1),    # n_fft not a power of two
                (16000, 512, 160, 600, 64, 125.0, 7500.0, 0, 1),     # window longer than the frame
                (16000, 512, 160, 400, 64, 125.0, 7500.0, 0, 3)):    # power
        with pytest.raises(ValueError):
            pats_audio.PatsAudioPlan(*cfg)
    plan = pats_audio.PatsAudioPlan(16000, 512, 160, 400, 64, 125.0, 7500.0, 0, 1)
    basis = np.zeros((64, 257), np.float32)
    from a2m import _native as N
    assert N.lib.a2m_pats_audio_plan_filterbank(ctypes.c_void_p(plan.host.data_ptr()), 8,
                                                basis.ctypes.data) == N.A2M_EINVAL
