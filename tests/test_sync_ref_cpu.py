"""tests/sync_ref.py (the float64 restatement of the synchrony metrics) against a planted
signal and against brute force, the host formulas of a2m.evaluation against both, and the condition the
GPU test's random inputs must meet.  No GPU."""
import numpy as np
import pytest

import sync_ref as S


def _mid(shape):
    return 'x'.join(str(s) for s in shape)


@pytest.mark.parametrize('late', [0, 2])
def test_planted_signal(late):
    """Onsets every 8 frames from frame 6, a speed dip exactly on each (late = 0) or 2 frames after: every
    distance is `late`, in both directions; with late = 0 beat_align = beat_recall = 1; the most negative
    correlation sits at lag `late`."""
    from a2m.evaluation import SYNC_METRICS, _sync_metrics
    audio, pose, on = S.planted(late)
    ref = S.sync_sums(audio, pose, pose, np.array([0, 1], np.int32), 2)
    fa, fr, ff = ref['flags']
    assert len(on) == 7 and np.array_equal(np.flatnonzero(fa[0]), on)
    assert np.array_equal(np.flatnonzero(fr[0]), on + late) and np.array_equal(fr, ff)
    want = np.zeros((2, 2, 2, 32), np.int64)
    want[..., late] = len(on)
    assert np.array_equal(ref['beat_dist'], want)
    assert np.array_equal(ref['beat_counts'], np.full((2, 3), len(on)))
    for m in (S.metrics(ref['beat_dist'][0], ref['beat_counts'][0], ref['lag_sums'][0], ref['lag_n'][0]),
              _sync_metrics(ref['beat_dist'][0], ref['beat_counts'][0], ref['lag_sums'][0], ref['lag_n'][0], 1.0)):
        assert sorted(m) == sorted(SYNC_METRICS)
        for key in ('beat_align_real', 'beat_align_fake', 'beat_recall_real', 'beat_recall_fake'):
            assert m[key] == pytest.approx(np.exp(-late ** 2 / 2.0), rel=1e-15)
            if late == 0:
                assert m[key] == 1.0
        r = np.array(m['sync_corr_real'])
        assert len(r) == 9 and not np.isnan(r).any()
        assert int(np.argmin(r)) - 4 == late and r.min() < -0.9
        assert m['sync_corr_fake'] == m['sync_corr_real']
        assert m['beat_far_share'] == 0.0 and m['n_audio_beats'] == len(on)
        assert m['sync_lag_real'] == int(np.argmax(r)) - 4


def test_against_brute_force():
    """The histograms against a loop over the beats, the lag sums' Pearson r against np.corrcoef on the
    pairs themselves, and a2m.evaluation's host formulas against sync_ref's."""
    from a2m.evaluation import _sync_metrics, beat_alignment, pearson_from_sums
    case = S.random_case((5, 64, 128, 52))
    B, T, n_lags, n_dist = 5, 64, 4, 3
    style = np.zeros(B, np.int32)
    ref = S.sync_sums(case['audio'], case['fake'], case['real'], style, 1, n_lags, n_dist, audio_std=case['std'])
    o, (fa, fr, ff) = ref['onset'], ref['flags']
    assert fa.sum() > 5 and fr.sum() > 5 and ff.sum() > 5
    hist = np.zeros((2, 2, n_dist), np.int64)
    for b in range(B):
        for w, fm in enumerate((fr, ff)):
            for src, dst, k in ((fm[b], fa[b], 0), (fa[b], fm[b], 1)):
                for t in np.flatnonzero(src):
                    near = [abs(t - u) for u in np.flatnonzero(dst)]
                    hist[w, k, min(min(near), n_dist - 1) if near else n_dist - 1] += 1
    assert np.array_equal(ref['beat_dist'][0], hist)
    assert hist[..., -1].sum() > 0 and hist[..., :-1].sum() > 0
    for w in range(2):
        s = ref['speed'][:, w]
        for i, l in enumerate(range(-n_lags, n_lags + 1)):
            t = np.arange(max(1, 1 - l), min(T - 1, T - 1 - l) + 1)
            x, y = o[:, t].reshape(-1), s[:, t + l].reshape(-1)
            assert ref['lag_n'][0, i] == len(x) == B * (T - 1 - abs(l))
            want = np.corrcoef(x, y)[0, 1]
            sums = ref['lag_sums'][0, i]
            got = S.pearson(len(x), [sums[0], sums[1], *sums[2 + 3 * w:5 + 3 * w]])
            assert abs(got - want) < 1e-9
    mine = S.metrics(ref['beat_dist'][0], ref['beat_counts'][0], ref['lag_sums'][0], ref['lag_n'][0], 1.5)
    theirs = _sync_metrics(ref['beat_dist'][0], ref['beat_counts'][0], ref['lag_sums'][0], ref['lag_n'][0], 1.5)
    for key, v in mine.items():
        assert np.allclose(theirs[key], v, rtol=1e-13, atol=0, equal_nan=True), key
    assert beat_alignment(np.zeros(4)) != beat_alignment(np.zeros(4))       # NaN: no beats
    assert beat_alignment([0, 0, 3]) == pytest.approx(np.exp(-2.0))
    r = pearson_from_sums([1, 5, 5], [1.0, 5.0, 5.0], [1.0, 5.0, 7.0], [2.0, 5.0, 5.0], [4.0, 9.0, 5.0], [2.0, 5.0, 5.0])
    assert np.isnan(r).all()           # one pair; no variance in x; no variance in y


def test_edges_of_the_definitions():
    """T < 4 has no beats and lag_n follows max(T - 1 - |l|, 0); a constant signal has no beats; a clip
    without audio beats sends its motion beats to the last bin; dropped styles add nothing."""
    g = np.random.default_rng(3)
    for T in (1, 2, 3):
        audio = g.standard_normal((2, T, 8)).astype(np.float32)
        pose = g.standard_normal((2, T, 10)).astype(np.float32)
        ref = S.sync_sums(audio, pose, pose, np.array([0, 7], np.int32), 2, n_lags=2)
        assert not ref['beat_dist'].any() and not ref['beat_counts'].any()
        assert np.array_equal(ref['lag_n'][0], [max(T - 1 - abs(l), 0) for l in range(-2, 3)])
        assert not ref['lag_n'][1].any() and not ref['lag_sums'][1].any()
    audio = np.ones((1, 32, 4), np.float32)
    pose = np.cumsum(g.standard_normal((1, 32, 10)), 1).astype(np.float32)
    ref = S.sync_sums(audio, pose, pose, np.zeros(1, np.int32), 1, n_dist=5)
    n = ref['beat_counts'][0, 1]
    assert ref['beat_counts'][0, 0] == 0 and n > 0
    assert ref['beat_dist'][0, 0, 0, -1] == n and ref['beat_dist'][0, 0, 0, :-1].sum() == 0
    assert not ref['beat_dist'][0, :, 1].any()
    still = np.zeros((1, 32, 10), np.float32)
    assert not S.sync_sums(audio, still, still, np.zeros(1, np.int32), 1)['beat_counts'].any()


@pytest.mark.parametrize('shape', S.RANDOM_SHAPES, ids=_mid)
def test_random_cases_keep_clear_of_the_thresholds(shape):
    """Every random case of tests/test_gpu_sync_eval.py keeps its beat decisions 1e-9 relative away from a
    tie, with audio_std absent and given: a condition on the inputs, not a measurement."""
    assert S.random_case(shape)['margin'] >= 1e-9
