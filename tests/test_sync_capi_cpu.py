"""a2m_eval_sync_f64 and a2m_eval_sync_finish_f64 refuse bad arguments before any launch: each call
below returns A2M_EINVAL with an error text of its own prefix.  No GPU is needed (nothing is launched;
the pointers are never followed)."""
import ctypes

import pytest

OK_PTR = ctypes.c_void_p(0x1000)   # any non-null value: a refused call reads nothing

SYNC_PTRS = ('audio', 'fake_px', 'real_px', 'style', 'beat_dist', 'beat_counts', 'part')
SYNC_NULLABLE = ('audio_std', 'onset_out', 'speed_out')
FINISH_PTRS = ('part', 'style', 'lag_sums', 'lag_n')


def _sync_args(**kw):
    a = dict({p: OK_PTR for p in SYNC_PTRS + SYNC_NULLABLE}, B=2, T=8, C=128, F=104, n_styles=3, n_lags=4, n_dist=32,
             delta=1.0)
    a.update(kw)
    return [a['audio'], a['fake_px'], a['real_px'], a['style'], a['audio_std'], a['B'], a['T'], a['C'], a['F'],
            a['n_styles'], a['n_lags'], a['n_dist'], a['delta'], a['beat_dist'], a['beat_counts'], a['part'],
            a['onset_out'], a['speed_out'], None]


def _finish_args(**kw):
    a = dict({p: OK_PTR for p in FINISH_PTRS}, B=2, T=8, n_styles=3, n_lags=4)
    a.update(kw)
    return [a['part'], a['style'], a['B'], a['T'], a['n_styles'], a['n_lags'], a['lag_sums'], a['lag_n'], None]


SYNC_BAD = [{p: None} for p in SYNC_PTRS] + [
    dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(C=0), dict(C=-128), dict(n_styles=0), dict(n_styles=-2),
    dict(n_dist=0), dict(n_dist=-4), dict(n_dist=1), dict(F=0), dict(F=2), dict(F=105), dict(F=-104), dict(n_lags=-1),
    dict(n_lags=17), dict(T=2049), dict(delta=-0.5), dict(delta=float('nan')), dict(delta=float('inf')),
    dict(T=2048, C=1 << 21)]
FINISH_BAD = [{p: None} for p in FINISH_PTRS] + [
    dict(B=0), dict(B=-1), dict(T=0), dict(n_styles=0), dict(n_styles=-1), dict(n_lags=-1), dict(n_lags=17)]


def _ids(d):
    return '-'.join(f'{k}{v}' for k, v in d.items())


@pytest.mark.parametrize('bad', SYNC_BAD, ids=_ids)
def test_eval_sync_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_eval_sync_f64(*_sync_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('eval_sync:')


@pytest.mark.parametrize('bad', FINISH_BAD, ids=_ids)
def test_eval_sync_finish_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_eval_sync_finish_f64(*_finish_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('eval_sync_finish:')


def test_wrappers_refuse_host_tensors_and_bad_sizes():
    """The wrappers and AudioSyncEvaluator.update refuse host tensors ("no CPU fallback" comes before every
    dtype check, so wrong dtypes on device tensors are in tests/test_gpu_sync_eval.py), and the evaluator
    refuses sizes out of range."""
    import torch
    from a2m import functional as F
    from a2m.evaluation import AudioSyncEvaluator
    audio, pose = torch.zeros(2, 8, 128), torch.zeros(2, 8, 104)
    style = torch.zeros(2, dtype=torch.int32)
    dist, counts = torch.zeros(3, 2, 2, 32, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.eval_sync(audio, pose, pose, style, dist, counts)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.eval_sync_finish(torch.zeros(2, 9, 8, dtype=torch.float64), style, 8,
                           torch.zeros(3, 9, 8, dtype=torch.float64), torch.zeros(3, 9, dtype=torch.int64))
    ev = AudioSyncEvaluator(3, device='cpu')
    assert sorted(ev.state()) == ['beat_counts', 'beat_dist', 'lag_n', 'lag_sums']
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ev.update(audio, pose, pose, style)
    for bad in (dict(n_styles=0), dict(n_styles=-1), dict(n_styles=2, n_dist=1), dict(n_styles=2, n_dist=0),
                dict(n_styles=2, n_lags=-1), dict(n_styles=2, n_lags=17), dict(n_styles=2, onset_delta=-1.0),
                dict(n_styles=2, onset_delta=float('nan'))):
        with pytest.raises(ValueError):
            AudioSyncEvaluator(device='cpu', **bad)

