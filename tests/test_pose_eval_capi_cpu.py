"""a2m_eval_clip_f32, a2m_eval_gram_f64 and a2m_eval_finish_f64 refuse bad arguments before any
launch: each call below returns A2M_EINVAL with an error text of its own prefix.  No GPU is needed
(nothing is launched; the pointers are never followed)."""
import ctypes

import pytest

OK_PTR = ctypes.c_void_p(0x1000)   # any non-null value: a refused call reads nothing

CLIP_PTRS = ('fake_norm', 'real_px', 'style', 'mean', 'std', 'fake_px', 'part', 'hits', 'hist')
GRAM_PTRS = ('fake_px', 'real_px', 'style', 'sx', 'gram')
FINISH_PTRS = ('part', 'hits', 'style', 'counts', 'sums')


def _clip_args(**kw):
    a = dict({p: OK_PTR for p in CLIP_PTRS}, B=2, T=8, F=104, n_styles=3, alpha=0.2, n_bins=512, sw=0.125, aw=0.125)
    a.update(kw)
    return [a['fake_norm'], a['real_px'], a['style'], a['mean'], a['std'], a['B'], a['T'], a['F'], a['n_styles'],
            a['alpha'], a['n_bins'], a['sw'], a['aw'], a['fake_px'], a['part'], a['hits'], a['hist'], None]


def _gram_args(**kw):
    a = dict({p: OK_PTR for p in GRAM_PTRS}, B=2, T=8, F=104, n_styles=3)
    a.update(kw)
    return [a['fake_px'], a['real_px'], a['style'], a['B'], a['T'], a['F'], a['n_styles'], a['sx'], a['gram'], None]


def _finish_args(**kw):
    a = dict({p: OK_PTR for p in FINISH_PTRS}, B=2, T=8, n_styles=3)
    a.update(kw)
    return [a['part'], a['hits'], a['style'], a['B'], a['T'], a['n_styles'], a['counts'], a['sums'], None]


CLIP_BAD = [{p: None} for p in CLIP_PTRS] + [
    dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(F=0), dict(F=2), dict(F=105), dict(F=-104), dict(n_styles=0),
    dict(n_styles=-2), dict(n_bins=0), dict(n_bins=-1), dict(sw=0.0), dict(aw=-1.0), dict(F=2562),
    dict(T=1 << 22, F=1024)]
GRAM_BAD = [{p: None} for p in GRAM_PTRS] + [
    dict(B=0), dict(B=-1), dict(T=0), dict(F=0), dict(F=-8), dict(n_styles=0), dict(n_styles=-1),
    dict(n_styles=1 << 16), dict(T=1 << 22, F=1024)]
FINISH_BAD = [{p: None} for p in FINISH_PTRS] + [dict(B=0), dict(B=-1), dict(T=0), dict(n_styles=0), dict(n_styles=-1)]


def _ids(d):
    return '-'.join(f'{k}{v}' for k, v in d.items())


@pytest.mark.parametrize('bad', CLIP_BAD, ids=_ids)
def test_eval_clip_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_eval_clip_f32(*_clip_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('eval_clip:')


@pytest.mark.parametrize('bad', GRAM_BAD, ids=_ids)
def test_eval_gram_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_eval_gram_f64(*_gram_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('eval_gram:')


@pytest.mark.parametrize('bad', FINISH_BAD, ids=_ids)
def test_eval_finish_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_eval_finish_f64(*_finish_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('eval_finish:')


def test_wrappers_refuse_host_and_wrong_dtype_tensors():
    import torch
    from a2m import functional as F
    from a2m.evaluation import PoseEvaluator
    pose, stat = torch.zeros(2, 8, 104), torch.zeros(104)
    style = torch.zeros(2, dtype=torch.int32)
    hist = torch.zeros(3, 4, 16, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.eval_clip(pose, pose, style, stat, stat, 3, 0.2, 0.125, 0.125, hist)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.eval_gram(pose, pose, style, torch.zeros(3, 2, 104, dtype=torch.float64),
                    torch.zeros(3, 2, 104, 104, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.eval_finish(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), style, 8,
                      torch.zeros(10, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.float64))
    for bad in (dict(n_styles=0), dict(n_styles=2, n_bins=0), dict(n_styles=2, speed_max=0.0)):
        with pytest.raises(ValueError, match='positive'):
            PoseEvaluator(stat, stat, device='cpu', **bad)
    with pytest.raises(ValueError, match='2K'):
        PoseEvaluator(torch.zeros(3), torch.zeros(3), 2, device='cpu')
