"""a2m_val_motion_f32 and a2m_val_finish_f32 refuse bad arguments before any launch: each call
below returns A2M_EINVAL with an error text.  No GPU is needed (nothing is launched; the pointers
are never followed)."""
import ctypes

import pytest

OK_PTR = ctypes.c_void_p(0x1000)   # any non-null value: a refused call reads nothing


def _motion_args(**kw):
    a = dict(fake=OK_PTR, real=OK_PTR, B=2, T=8, Fd=104, motion=OK_PTR, part=OK_PTR)
    a.update(kw)
    return [a['fake'], a['real'], a['B'], a['T'], a['Fd'], a['motion'], a['part'], None]


def _finish_args(**kw):
    a = dict(part=OK_PTR, B=2, T=8, Fd=104, logits=OK_PTR, L=4, bone=OK_PTR, angle=OK_PTR, acc=OK_PTR)
    a.update(kw)
    return [a['part'], a['B'], a['T'], a['Fd'], a['logits'], a['L'], a['bone'], a['angle'], 1.0, 1.0, a['acc'], None]


MOTION_BAD = [dict(fake=None), dict(real=None), dict(motion=None), dict(part=None), dict(B=0), dict(B=-1),
              dict(T=1), dict(T=0), dict(Fd=0), dict(Fd=-4), dict(Fd=1921), dict(T=1 << 22, Fd=1024)]
FINISH_BAD = [dict(part=None), dict(logits=None), dict(bone=None), dict(angle=None), dict(acc=None), dict(B=0),
              dict(T=1), dict(Fd=0), dict(L=0), dict(L=-1)]


@pytest.mark.parametrize('bad', MOTION_BAD, ids=lambda d: '-'.join(f'{k}{v}' for k, v in d.items()))
def test_val_motion_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_val_motion_f32(*_motion_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('val_motion:')


@pytest.mark.parametrize('bad', FINISH_BAD, ids=lambda d: '-'.join(f'{k}{v}' for k, v in d.items()))
def test_val_finish_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_val_finish_f32(*_finish_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('val_finish:')


def test_wrappers_refuse_host_and_wrong_dtype_tensors():
    import torch
    from a2m import functional as F
    pose = torch.zeros(2, 8, 104)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.val_motion(pose, pose)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.val_finish(torch.zeros(2, 3, dtype=torch.float64), 8, 104, torch.zeros(4, 4), torch.zeros(()),
                     torch.zeros(()), 1.0, 1.0, torch.zeros(8, dtype=torch.float64))
