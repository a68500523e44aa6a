"""a2m_nn_search_f32 and a2m_window_median_f32 refuse bad arguments before any launch: each call
below returns A2M_EINVAL with an error text of its own prefix.  No GPU is needed (nothing is
launched; the pointers are never followed).  The wrappers refuse host tensors and the modules a
loader that lacks a modality."""
import ctypes

import pytest

OK_PTR = ctypes.c_void_p(0x1000)   # any non-null, 16-byte aligned value: a refused call reads nothing
ODD_PTR = ctypes.c_void_p(0x1004)

NN_PTRS = ('arena', 'start', 'query', 'best', 'best_dist', 'ws')
MED_PTRS = ('arena', 'start', 'out', 'ws')


def _nn_args(**kw):
    a = dict({p: OK_PTR for p in NN_PTRS}, lo=3, n_cand=100, C=128, window=382, interval=6, mode=0, mean=None,
             std=None, B=5, ws_bytes=1 << 20)
    a.update(kw)
    return [a['arena'], a['start'], a['lo'], a['n_cand'], a['C'], a['window'], a['interval'], a['mode'], a['mean'],
            a['std'], a['query'], a['B'], a['best'], a['best_dist'], a['ws'], a['ws_bytes'], None]


def _med_args(**kw):
    a = dict({p: OK_PTR for p in MED_PTRS}, lo=3, n=100, C=104, window=64, interval=1, mode=2, ws_bytes=1 << 20)
    a.update(kw)
    return [a['arena'], a['start'], a['lo'], a['n'], a['C'], a['window'], a['interval'], a['mode'], a['out'], a['ws'],
            a['ws_bytes'], None]


NN_BAD = [{p: None} for p in NN_PTRS] + [
    dict(B=0), dict(B=-1), dict(n_cand=0), dict(n_cand=-5), dict(window=0), dict(window=-1), dict(interval=0),
    dict(interval=-2), dict(C=0), dict(C=-4), dict(C=6), dict(C=127), dict(lo=-1), dict(mode=2), dict(mode=3),
    dict(mode=-1), dict(mode=0, mean=OK_PTR), dict(mode=0, std=OK_PTR), dict(mode=0, mean=OK_PTR, std=OK_PTR),
    dict(mode=1), dict(mode=1, mean=OK_PTR), dict(mode=1, std=OK_PTR), dict(arena=ODD_PTR), dict(query=ODD_PTR),
    dict(ws_bytes=0), dict(ws_bytes=2 * 5 * 8 - 1),                      # 100 candidates: two chunks of 64
    dict(n_cand=(1 << 31) - (1 << 16) + 1, ws_bytes=1 << 40), dict(n_cand=1 << 40, ws_bytes=1 << 60),
    dict(window=1 << 22, interval=1, C=1024), dict(window=(1 << 30) + 1, interval=1, C=4)]
MED_BAD = [{p: None} for p in MED_PTRS] + [
    dict(n=0), dict(n=-1), dict(window=0), dict(window=-3), dict(interval=0), dict(interval=-1), dict(C=0),
    dict(C=-104), dict(C=102, mode=0), dict(C=(1 << 20) + 4, mode=0, ws_bytes=1 << 40), dict(lo=-1), dict(mode=1),
    dict(mode=3), dict(mode=-1), dict(mode=2, C=128), dict(mode=2, C=52), dict(arena=ODD_PTR), dict(ws_bytes=0),
    dict(ws_bytes=(104 * 4 + 4 * 104 * 512) * 4 - 1), dict(n=1 << 26, window=64), dict(n=1 << 32, window=1),
    dict(n=(1 << 32) - 1, window=2, interval=1)]


def _ids(d):
    return '-'.join(f'{k}{"" if v is None else v.value if isinstance(v, ctypes.c_void_p) else v}' for k, v in d.items())


@pytest.mark.parametrize('bad', NN_BAD, ids=_ids)
def test_nn_search_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_nn_search_f32(*_nn_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('nn_search:')


@pytest.mark.parametrize('bad', MED_BAD, ids=_ids)
def test_window_median_refuses_bad_arguments(bad):
    from a2m import _native as N
    rc = N.lib.a2m_window_median_f32(*_med_args(**bad))
    assert rc == N.A2M_EINVAL
    assert N.last_error().startswith('window_median:')


def test_workspace_sizes():
    """One 8-byte (distance bits, position) slot per query and 64-candidate tile up to 2048 chunks, then
    per chunk of several tiles; the median's state and four passes of two 256-bin histograms a channel."""
    from a2m import _native as N
    f = N.lib.a2m_nn_search_ws_bytes
    assert f(5, 1) == 5 * 8 and f(5, 64) == 5 * 8 and f(5, 65) == 2 * 5 * 8 and f(64, 20000) == 313 * 64 * 8
    assert f(3, 64 * 2048) == 2048 * 3 * 8 and f(3, 64 * 2048 + 1) == 1025 * 3 * 8
    assert f(0, 10) == 0 and f(3, 0) == 0 and f(3, 1 << 40) == 0
    g = N.lib.a2m_window_median_ws_bytes
    assert g(104) == (104 * 4 + 4 * 104 * 512) * 4 and g(0) == 0 and g(-4) == 0


def test_wrappers_refuse_host_tensors():
    import torch
    from a2m import functional as F
    arena, start = torch.zeros(100, 8), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.nn_search(torch.zeros(2, 3, 8), arena, start, 0, 4, 5, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.window_median(arena, start, 0, 4, 5, 2)


def test_modules_refuse_a_loader_without_both_modalities():
    """A loader of poses alone, of audio alone, and one whose pose and audio windows differ in length;
    built on the host (the refusal comes before any native call)."""
    import numpy as np
    import pats_data_ref as P
    from a2m.baselines import MedianPose, NearestAudio, RandomClip, evaluate_baselines
    from a2m.data import PatsLoader
    arr = P.arrays()
    stat = np.ones(104, np.float32)
    for mods, fs in (((P.POSE,), (15,)), ((P.AUDIO,), (15,))):
        loader = PatsLoader(arr, P.table(), 'oliver', modalities=mods, fs_new=fs, time=P.TIME, window_hop=5,
                            device='cpu')
        for cls in (MedianPose, RandomClip, NearestAudio):
            with pytest.raises(ValueError, match='one pose and one audio'):
                cls(loader, stat, stat)
        with pytest.raises(ValueError, match='one pose and one audio'):
            evaluate_baselines(loader, 'train', pose_mean=stat, pose_std=stat)
    loader = PatsLoader(arr, P.table(), 'oliver', time=P.TIME, fs_new=(15, 30), window_hop=5, device='cpu')
    with pytest.raises(ValueError, match='pose windows hold 64 rows, audio windows 128'):
        NearestAudio(loader, stat, stat)
    loader = PatsLoader(arr, P.table(), 'oliver', time=P.TIME, fs_new=P.FS_NEW, window_hop=5, device='cpu')
    with pytest.raises(ValueError, match='no clip'):
        RandomClip(loader, stat, stat, split='dev')
    with pytest.raises(ValueError, match='pose_mean and pose_std'):
        RandomClip(loader, None, None)
