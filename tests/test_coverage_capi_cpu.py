"""a2m_coverage_store_f32, a2m_pair_dist2_f32, a2m_row_kth_f32 and a2m_row_cover_f32 refuse bad arguments
before any launch: each call below returns A2M_EINVAL with an error text of its own prefix.  No GPU is
needed (nothing is launched; the pointers are never followed).  The wrappers and the evaluator refuse host
tensors and bad settings."""
import ctypes

import pytest

OK_PTR = ctypes.c_void_p(0x1000)   # any non-null, 16-byte aligned value: a refused call reads nothing
ODD_PTR = ctypes.c_void_p(0x1004)  # 4-byte, not 16-byte aligned
BYTE_PTR = ctypes.c_void_p(0x1001)

STORE_PTRS = ('fake', 'real', 'style', 'mean', 'std', 'feat_fake', 'feat_real', 'styles')
PAIR_PTRS = ('feat_a', 'rows_a', 'feat_b', 'rows_b', 'slab')
KTH_PTRS = ('slab', 'kth', 'sums')
COVER_PTRS = ('slab', 'r2', 'count', 'rowmin')


def _store_args(**kw):
    a = dict({p: OK_PTR for p in STORE_PTRS}, n=5, T=8, Fd=104, feature=0, row0=3, capacity=20)
    a.update(kw)
    return [a['fake'], a['real'], a['style'], a['mean'], a['std'], a['n'], a['T'], a['Fd'], a['feature'], a['row0'],
            a['capacity'], a['feat_fake'], a['feat_real'], a['styles'], None]


def _pair_args(**kw):
    a = dict({p: OK_PTR for p in PAIR_PTRS}, cap_a=200, nA=100, cap_b=300, nB=150, D=832, exclude_self=0, diag0=0,
             slab_bytes=1 << 20)
    a.update(kw)
    return [a['feat_a'], a['cap_a'], a['rows_a'], a['nA'], a['feat_b'], a['cap_b'], a['rows_b'], a['nB'], a['D'],
            a['exclude_self'], a['diag0'], a['slab'], a['slab_bytes'], None]


def _kth_args(**kw):
    a = dict({p: OK_PTR for p in KTH_PTRS}, nA=100, nB=150, k=5, exclude_self=1)
    a.update(kw)
    return [a['slab'], a['nA'], a['nB'], a['k'], a['exclude_self'], a['kth'], a['sums'], None]


def _cover_args(**kw):
    a = dict({p: OK_PTR for p in COVER_PTRS}, nA=100, nB=150)
    a.update(kw)
    return [a['slab'], a['nA'], a['nB'], a['r2'], a['count'], a['rowmin'], None]


STORE_BAD = [{p: None} for p in STORE_PTRS] + [
    {p: ODD_PTR} for p in ('fake', 'real', 'mean', 'std', 'feat_fake', 'feat_real')] + [
    dict(style=BYTE_PTR), dict(styles=BYTE_PTR), dict(n=0), dict(n=-1), dict(T=0), dict(T=-2), dict(T=1, feature=1),
    dict(Fd=0), dict(Fd=-4), dict(Fd=102), dict(Fd=3), dict(feature=2), dict(feature=-1), dict(row0=-1),
    dict(row0=16), dict(row0=20), dict(capacity=0), dict(capacity=7), dict(row0=1 << 40),
    dict(T=1 << 20, Fd=1 << 12), dict(n=1 << 20, T=1 << 10, Fd=1 << 20, capacity=1 << 30)]
PAIR_BAD = [{p: None} for p in PAIR_PTRS] + [
    dict(feat_a=ODD_PTR), dict(feat_b=ODD_PTR), dict(rows_a=BYTE_PTR), dict(rows_b=BYTE_PTR), dict(slab=BYTE_PTR),
    dict(nA=0), dict(nA=-1), dict(nB=0), dict(nB=-3), dict(cap_a=0), dict(cap_b=-1), dict(D=0), dict(D=-4), dict(D=6),
    dict(D=831), dict(D=(1 << 30) + 4), dict(exclude_self=2), dict(exclude_self=-1), dict(diag0=-1), dict(diag0=1),
    dict(exclude_self=1, diag0=51), dict(exclude_self=1, nA=151), dict(slab_bytes=0),
    dict(slab_bytes=100 * 150 * 4 - 1), dict(nA=65535 * 64 + 1, slab_bytes=1 << 60),
    dict(nB=(1 << 31) - (1 << 16) + 1, slab_bytes=1 << 60), dict(cap_a=1 << 31), dict(cap_b=1 << 31),
    dict(nA=1 << 40, slab_bytes=1 << 62)]
KTH_BAD = [{p: None} for p in KTH_PTRS] + [
    dict(slab=BYTE_PTR), dict(kth=BYTE_PTR), dict(sums=ODD_PTR), dict(nA=0), dict(nA=-1), dict(nB=0), dict(nB=-1),
    dict(k=0), dict(k=-1), dict(k=33), dict(exclude_self=2), dict(exclude_self=-1), dict(k=5, nB=5),
    dict(k=32, nB=32), dict(k=5, nB=4, exclude_self=0), dict(nA=(1 << 31) - (1 << 16) + 1), dict(nB=1 << 31),
    dict(nA=1 << 40)]
COVER_BAD = [{p: None} for p in COVER_PTRS] + [
    {p: BYTE_PTR} for p in COVER_PTRS] + [
    dict(nA=0), dict(nA=-1), dict(nB=0), dict(nB=-1), dict(nA=(1 << 31) - (1 << 16) + 1), dict(nB=1 << 31)]


def _ids(d):
    return '-'.join(f'{k}{"" if v is None else hex(v.value) if isinstance(v, ctypes.c_void_p) else v}' for k, v in d.items())


@pytest.mark.parametrize('bad', STORE_BAD, ids=_ids)
def test_coverage_store_refuses_bad_arguments(bad):
    from a2m import _native as N
    assert N.lib.a2m_coverage_store_f32(*_store_args(**bad)) == N.A2M_EINVAL
    assert N.last_error().startswith('coverage_store:')


@pytest.mark.parametrize('bad', PAIR_BAD, ids=_ids)
def test_pair_dist2_refuses_bad_arguments(bad):
    from a2m import _native as N
    assert N.lib.a2m_pair_dist2_f32(*_pair_args(**bad)) == N.A2M_EINVAL
    assert N.last_error().startswith('pair_dist2:')


@pytest.mark.parametrize('bad', KTH_BAD, ids=_ids)
def test_row_kth_refuses_bad_arguments(bad):
    from a2m import _native as N
    assert N.lib.a2m_row_kth_f32(*_kth_args(**bad)) == N.A2M_EINVAL
    assert N.last_error().startswith('row_kth:')


@pytest.mark.parametrize('bad', COVER_BAD, ids=_ids)
def test_row_cover_refuses_bad_arguments(bad):
    from a2m import _native as N
    assert N.lib.a2m_row_cover_f32(*_cover_args(**bad)) == N.A2M_EINVAL
    assert N.last_error().startswith('row_cover:')


def test_slab_sizes():
    """The slab is the workspace: 4 bytes an element, 0 for sizes the entry refuses.  A test split of 6,640
    clips in blocks of 4,096 rows needs 109 MB, not the 176 MB of the whole matrix."""
    from a2m import _native as N
    f = N.lib.a2m_pair_dist2_ws_bytes
    assert f(1, 1) == 4 and f(100, 150) == 60000 and f(4096, 6640) == 4096 * 6640 * 4 < 6640 * 6640 * 4
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(-1, 5) == 0 and f(65535 * 64 + 1, 1) == 0 and f(1, 1 << 31) == 0
    assert f(65535 * 64, 1) == 65535 * 64 * 4


def test_wrappers_refuse_host_tensors():
    import torch
    from a2m import functional as F
    feat, rows = torch.zeros(10, 8), torch.zeros(4, dtype=torch.int32)
    x, st, stat = torch.zeros(2, 3, 8), torch.zeros(2, dtype=torch.int32), torch.ones(8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.coverage_store(x, x, st, stat, stat, 0, torch.zeros(10, 24), torch.zeros(10, 24),
                         torch.zeros(10, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.pair_dist2(feat, rows, feat, rows)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.row_kth(torch.zeros(4, 4), 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        F.row_cover(torch.zeros(4, 4), torch.zeros(4))


def test_evaluator_refuses_bad_settings():
    """Refused on the host before anything is allocated on a device."""
    import numpy as np
    from a2m.evaluation import CoverageEvaluator
    stat = np.ones(104, np.float32)
    for kw in (dict(k=0), dict(k=33), dict(feature='velocity'), dict(capacity=0), dict(n_styles=0),
               dict(T=1, feature='motion'), dict(T=0), dict(block_rows=0)):
        args = dict(n_styles=2, capacity=10, T=8, device='cpu')
        args.update(kw)
        with pytest.raises(ValueError):
            CoverageEvaluator(stat, stat, **args)
    with pytest.raises(ValueError, match='multiple of 4'):
        CoverageEvaluator(np.ones(6, np.float32), np.ones(6, np.float32), 2, 10, 8, device='cpu')
