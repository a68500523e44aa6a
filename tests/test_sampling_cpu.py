"""The train samplers without a GPU: the argument checks of a2m_clip_velocity_f32, a2m_select_f32
and a2m_classify_f32 (csrc/sampling.hip), which return before any launch, and
PatsLoader.train_sampler on a host velocity array (velocity=), where the thresholds, the bins and
the class lists come from numpy: the precedence, every refusal, the subsets against the float64
statements of tests/sampling_ref.py, and every order against torch's own samplers or draws under
the same seed.  The loader lives on the CPU device here: nothing is launched."""
import ctypes

import numpy as np
import pytest
import torch
from torch.utils.data import RandomSampler, SubsetRandomSampler, WeightedRandomSampler

import pats_data_ref as P
import sampling_ref as S

ARR = S.arrays()
IDS = list('ABCD')
VEL = S.clip_velocities(ARR, IDS, 5)          # float64 [13]


# ------------------------------------------------------------------------------ the C entry points
@pytest.fixture(scope='module')
def abi():
    from a2m import _native as N
    buf = (ctypes.c_float * 1024)()
    addr = (ctypes.addressof(buf) + 15) // 16 * 16
    return N, addr


def _velocity(N, addr, arena=True, start=True, lo=0, n=4, C=104, window=64, interval=1, out=True, bad=True):
    def p(f):
        return addr if f else None
    return N.lib.a2m_clip_velocity_f32(p(arena), p(start), lo, n, C, window, interval, p(out), p(bad), None)


def _select(N, addr, x=True, n=5, ranks=(0, 4), k=None, out=True, minmax=True, ws=True, ws_off=0, ws_bytes=None):
    def p(f):
        return addr if f else None
    r = None if ranks is None else (ctypes.c_int64 * max(len(ranks), 1))(*ranks)
    k = (0 if ranks is None else len(ranks)) if k is None else k
    ws_bytes = N.lib.a2m_select_f32_ws_bytes(n) if ws_bytes is None else ws_bytes
    return N.lib.a2m_select_f32(p(x), n, r, k, p(out), p(minmax), (addr + ws_off) if ws else None, ws_bytes, None)


def _classify(N, addr, x=True, n=5, kind=2, thr=(0., 1., 2.), n_thr=None, cls=True, counts=True):
    def p(f):
        return addr if f else None
    t = None if thr is None else (ctypes.c_double * max(len(thr), 1))(*thr)
    n_thr = (0 if thr is None else len(thr)) if n_thr is None else n_thr
    return N.lib.a2m_classify_f32(p(x), n, kind, t, n_thr, p(cls), p(counts), None)


REFUSED = {
    'clip_velocity': (_velocity, {
        'negative n': dict(n=-1),
        'negative lo': dict(lo=-2),
        'null arena': dict(arena=False),
        'null start': dict(start=False),
        'null out': dict(out=False),
        'null n_nonfinite': dict(bad=False),
        'odd C': dict(C=103),
        'one joint': dict(C=2),
        'C 0': dict(C=0),
        'window 0': dict(window=0),
        'window negative': dict(window=-64),
        'interval 0': dict(interval=0),
        'interval negative': dict(interval=-1),
        'one frame': dict(window=1),
        'one frame at interval 6': dict(window=6, interval=6),
    }),
    'select': (_select, {
        'negative n': dict(n=-1),
        'n 2^32': dict(n=1 << 32, ws_bytes=1 << 20),
        'null x': dict(x=False),
        'null ranks': dict(ranks=None, k=2),
        'null out': dict(out=False),
        'null minmax': dict(minmax=False),
        'null ws': dict(ws=False),
        'k 0': dict(ranks=(), k=0),
        'k 9': dict(ranks=(0,) * 9),
        'rank n': dict(ranks=(0, 5)),
        'rank negative': dict(ranks=(-1, 2)),
        'ws misaligned': dict(ws_off=2),
        'ws too small': dict(ws_bytes=64),
    }),
    'classify': (_classify, {
        'negative n': dict(n=-1),
        'unknown kind': dict(kind=3),
        'negative kind': dict(kind=-1),
        'null x': dict(x=False),
        'null thr': dict(thr=None, n_thr=3),
        'null cls': dict(cls=False),
        'null counts': dict(counts=False),
        'above with 2': dict(kind=0, thr=(0., 1.)),
        'tail with 1': dict(kind=1, thr=(0.,)),
        'tail with 3': dict(kind=1),
        'bins with 1 edge': dict(thr=(0.,)),
        'bins with 258 edges': dict(thr=tuple(float(j) for j in range(258))),
        'NaN threshold': dict(kind=0, thr=(float('nan'),)),
        'NaN edge': dict(thr=(0., float('nan'), 2.)),
        'descending edges': dict(thr=(0., 2., 1.)),
    }),
}


@pytest.mark.parametrize('entry,case', [(e, c) for e, (_, cases) in REFUSED.items() for c in cases])
def test_entry_points_refuse_before_any_launch(abi, entry, case):
    N, addr = abi
    call, cases = REFUSED[entry]
    assert N.lib.a2m_window_gather_f32(None, 0, 0, None, 0, 0, 0, None, None, None, None) == N.A2M_EINVAL
    assert entry not in N.last_error()
    assert call(N, addr, **cases[case]) == N.A2M_EINVAL, case
    assert N.last_error().startswith(entry + ':'), N.last_error()


def test_empty_input_is_a_no_op(abi):
    """n = 0: nothing to read, nothing launched, whatever the pointers."""
    N, addr = abi
    assert N.lib.a2m_clip_velocity_f32(None, None, 0, 0, 0, 0, 0, None, None, None) == 0
    assert N.lib.a2m_select_f32(None, 0, None, 0, None, None, None, 0, None) == 0
    assert N.lib.a2m_classify_f32(None, 0, 0, None, 0, None, None, None) == 0
    assert N.lib.a2m_classify_f32(None, 0, 2, None, 0, None, None, None) == 0
    assert _velocity(N, addr, n=0, C=103, window=0) == 0
    assert N.lib.a2m_select_f32_ws_bytes(1) > 0 and N.lib.a2m_select_f32_ws_bytes(70001) > 0
    assert {'a2m_clip_velocity_f32', 'a2m_select_f32', 'a2m_select_f32_ws_bytes', 'a2m_classify_f32'} <= set(
        N.exported_symbols())


def test_header_and_library_agree_on_the_new_symbols():
    from test_capi_cpu import header_symbols
    from a2m import _native as N
    syms = header_symbols()
    for name in ('a2m_clip_velocity_f32', 'a2m_select_f32', 'a2m_select_f32_ws_bytes', 'a2m_classify_f32'):
        assert name in syms and hasattr(N.lib, name)
    assert sorted(N.SIGNATURES) == syms


# ------------------------------------------------------------------------------ the fixture's properties
def test_the_fixture_is_what_the_tests_assume():
    assert len(VEL) == 13 == sum(P.COUNTS[5]) and len(set(VEL.tolist())) == 13
    assert 0.37 < VEL.min() < 0.38 and 7.5 < VEL.max() < 7.6
    assert [len(c) for c in S.rebalance(VEL, 3)] == [1, 4, 8]
    ordered = np.sort(VEL)
    for q in (0.9, 0.4):
        thr = S.quantile(VEL, q)
        assert ordered[int(np.floor(q * 12))] < thr < ordered[int(np.ceil(q * 12))]
        assert np.abs(VEL - thr).min() > 1e-3 * thr
    assert S.quantile(VEL, 0.5) == ordered[6]
    assert S.quantile(VEL, 0.25) == ordered[3] and np.abs(VEL - S.quantile(VEL, 0.9)).min() > 1e-3


# ------------------------------------------------------------------------------ train_sampler on a host velocity
def _table(two_speakers=False):
    # two speakers with their intervals interleaved in id order: A, D speak as one, B, C as the other
    return [P.row('train', i, ('oliver' if i in 'AD' else 'seth') if two_speakers else 'oliver') for i in IDS]


def _loader(two_speakers=False, batch_size=4, **kw):
    from a2m.data import PatsLoader
    speaker = ['seth', 'oliver'] if two_speakers else 'oliver'
    return PatsLoader(ARR, _table(two_speakers), speaker, time=P.TIME, fs_new=P.FS_NEW, window_hop=5,
                      batch_size=batch_size, device='cpu', **kw)


@pytest.fixture(scope='module')
def loader():
    return _loader()


def test_precedence_is_the_references(loader):
    every = dict(style_iters=2, num_training_sample=5, quantile_sample=0.5, weighted=2, num_training_iters=3)
    kinds = []
    for name in ('style_iters', 'num_training_sample', 'quantile_sample', 'weighted', 'num_training_iters'):
        s = loader.train_sampler('train', velocity=VEL, **every)
        kinds.append(s.kind)
        del every[name]
    assert kinds == ['alternate', 'few_shot', 'above', 'weighted', 'iters']
    assert loader.train_sampler('train', velocity=VEL) is None
    assert loader.train_sampler('train', quantile_num_training_sample=3) is None
    assert loader.train_sampler(quantile_sample=[0.25, 0.9], velocity=VEL).kind == 'tail'
    assert loader.train_sampler(quantile_sample=3, quantile_num_training_sample=2, velocity=VEL).kind == 'rebalance'


@pytest.mark.parametrize('bad', [1, 1.0, -0.1, -3, [0.5], [0.1, 0.5, 0.9], [0.5, 1.5], [-0.1, 0.5], 'high',
                                 float('nan')])
def test_quantile_argument_refusals(loader, bad):
    with pytest.raises(ValueError, match='quantile_sample'):
        loader.train_sampler(quantile_sample=bad, quantile_num_training_sample=2, velocity=VEL)


def test_other_refusals(loader):
    with pytest.raises(ValueError, match='quantile_num_training_sample'):
        loader.train_sampler(quantile_sample=3, velocity=VEL)
    with pytest.raises(NotImplementedError, match='sample_all_styles'):
        loader.train_sampler(sample_all_styles=1, style_iters=2)
    with pytest.raises(NotImplementedError, match='sample_all_styles'):
        loader.train_sampler(sample_all_styles=1)
    bad = VEL.copy()
    bad[[2, 7]] = np.nan, np.inf
    with pytest.raises(ValueError, match='2 of the 13 clips'):
        loader.train_sampler(quantile_sample=0.5, velocity=bad)
    with pytest.raises(ValueError, match='12 values'):
        loader.train_sampler(quantile_sample=0.5, velocity=VEL[:12])
    with pytest.raises(ValueError, match='no clips'):
        loader.train_sampler('dev', weighted=1)
    s = loader.train_sampler(weighted=1)
    with pytest.raises(ValueError, match='give one'):
        loader.pairs('train', sampler=s, order=[0, 1])
    with pytest.raises(ValueError, match='built for'):
        loader.pairs('dev', sampler=s)
    with pytest.raises(NotImplementedError):                    # the constructor refuses them as before
        _loader(quantile_sample=0.5)


@pytest.mark.parametrize('q', [0, 0.4, 0.5, 0.9, [0.25, 0.9]], ids=str)
def test_above_and_tail_subsets(loader, q):
    s = loader.train_sampler(quantile_sample=q, velocity=VEL)
    qs = q if isinstance(q, list) else [q]
    want = S.tail(VEL, *q) if isinstance(q, list) else S.above(VEL, q)
    assert s.kind == ('tail' if isinstance(q, list) else 'above') and len(s.classes) == 1
    assert np.array_equal(s.classes[0], want) and len(s) == len(want) and s.classes[0].dtype == np.int64
    for thr, x in zip(s.thresholds, qs):
        assert abs(thr - np.quantile(VEL, x)) <= 1e-12 * abs(np.quantile(VEL, x)), (thr, x)
    if q == 0.5:
        on = int(np.argsort(VEL)[6])
        assert s.thresholds[0] == VEL[on] and on not in s.classes[0] and len(want) == 6
    if q == 0:
        assert len(want) == 12 and int(np.argmin(VEL)) not in want
    if isinstance(q, list):
        assert len(want) == 5                                       # 3 below the element of rank 3, 2 above Q(0.9)
    # two consecutive passes in SubsetRandomSampler's order under one seed
    torch.manual_seed(6)
    got = [s.draw(), s.draw()]
    torch.manual_seed(6)
    ref = SubsetRandomSampler(want.tolist())
    for g in got:
        assert g.dtype == np.int64 and np.array_equal(g, np.asarray(list(ref), np.int64))
    if len(want) > 3:
        assert not np.array_equal(got[0], got[1])


@pytest.mark.parametrize('q,sizes', [(3, [1, 4, 8]), (8, None), (3.7, [1, 4, 8])], ids=str)
def test_rebalance(loader, q, sizes):
    s = loader.train_sampler(quantile_sample=q, quantile_num_training_sample=5, velocity=VEL)
    want = S.rebalance(VEL, int(q))
    assert s.kind == 'rebalance' and len(s.classes) == len(want)
    assert all(np.array_equal(a, b) for a, b in zip(s.classes, want))
    if sizes:
        assert [len(c) for c in s.classes] == sizes
    else:
        assert len(want) < 8 and all(len(c) for c in s.classes) and sum(len(c) for c in s.classes) == 13
    assert s.thresholds == S.edges(VEL, int(q)) and s.thresholds[-1] == VEL.max()
    nc = len(want)
    m = 5 * 4 // nc
    assert len(s) == m * nc
    gen = torch.Generator().manual_seed(9)
    s.generator = gen
    got = [s.draw(), s.draw()]
    gen = torch.Generator().manual_seed(9)
    for g in got:
        assert g.shape == (m * nc,) and g.dtype == np.int64
        draws = [c[torch.randint(0, len(c), (m,), generator=gen).numpy()] for c in want]   # class by class
        for p, idx in enumerate(g):
            assert idx == draws[p % nc][p // nc] and idx in want[p % nc]
    assert not np.array_equal(got[0], got[1])


def test_alternate_over_interleaved_speakers():
    """B, C as speaker 0 and A, D as speaker 1 (B holds no clip): class 0 is C's one clip (global index
    4), class 1 is A's 4 and D's 8, which are not contiguous in the concatenation (0..3 and 5..12)."""
    loader = _loader(two_speakers=True, batch_size=5)
    s = loader.train_sampler(style_iters=3)
    want = [np.arange(4, 5), np.r_[0:4, 5:13]]
    assert s.kind == 'alternate' and all(np.array_equal(a, b) for a, b in zip(s.classes, want))
    m = 3 * 5 // 2
    assert len(s) == 2 * m == 14
    torch.manual_seed(2)
    got = [s.draw(), s.draw()]
    torch.manual_seed(2)
    for g in got:
        draws = [c[torch.randint(0, len(c), (m,)).numpy()] for c in want]
        assert np.array_equal(g, np.stack(draws, 1).reshape(-1))
        assert all(g[p] in want[p % 2] for p in range(len(g)))
    assert not np.array_equal(got[0], got[1])
    one = _loader().train_sampler(style_iters=3)                   # one speaker: one class, every clip
    assert len(one.classes) == 1 and np.array_equal(one.classes[0], np.arange(13)) and len(one) == 12


def test_weighted_iters_and_few_shot_are_torchs(loader):
    torch.manual_seed(4)
    s = loader.train_sampler(weighted=3)
    got = [s.draw(), s.draw()]
    torch.manual_seed(4)
    ref = WeightedRandomSampler([1] * 13, 3 * 4)
    assert len(s) == 12 and all(np.array_equal(g, np.asarray(list(ref))) for g in got)
    assert not np.array_equal(got[0], got[1]) and s.classes == []

    torch.manual_seed(4)
    s = loader.train_sampler(num_training_iters=5)
    got = [s.draw(), s.draw()]
    torch.manual_seed(4)
    ref = RandomSampler(range(13), replacement=True, num_samples=5 * 4)
    assert len(s) == 20 and all(np.array_equal(g, np.asarray(list(ref))) for g in got)
    assert not np.array_equal(got[0], got[1]) and max(got[0]) < 13

    torch.manual_seed(4)
    s = loader.train_sampler(num_training_sample=6)
    got = [s.draw(), s.draw()]
    torch.manual_seed(4)
    subset = torch.randperm(13)[:6]
    ref = SubsetRandomSampler(subset)
    assert s.kind == 'few_shot' and np.array_equal(s.classes[0], subset.numpy()) and len(s) == 6
    assert all(np.array_equal(g, np.asarray([int(i) for i in ref])) for g in got)
    assert not np.array_equal(got[0], got[1]) and sorted(got[0]) == sorted(subset.tolist())


def test_generator_feeds_every_draw():
    """A generator given to the loader, or to train_sampler, replaces torch's global one: two samplers
    with generators in the same state draw the same orders, whatever the global state."""
    a = _loader(generator=torch.Generator().manual_seed(7)).train_sampler(num_training_sample=6)
    torch.manual_seed(123)
    b = _loader().train_sampler(num_training_sample=6, generator=torch.Generator().manual_seed(7))
    assert np.array_equal(a.classes[0], b.classes[0])
    assert all(np.array_equal(a.draw(), b.draw()) for _ in range(2))


def test_dp_plan_follows_the_samplers_length(loader):
    from a2m.data import dp_plan
    s = loader.train_sampler(quantile_sample=3, quantile_num_training_sample=3, velocity=VEL)
    assert len(s) == 12
    odd = loader.train_sampler(num_training_sample=7)
    for smp in (s, odd):
        order = smp.draw()
        plans = [dp_plan(len(smp), 4, r, 2)[0] for r in range(2)]
        whole = dp_plan(len(smp), 4, 0, 1)[0]
        assert len(plans[0]) == len(plans[1])
        k = 0
        for (b0, n) in whole:
            m = n // 2
            if not m:
                continue
            rows = [order[p[k][0]:p[k][0] + p[k][1]] for p in plans]
            assert np.array_equal(np.concatenate(rows), order[b0:b0 + 2 * m])
            k += 1
        assert k == len(plans[0])
    assert len(loader.pairs('train', sampler=s)) == 3 and len(loader.pairs('train', sampler=odd)) == 2
    assert len(loader.sampled('train', odd)) == 2
    two = _loader(rank=1, world=2)
    assert len(two.pairs('train', sampler=two.train_sampler(num_training_sample=7))) == 2   # 4 -> 2 rows, 3 -> 1 row
