"""The train samplers on the device (csrc/sampling.hip, a2m/sampling.py) against the float64
statements of tests/sampling_ref.py: the clip velocity, the radix select and the classification
kernel at the shapes where their indexing can go wrong, then PatsLoader.train_sampler end to end
and passes of pairs(..., sampler=) / sampled().

Velocity bound, 1e-6 relative: every term carries at most about three fp32 roundings (the two
differences, the sum of squares, the root), under 2e-7 relative; the float64 sum of the positive
terms adds nothing to that; the one rounding of the mean to float adds 6e-8.  1e-6 leaves a factor
of four, contraction of the sum of squares to an FMA included.  Select and classify are exact."""
import numpy as np
import pytest
import torch

import pats_data_ref as P
import sampling_ref as S
from test_gpu_validate import _trainer

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
ARR = S.arrays()
IDS = list('ABCD')
SPEAKERS = ['seth', 'oliver']            # A, B speak as 'oliver' (style 1), C, D as 'seth' (style 0)
STYLE = {'A': 1, 'B': 1, 'C': 0, 'D': 0}
VEL = S.clip_velocities(ARR, IDS, 5)     # float64 [13]


def _np(t):
    return t.detach().cpu().numpy()


def _table(datasets=('train',) * 4, ids=IDS):
    return [P.row(d, i, 'oliver' if i in 'AB' else 'seth') for d, i in zip(datasets, ids)]


def _loader(hop=5, shuffle=True, **kw):
    from a2m.data import PatsLoader
    kw.setdefault('table', _table())
    kw.setdefault('batch_size', 4)
    return PatsLoader(kw.pop('arrays', ARR), speaker=SPEAKERS, time=P.TIME, fs_new=P.FS_NEW, window_hop=hop,
                      shuffle=shuffle, device=DEV, **kw)


def _stats(seed=11):
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    return [torch.from_numpy(x).to(DEV) for x in (pm, ps, am, asd)]


# ------------------------------------------------------------------------------ velocity
@pytest.mark.parametrize('hop', [5, 0])
def test_loader_velocity_matches_float64(hop):
    loader = _loader(hop)
    vel = loader.clip_velocity('train')
    want = S.clip_velocities(ARR, IDS, hop)
    assert vel.is_cuda and vel.dtype == torch.float32 and vel.shape == (sum(P.COUNTS[hop]),)
    err = np.abs(_np(vel) - want) / want
    print(f'SAMPLING velocity hop {hop}: max rel err {err.max():.3e}')
    assert err.max() <= 1e-6
    assert loader.clip_velocity('train') is vel                         # cached
    assert int(loader._velocity_bad['train'].item()) == 0
    assert loader.clip_velocity('dev').shape == (0,)
    loader.update_dataloaders(P.TIME, 5 - hop)                          # drops the cache
    again = loader.clip_velocity('train')
    assert again.shape == (sum(P.COUNTS[5 - hop]),)
    assert np.abs(_np(again) - S.clip_velocities(ARR, IDS, 5 - hop)).max() <= 1e-6 * want.max()


# (C, window, interval, n, lo): rows that are not contiguous, two frames, table offsets, and n around
# the wave, the workgroup (4 clips) and the XCD remap (8 workgroups)
DIRECT = [(6, 13, 3, 65, 0), (104, 2, 1, 63, 0), (104, 64, 1, 1, 0), (104, 64, 1, 64, 3), (96, 64, 1, 257, 2),
          (4, 5, 2, 33, 1), (104, 382, 6, 5, 0)]


@pytest.mark.parametrize('C,window,interval,n,lo', DIRECT)
def test_velocity_direct(C, window, interval, n, lo):
    """The wrapper on a small arena: random start rows, the last clip ending on the arena's last row,
    the float64 statement within 1e-6, two runs byte-identical, no non-finite clip counted."""
    from a2m import functional as F
    g = np.random.default_rng(C * 1000 + n)
    T = -(-window // interval)
    span = (T - 1) * interval + 1                                       # rows from a clip's first to its last
    rows = span + 150
    arena = (300 + np.cumsum(g.standard_normal((rows, C)) * g.uniform(0.1, 4, (rows, 1)), 0)).astype(np.float32)
    start = g.integers(0, rows - span + 1, lo + n)
    start[-1] = rows - span
    out, bad = F.clip_velocity(torch.from_numpy(arena).to(DEV), torch.from_numpy(start).to(DEV), lo, n, window,
                               interval)
    out2, _ = F.clip_velocity(torch.from_numpy(arena).to(DEV), torch.from_numpy(start).to(DEV), lo, n, window,
                              interval)
    want = S.table_velocity(arena, start[lo:], window, interval)
    assert arena[start[-1]:start[-1] + window:interval].shape[0] == T and start[-1] + span == rows
    err = np.abs(_np(out) - want) / want
    print(f'SAMPLING velocity C={C} window={window}/{interval} n={n} lo={lo}: max rel err {err.max():.3e}')
    assert out.shape == (n,) and err.max() <= 1e-6
    assert torch.equal(out, out2) and int(bad.item()) == 0


def test_velocity_counts_a_nan_clip():
    from a2m import functional as F
    g = np.random.default_rng(3)
    arena = (300 + np.cumsum(g.standard_normal((64 * 6, 104)), 0)).astype(np.float32)
    start = np.arange(6) * 64                                           # clips that share no row
    clean = S.table_velocity(arena, start, 64, 1)
    arena[2 * 64 + 17] = np.nan
    out, bad = F.clip_velocity(torch.from_numpy(arena).to(DEV), torch.from_numpy(start).to(DEV), 0, 6, 64, 1)
    got = _np(out)
    assert int(bad.item()) == 1 and not np.isfinite(got[2])
    keep = [0, 1, 3, 4, 5]
    assert np.isfinite(got[keep]).all() and (np.abs(got[keep] - clean[keep]) / clean[keep]).max() <= 1e-6
    with pytest.raises(ValueError, match='clip_velocity'):
        F.clip_velocity(torch.from_numpy(arena[:, :103].copy()).to(DEV), torch.from_numpy(start).to(DEV), 0, 6, 64, 1)


# ------------------------------------------------------------------------------ select
def _values(kind, n):
    g = np.random.default_rng(n)
    if kind == 'random':
        return np.abs(g.standard_normal(n) * 3).astype(np.float32)
    if kind == 'equal':
        return np.full(n, 2.5, np.float32)
    if kind == 'ties':
        return np.round(g.random(n) * 2).astype(np.float32) * np.float32(1.25)      # 0, 1.25, 2.5
    tiny = np.array([0.0, 1e-45, 3e-45, 1e-40, 1.1754942e-38, 1.17549435e-38, 1e-30, 1.0], np.float32)
    return tiny[g.integers(0, len(tiny), n)]


SELECT = [('random', n) for n in (1, 2, 255, 256, 257, 70001)] + [('equal', 257), ('ties', 1000), ('tiny', 513)]


@pytest.mark.parametrize('kind,n', SELECT)
def test_select_is_the_sorted_element(kind, n):
    from a2m import functional as F
    x = _values(kind, n)
    assert (x >= 0).all() and not np.signbit(x).any()
    ranks = [0, n - 1, n // 2, n // 2]
    out, minmax = F.select(torch.from_numpy(x).to(DEV), ranks)
    ordered = np.sort(x)
    assert np.array_equal(_np(out).view(np.uint32), ordered[ranks].view(np.uint32))
    assert np.array_equal(_np(minmax).view(np.uint32), ordered[[0, -1]].view(np.uint32))
    if kind == 'tiny':
        assert (x == 0).any() and ((x > 0) & (x < 1.17549435e-38)).any()        # zeros and subnormals are there
    if n == 257:
        eight, _ = F.select(torch.from_numpy(x).to(DEV), [256, 0, 1, 128, 255, 7, 7, 200])
        assert np.array_equal(_np(eight), ordered[[256, 0, 1, 128, 255, 7, 7, 200]])
        with pytest.raises(ValueError, match='select'):
            F.select(torch.from_numpy(x).to(DEV), [257])


# ------------------------------------------------------------------------------ classify
@pytest.mark.parametrize('n', [1, 70001])
def test_classify_equals_numpy(n):
    """Values drawn from a small set that holds every threshold and edge exactly (all of them float32
    numbers, so the float64 comparison sees equality), values off them, and values outside."""
    from a2m import functional as F
    g = np.random.default_rng(n)
    edges = [0.5, 1.25, 1.25 + 2 ** -20, 3.0, 7.75]                    # first, inner (one a float32 ulp-ish step on), last
    pool = np.array(edges + [0.25, 0.5 - 2 ** -25, 0.75, 1.25 + 2 ** -21, 2.0, 5.0, 7.75 + 2 ** -21, 9.0], np.float32)
    x = pool[g.integers(0, len(pool), n)] if n > 1 else np.array([1.25], np.float32)
    xd = torch.from_numpy(x).to(DEV)
    v = x.astype(np.float64)
    cases = [('above', [1.25], np.where(v > 1.25, 0, -1)),
             ('above', [1.25 + 2 ** -40], np.where(v > 1.25 + 2 ** -40, 0, -1)),          # not a float32 number
             ('tail', [1.25, 3.0], np.where((v > 3.0) | (v < 1.25), 0, -1)),
             ('bins', edges, S.bins_of(v, edges))]
    for kind, thr, want in cases:
        cls, counts = F.classify(xd, kind, thr)
        assert cls.dtype == torch.int32 and counts.dtype == torch.int64
        assert np.array_equal(_np(cls), want.astype(np.int32)), (kind, thr)
        n_cls = len(thr) - 1 if kind == 'bins' else 1
        assert _np(counts).tolist() == [int((want == c).sum()) for c in range(n_cls)], (kind, thr)
    if n > 1:
        on_inner = S.bins_of(np.array([1.25, 1.25 + 2 ** -20, 3.0, 0.5, 7.75]), edges)
        assert on_inner.tolist() == [0, 1, 2, 0, 3]                     # an inner edge: the lower bin; both ends closed
        assert {-1, 0, 1, 2, 3} == set(S.bins_of(v, edges).tolist())


# ------------------------------------------------------------------------------ end to end
@pytest.fixture(scope='module')
def loader():
    return _loader()


@pytest.mark.parametrize('q', [0.4, 0.5, 0.9])
def test_quantile_sampler_selects_the_float64_subset(loader, q):
    thr = S.quantile(VEL, q)
    if q != 0.5:
        assert np.abs(VEL - thr).min() > 1e-5 * thr                    # fp32 velocities cannot cross the threshold
    s = loader.train_sampler(quantile_sample=q)
    assert s.kind == 'above' and np.array_equal(s.classes[0], S.above(VEL, q))
    assert abs(s.thresholds[0] - thr) <= 2e-6 * thr
    host = loader.train_sampler(quantile_sample=q, velocity=_np(loader.clip_velocity('train')))
    assert np.array_equal(host.classes[0], s.classes[0]) and host.thresholds == s.thresholds
    tail = loader.train_sampler(quantile_sample=[0.25, 0.9])
    assert tail.kind == 'tail' and np.array_equal(tail.classes[0], S.tail(VEL, 0.25, 0.9))


def test_rebalance_sampler_gives_the_float64_classes(loader):
    s = loader.train_sampler(quantile_sample=3, quantile_num_training_sample=2)
    want = S.rebalance(VEL, 3)
    assert [len(c) for c in want] == [1, 4, 8]
    assert s.kind == 'rebalance' and len(s.classes) == 3 and all(np.array_equal(a, b) for a, b in zip(s.classes, want))
    assert len(s) == (2 * 4 // 3) * 3 == 6
    eight = loader.train_sampler(quantile_sample=8, quantile_num_training_sample=2)
    assert all(np.array_equal(a, b) for a, b in zip(eight.classes, S.rebalance(VEL, 8))) and len(eight.classes) < 8


def test_non_finite_velocity_is_refused():
    arr = {i: {m: a.copy() for m, a in mods.items()} for i, mods in ARR.items()}
    arr['D'][P.POSE][30, 7] = np.inf
    with pytest.raises(ValueError, match='of the 13 clips of train have a non-finite velocity'):
        _loader(arrays=arr).train_sampler(quantile_sample=0.5)


@pytest.mark.parametrize('batch_size', [4, 5])
def test_sampled_pairs_are_the_ordered_pairs(batch_size):
    """Every batch of pairs(..., sampler=s) is bitwise the batch pairs(..., order=that pass's order)
    yields, over two passes, and holds only clips of the subset; sampled() gives the same pass as
    the batch dict."""
    loader = _loader(batch_size=batch_size)
    stats = _stats()
    s = loader.train_sampler(quantile_sample=0.4)
    subset = set(S.above(VEL, 0.4).tolist())
    assert len(s) == 8
    view = loader.pairs('train', *stats, sampler=s, copy=True)
    assert len(view) == -(-8 // batch_size)
    smp = P.samples(IDS, 5)
    for seed in (0, 1):
        torch.manual_seed(seed)
        got = list(view)
        torch.manual_seed(seed)
        order = s.draw()
        assert set(order.tolist()) == subset and len(order) == 8
        want = list(loader.pairs('train', *stats, order=order, copy=True))
        assert [a.shape[0] for a, _ in got] == [len(order[k:k + batch_size]) for k in range(0, 8, batch_size)]
        assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(got, want)) and len(got) == len(want)
        raw = list(loader.pairs('train', sampler=s, copy=True)) if seed == 0 else None
        torch.manual_seed(seed)
        dicts = list(loader.sampled('train', s))
        assert len(dicts) == len(got) == len(loader.sampled('train', s))
        for k, batch in enumerate(dicts):
            idx = order[k * batch_size:(k + 1) * batch_size]
            assert np.array_equal(_np(batch['idx']), idx)
            assert np.array_equal(_np(batch[P.POSE]), P.stack(ARR, smp, idx, P.POSE, 5))
            assert np.array_equal(_np(batch[P.AUDIO]), P.stack(ARR, smp, idx, P.AUDIO, 5))
            assert np.array_equal(_np(batch['style'])[:, 0], [STYLE[smp[i][0]] for i in idx])
            assert batch['meta']['interval_id'] == [smp[i][0] for i in idx]
            assert batch['meta']['idx'].tolist() == [smp[i][1] for i in idx]
        assert raw is None or all(a.shape[1:] == (64, 128) and p.shape[1:] == (64, 104) for a, p in raw)


def test_augment_and_style_follow_the_order(loader):
    from a2m.data import Augment
    stats = _stats()
    s = loader.train_sampler(quantile_sample=3, quantile_num_training_sample=3)
    smp = P.samples(IDS, 5)
    view = loader.pairs('train', *stats, sampler=s, copy=True, with_style=True,
                        augment=Augment(seed=1, p_mirror=0.5, speed=0.1, gain=0.5))
    torch.manual_seed(8)
    got = list(view)
    torch.manual_seed(8)
    order = s.draw()
    assert len(order) == 12 and [a.shape[0] for a, _, _ in got] == [4, 4, 4]
    for k, (audio, pose, style) in enumerate(got):
        assert audio.shape == (4, 64, 128) and pose.shape == (4, 64, 104) and style.dtype == torch.int32
        assert _np(style).tolist() == [STYLE[smp[i][0]] for i in order[4 * k:4 * k + 4]]
        assert torch.isfinite(audio).all() and torch.isfinite(pose).all()
    plain = list(loader.pairs('train', *stats, order=order, copy=True, with_style=True,
                              augment=Augment(seed=1, p_mirror=0.5, speed=0.1, gain=0.5)))
    assert all(torch.equal(a, b) for x, y in zip(got, plain) for a, b in zip(x, y))


def test_two_ranks_take_disjoint_halves():
    def gen():
        return torch.Generator().manual_seed(3)

    whole = _loader(generator=gen())
    ranks = [_loader(generator=gen(), rank=r, world=2) for r in range(2)]
    stats = _stats()
    samplers = [ld.train_sampler(num_training_iters=3) for ld in [whole] + ranks]           # 12 draws: 3 batches of 4
    views = [ld.pairs('train', *stats, sampler=s, copy=True) for ld, s in zip([whole] + ranks, samplers)]
    assert [len(v) for v in views] == [3, 3, 3]
    for _ in range(2):                                                  # the generators advance alike
        full, r0, r1 = (list(v) for v in views)
        for k in range(3):
            assert r0[k][0].shape[0] == r1[k][0].shape[0] == 2
            for j in range(2):
                assert torch.equal(torch.cat([r0[k][j], r1[k][j]]), full[k][j])


def test_sampled_pass_does_not_synchronise(loader):
    stats = _stats()
    s = loader.train_sampler(quantile_sample=[0.25, 0.9])
    pairs = loader.pairs('train', *stats, sampler=s)
    assert sum(1 for _ in pairs) == 2                      # buffers and the kernel's code object exist from here on
    torch.manual_seed(0)
    it = iter(pairs)                                       # the draw and the one upload
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            seen = [(a, p) for a, p in it]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("the installed ROCm torch does not honour torch.cuda.set_sync_debug_mode('error')")
    assert [a.shape[0] for a, _ in seen] == [4, 1]
    torch.manual_seed(0)
    order = s.draw()
    want = list(loader.pairs('train', *stats, order=order, copy=True))
    assert torch.equal(seen[1][1], want[1][1]) and torch.equal(seen[0][0], want[0][0])


def test_sampled_pass_captures_into_a_graph(loader):
    """A whole pass (two gathers) recorded after iter(): the replay writes the eager pass's bytes."""
    stats = _stats()
    s = loader.train_sampler(quantile_sample=[0.25, 0.9])
    pairs = loader.pairs('train', *stats, sampler=s)
    torch.manual_seed(4)
    eager = [(a.clone(), p.clone()) for a, p in pairs]
    torch.manual_seed(4)
    it = iter(pairs)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        kept = [(a.clone(), p.clone()) for a, p in it]
    for a, p in kept:
        a.zero_()
        p.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(kept) == len(eager) == 2
    assert all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(kept, eager))


def test_fit_runs_on_a_sampled_view():
    """A, D in train and C in dev at batch size 2: one epoch of two train batches drawn by the
    fixed-iterations sampler; every epoch's iter() is a new draw."""
    from a2m import normalization as NZ
    loader = _loader(table=_table(('train', 'train', 'dev', 'train')), batch_size=2)
    m, sd = NZ.get_mean_std_necksub(loader)
    s = loader.train_sampler(num_training_iters=2)
    view = loader.pairs('train', m, sd, sampler=s)
    assert len(view) == 2
    rec = _trainer().fit(view, loader.pairs('dev', m, sd), 1, log_every=1, log=lambda s: None)
    assert len(rec['train_g']) == 2 and len(rec['val_terms']) == 1
    assert all(np.isfinite(v) for v in rec['train_g'] + rec['train_d'] + rec['val_g'] + rec['val_d'])
