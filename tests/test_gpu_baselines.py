"""The evaluation baselines on the device (csrc/baselines.hip, a2m/baselines.py) against
tests/baselines_ref.py.

Median: equality (==, so -0.0 and +0.0 agree) with np.median on the value families of
test_baselines_ref_cpu.py laid into an arena with overlapping windows, a table range that starts at
lo > 0 and canary rows of +-1e30 everywhere the kernel must not read.

Search, exact: integer-valued floats in [-3, 3] at the flagship window (T = 64, C = 128): every
product and partial sum is an integer below T*C*36 < 2^24, exact in fp32 under any summation order, so
best_dist and the lowest-index argmin must equal the integer reference exactly.

Search, floats: K = T*C; |q|^2, |w|^2 and q.w are each an fp32 sum of K terms (an fma chain, or chains
and a tree), so each is within K 2^-24 of the sum of its terms' magnitudes, and with
|q.w| <= sum |q w| <= (|q|^2 + |w|^2) / 2 the computed (|q|^2 + |w|^2) - 2 q.w is within
tol(b, p) = 4 K 2^-24 (|q_b|^2 + |w_p|^2) of the exact distance, two final roundings included."""
import numpy as np
import pytest
import torch

import baselines_ref as R
import pats_data_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
FAMILIES = ['normal', 'equal', 'duplicates', 'zeros', 'signed_zero', 'denormal', 'low_byte', 'wide']


def _np(t):
    return t.detach().cpu().numpy()


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _windows(arena, start, window, interval):
    """[len(start), T, C]: arena[s : s + window : interval] of every start."""
    return np.stack([arena[s:s + window:interval] for s in start])


# ------------------------------------------------------------------------------ the median
MEDIAN_SHAPES = [(1, 1, 1, 4, False), (1, 2, 1, 4, False), (3, 5, 2, 4, False), (7, 9, 3, 8, False),
                 (5, 64, 1, 104, False), (5, 64, 1, 104, True), (40, 382, 6, 104, True)]


def _median_case(n, window, interval, C, seed=0):
    """An arena whose read rows hold one value family per channel and whose every other row (before and
    after the windows, and between the rows of a window when interval > 1: the hop is a multiple of the
    interval) is a +-1e30 canary; overlapping windows; a table with lo = 3 whose entries outside
    [lo, lo + n) point at canary rows."""
    lo, pad = 3, 5
    T = (window + interval - 1) // interval
    hop = interval * max(1, T // 3)
    rows = pad + (n - 1) * hop + window + pad
    arena = np.where(np.arange(rows)[:, None] % 2 == 0, np.float32(1e30), np.float32(-1e30)) * np.ones((1, C), np.float32)
    arena = arena.astype(np.float32)
    start = pad + hop * np.arange(n, dtype=np.int64)
    read = np.unique((start[:, None] + interval * np.arange(T)[None]).reshape(-1))
    fam = R.value_families(len(read), seed)
    for c in range(C):
        arena[read, c] = fam[FAMILIES[c % len(FAMILIES)]]
    table = np.concatenate([np.array([0, rows - window, 1], np.int64), start, np.array([0, 2], np.int64)])
    return arena, table, lo


@pytest.mark.parametrize('n,window,interval,C,necksub', MEDIAN_SHAPES)
def test_window_median_is_numpy_median(n, window, interval, C, necksub):
    from a2m import functional as F
    arena, table, lo = _median_case(n, window, interval, C)
    pop = _windows(arena, table[lo:lo + n], window, interval).reshape(-1, C)
    assert pop.shape[0] == n * ((window + interval - 1) // interval) and np.abs(pop).max() < 1e30
    if necksub:
        pop = P.necksub(pop)
    ref = R.median(pop)
    a, t = _dev(arena, table)
    got = _np(F.window_median(a, t, lo, n, window, interval, necksub=necksub))
    assert got.dtype == np.float32 and got.shape == (C,)
    assert np.array_equal(got, ref), (np.flatnonzero(got != ref), got[got != ref], ref[got != ref])
    if necksub:
        assert got[0] == 0 and got[52] == 0
    if n * ((window + interval - 1) // interval) <= 64:      # the select's own restatement, where it is cheap
        assert all(R.radix_select_median(pop[:, c]) == got[c] for c in range(C))


# ------------------------------------------------------------------------------ the search, exact
WINDOW, INTERVAL, T, C = 382, 6, 64, 128
LO, NMAX, BMAX, HOP = 4, 257, 65, 7
DUP_NEAR, DUP_FAR = (5, 9), (20, 230)          # equal start entries: within one 64-tile, and 210 apart
_EXACT = {}


def _exact_case(standardise):
    """One arena, table and query set per mode, shared by every (n_cand, B): the candidates of a case are
    the first n_cand table entries after LO and its queries the first B.  Returns (device tensors, the
    float64 distances [BMAX, NMAX])."""
    if standardise in _EXACT:
        return _EXACT[standardise]
    g = np.random.default_rng(17 + standardise)
    rows = 3 + (NMAX - 1) * HOP + WINDOW
    v = g.integers(-3, 4, (rows, C)).astype(np.float32)          # the values the distances are taken over
    mean = g.integers(-2, 3, C).astype(np.float32)
    std = (2.0 ** g.integers(-1, 3, C)).astype(np.float32)
    arena = (v * std + mean).astype(np.float32) if standardise else v
    if standardise:
        assert np.array_equal(P.standardise(arena, mean, std), v)
    start = 3 + HOP * np.arange(NMAX, dtype=np.int64)
    start[DUP_NEAR[1]], start[DUP_FAR[1]] = start[DUP_NEAR[0]], start[DUP_FAR[0]]
    table = np.concatenate([np.zeros(LO, np.int64), start, np.zeros(2, np.int64)])
    wins = _windows(v, start, WINDOW, INTERVAL)
    query = g.integers(-3, 4, (BMAX, T, C)).astype(np.float32)
    query[0], query[1] = wins[DUP_NEAR[0]], wins[DUP_FAR[0]]
    query[64] = wins[DUP_FAR[1]]                                 # a planted query in the second query tile
    d = R.nn_distances(query, wins)
    assert d.max() < 2 ** 24 and np.array_equal(d, np.round(d))
    dev = _dev(arena, table, query) + (_dev(mean, std) if standardise else [None, None])
    _EXACT[standardise] = dev, d
    return _EXACT[standardise]


@pytest.mark.parametrize('standardise', [0, 1], ids=['raw', 'standardise'])
@pytest.mark.parametrize('B', [1, 3, 65])
@pytest.mark.parametrize('n_cand', [1, 63, 64, 65, 257])
def test_nn_search_exact_on_integers(n_cand, B, standardise):
    from a2m import functional as F
    (arena, table, query, mean, std), d = _exact_case(standardise)
    best, dist = F.nn_search(query[:B], arena, table, LO, n_cand, WINDOW, INTERVAL, mean, std)
    best, dist = _np(best), _np(dist)
    assert best.dtype == np.int64 and dist.dtype == np.float32
    ref = d[:B, :n_cand]
    assert np.array_equal(best, LO + ref.argmin(1))              # np.argmin: the lowest index among equals
    assert np.array_equal(dist.astype(np.float64), ref.min(1))
    if n_cand > DUP_NEAR[1]:
        assert best[0] == LO + DUP_NEAR[0] and dist[0] == 0
    if n_cand > DUP_FAR[1] and B > 1:
        assert best[1] == LO + DUP_FAR[0] and dist[1] == 0
    if n_cand > DUP_FAR[1] and B > 64:
        assert best[64] == LO + DUP_FAR[0] and dist[64] == 0


# ------------------------------------------------------------------------------ the search, floats
FLOAT_SHAPES = [(1, 1, 4), (5, 2, 4), (9, 2, 8), (382, 6, 128)]      # (window, interval, C): (T, C) = (1,4) (3,4) (5,8) (64,128)


@pytest.mark.parametrize('standardise', [0, 1], ids=['raw', 'standardise'])
@pytest.mark.parametrize('window,interval,C', FLOAT_SHAPES)
def test_nn_search_floats_within_the_sum_bound(window, interval, C, standardise):
    from a2m import functional as F
    Tn = (window + interval - 1) // interval
    K = Tn * C
    n_cand, B, lo, hop = 150, 70 if K < 1000 else 9, 2, max(1, window // 2)
    planted = [0, 63, 64, 149][:B]
    g = np.random.default_rng(1000 * K + standardise)
    rows = (n_cand - 1) * hop + window
    arena = g.standard_normal((rows, C)).astype(np.float32)
    mean, std = g.standard_normal(C).astype(np.float32), (g.random(C) * 2 + 0.5).astype(np.float32)
    std[1] = 1e-8                                                  # below the guard: divides by 1
    start = hop * np.arange(n_cand, dtype=np.int64)
    table = np.concatenate([np.zeros(lo, np.int64), start, np.zeros(1, np.int64)])
    wins = _windows(P.standardise(arena, mean, std) if standardise else arena, start, window, interval)
    query = g.standard_normal((B, Tn, C)).astype(np.float32)
    for b, p in enumerate(planted):
        query[b] = wins[p] + np.float32(0.05) * g.standard_normal((Tn, C)).astype(np.float32)
    d = R.nn_distances(query, wins)
    tol = 4 * K * 2.0 ** -24 * (R.sq_norms(query)[:, None] + R.sq_norms(wins)[None, :])
    for b, p in enumerate(planted):                                # on the reference alone: the plant is decidable
        others = np.delete(d[b], p)
        assert d[b].argmin() == p and others.min() > d[b, p] + 8 * tol[b].max()
    a, t, q, m, s = _dev(arena, table, query, mean, std)
    best, dist = F.nn_search(q, a, t, lo, n_cand, window, interval, *((m, s) if standardise else (None, None)))
    best, dist = _np(best) - lo, _np(dist).astype(np.float64)
    assert best.min() >= 0 and best.max() < n_cand and dist.min() >= 0
    rows_b = np.arange(B)
    err = np.abs(dist - d[rows_b, best])
    print(f'NN floats T={Tn} C={C} standardise={standardise}: worst err / tol = {(err / tol[rows_b, best]).max():.3e}')
    assert np.all(err <= tol[rows_b, best])
    assert np.all(d[rows_b, best] <= d.min(1) + tol[rows_b, best] + tol[rows_b, d.argmin(1)])
    assert np.array_equal(best[:len(planted)], planted)


# ------------------------------------------------------------------------------ the modules
ARR = P.arrays()
SPEAKERS = ['seth', 'oliver']
N_TRAIN = 13


def _loader(datasets=('train',) * 4, **kw):
    from a2m.data import PatsLoader
    table = [P.row(d, i, 'oliver' if i in 'AB' else 'seth') for d, i in zip(datasets, 'ABCD')]
    kw.setdefault('batch_size', 4)
    return PatsLoader(ARR, table, SPEAKERS, time=P.TIME, fs_new=P.FS_NEW, window_hop=5, shuffle=False, device=DEV, **kw)


def _stats(seed=11):
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    asd[5] = 1e-8
    return _dev(pm, ps, am, asd)


@pytest.mark.parametrize('standardise', [False, True], ids=['raw', 'standardise'])
def test_nearest_audio_finds_every_clip_itself(standardise):
    from a2m.baselines import NearestAudio
    loader = _loader()
    pm, ps, am, asd = _stats()
    audio_stats = (am, asd) if standardise else (None, None)
    model = NearestAudio(loader, pm, ps, *audio_stats)
    seen = 0
    for audio, pose in loader.pairs('train', pm, ps, *audio_stats):
        out, extra = model(audio)
        n = audio.shape[0]
        assert extra is None and torch.equal(model.last_index, torch.arange(seen, seen + n, device=DEV))
        assert torch.equal(out, pose) and model.last_distance.shape == (n,)
        assert float(model.last_distance.max()) <= 4 * 8192 * 2.0 ** -24 * 2 * float((audio * audio).sum((1, 2)).max())
        seen += n
    assert seen == N_TRAIN


def test_random_clip_is_the_drawn_clips_and_repeats():
    from a2m.baselines import RandomClip
    loader = _loader()
    pm, ps, _, _ = _stats()
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    model = RandomClip(loader, pm, ps, generator=gen)
    audio = torch.zeros(6, 64, 128, device=DEV)
    out, extra = model(audio)
    idx = model.last_index.clone()
    assert extra is None and idx.dtype == torch.int64 and int(idx.min()) >= 0 and int(idx.max()) < N_TRAIN
    ref = torch.cat([p for _, p in loader.pairs('train', pm, ps, order=idx.cpu(), copy=True)])
    assert torch.equal(out, ref)
    assert len(set(idx.tolist())) > 1
    gen.manual_seed(5)
    again, _ = model(audio)
    assert torch.equal(model.last_index, idx) and torch.equal(again, out)


def test_median_pose_is_the_numpy_median():
    from a2m.baselines import MedianPose
    loader = _loader()
    pm, ps, _, _ = _stats()
    model = MedianPose(loader, pm, ps)
    smp = P.samples('ABCD', 5)
    pop = P.necksub(P.stack(ARR, smp, np.arange(N_TRAIN), P.POSE, 5)).reshape(-1, 104)
    ref = R.median(pop)
    assert np.array_equal(_np(model.median_px), ref)
    out, extra = model(torch.zeros(3, 64, 128, device=DEV))
    norm = (ref - _np(pm)) / _np(ps)
    assert extra is None and out.shape == (3, 64, 104) and out.is_contiguous()
    assert np.array_equal(_np(out), np.broadcast_to(norm, (3, 64, 104)))


def test_evaluate_takes_the_baselines():
    """evaluate() on NearestAudio over the split it was built from reproduces the clips: pck 1 and an L1
    of the few ulp (of pixel values of order 1e2 - 1e3) that normalising and de-normalising cost; and
    evaluate_baselines returns the three results, the median's L1 that of the broadcast median."""
    from a2m.baselines import NearestAudio, evaluate_baselines
    from a2m.evaluation import METRICS, evaluate
    loader = _loader()
    pm, ps, am, asd = _stats()
    res = evaluate(NearestAudio(loader, pm, ps, am, asd), loader, 'train', pose_mean=pm, pose_std=ps, audio_mean=am,
                   audio_std=asd)
    print(f"BASELINES nearest on its own split: pck {res['all']['pck']}, l1 {res['all']['l1']:.3e}")
    assert res['all']['pck'] == 1.0 and res['all']['l1'] < 1e-2 and res['all']['n_clips'] == N_TRAIN
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1)
    three = evaluate_baselines(loader, 'train', pose_mean=pm, pose_std=ps, audio_mean=am, audio_std=asd, generator=gen)
    assert sorted(three) == ['median', 'nearest', 'random']
    assert all(sorted(r['all']) == sorted(METRICS) for r in three.values())
    assert three['nearest']['all']['l1'] == res['all']['l1']
    smp = P.samples('ABCD', 5)
    real = P.necksub(P.stack(ARR, smp, np.arange(N_TRAIN), P.POSE, 5)).astype(np.float64)
    med = R.median(real.reshape(-1, 104)).astype(np.float64)
    l1 = np.abs(real - med).mean()
    assert abs(three['median']['all']['l1'] - l1) <= 1e-4 * l1
    assert three['median']['all']['l1'] < three['random']['all']['l1']


def test_nearest_audio_captures_and_follows_the_query():
    from a2m.baselines import NearestAudio
    loader = _loader()
    pm, ps, am, asd = _stats()
    model = NearestAudio(loader, pm, ps, am, asd)
    batches = [(a, p) for a, p in loader.pairs('train', pm, ps, am, asd, copy=True)]
    query = batches[0][0].clone()
    eager, _ = model(query)
    assert torch.equal(eager, batches[0][1])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, _ = model(query)
        index = model.last_index
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, batches[0][1]) and torch.equal(index, torch.arange(4, device=DEV))
    query.copy_(batches[2][0])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, batches[2][1]) and torch.equal(index, torch.arange(8, 12, device=DEV))


def test_forwards_do_not_synchronise():
    """The three forwards under torch's sync debug mode 'error', as tests/test_gpu_data.py checks the
    loader's pass, after a first call has created the code objects."""
    from a2m.baselines import MedianPose, NearestAudio, RandomClip
    loader = _loader()
    pm, ps, am, asd = _stats()
    gen = torch.Generator(device=DEV)
    models = [MedianPose(loader, pm, ps), RandomClip(loader, pm, ps, generator=gen), NearestAudio(loader, pm, ps, am, asd)]
    audio, pose = next(iter(loader.pairs('train', pm, ps, am, asd, copy=True)))
    for m in models:
        m(audio)
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
            outs = [m(audio)[0] for m in models]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("the installed ROCm torch does not honour torch.cuda.set_sync_debug_mode('error')")
    assert torch.equal(outs[2], pose) and all(o.shape == pose.shape for o in outs)
