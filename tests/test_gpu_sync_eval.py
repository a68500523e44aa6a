"""The audio-motion synchrony metrics on the device: csrc/pose_eval.hip's eval_sync and eval_sync_finish
kernels against tests/sync_ref.py (float64 numpy), and a2m.evaluation.AudioSyncEvaluator /
evaluate(..., sync=True) on the real generator and a synthetic PatsLoader.

Integers (beat distance histograms, beat counts, pair counts) are compared for equality.  Both sides decide
a beat in float64 from the same float32 values, a few ulps of float64 apart, so the random inputs keep every
beat comparison 1e-9 relative clear of a tie in the reference alone (sync_ref.random_case; asserted on the
CPU in test_sync_ref_cpu.py), and the tie cases use inputs whose onsets and speeds are exact in any order.

The lag sums pass within eval_ref.sum_tol(n_terms + C + 2K, sum |terms|): the outer sum of n terms costs
n u, each term carries at most about (C + 2K) u from the sums inside its onset and its speed, and sum_tol's
factor 8 covers the roundings inside a term.  The per-frame series pass within 8 (C + 2K) u |value|
(sync_ref.series_tol).  Both bounds are derived, not measured."""
import functools

import numpy as np
import pytest
import torch

import pats_data_ref as P
import sync_ref as S
from test_gpu_configs import _models

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

N_STYLES = S.N_STYLES
CANARY = -7777.25
ICANARY = -7777


def _mid(shape):
    return 'x'.join(str(s) for s in shape)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape):
    return S.random_case(shape)


def _padded(shape, dtype):
    """A canary-filled buffer with the zeroed accumulator as a view of its head."""
    n = int(np.prod(shape))
    buf = torch.full((n + 64,), ICANARY if dtype == torch.int64 else CANARY, dtype=dtype, device=DEV)
    return buf, buf[:n].view(shape)


def _run(audio, fake, real, style, std=None, n_styles=N_STYLES, n_lags=4, n_dist=32, onset_delta=1.0):
    """Both launches on zeroed accumulators inside canary-filled buffers; everything back on the host."""
    from a2m import functional as F
    B, T, _ = audio.shape
    L = 2 * n_lags + 1
    shapes = dict(beat_dist=((n_styles, 2, 2, n_dist), torch.int64), beat_counts=((n_styles, 3), torch.int64),
                  lag_sums=((n_styles, L, 8), torch.float64), lag_n=((n_styles, L), torch.int64),
                  part=((B, L, 8), torch.float64), onset=((B, T), torch.float64), speed=((B, 2, T), torch.float64))
    bufs = {k: _padded(*v) for k, v in shapes.items()}
    for k in ('beat_dist', 'beat_counts', 'lag_sums', 'lag_n'):
        bufs[k][1].zero_()
    dev = [torch.from_numpy(a).to(DEV) for a in (audio, fake, real, style)]
    dstd = None if std is None else torch.from_numpy(std).to(DEV)
    part = F.eval_sync(*dev, bufs['beat_dist'][1], bufs['beat_counts'][1], n_lags, onset_delta, dstd, bufs['part'][1],
                       bufs['onset'][1], bufs['speed'][1])
    F.eval_sync_finish(part, dev[3], T, bufs['lag_sums'][1], bufs['lag_n'][1])
    torch.cuda.synchronize()
    assert part.data_ptr() == bufs['part'][0].data_ptr()
    for k, (shape, dtype) in shapes.items():
        tail = bufs[k][0][int(np.prod(shape)):]
        assert (tail == (ICANARY if dtype == torch.int64 else CANARY)).all(), k
    return {k: _np(v[1]) for k, v in bufs.items()}


def _compare(got, ref, style, C, K, n_styles=N_STYLES, exact=False):
    """Integers equal; sums within sum_tol(n + C + 2K, |sum|); series within series_tol; a dropped clip's part
    untouched.  exact: the floats equal too."""
    ok = (style >= 0) & (style < n_styles)
    assert np.array_equal(got['beat_dist'], ref['beat_dist'])
    assert np.array_equal(got['beat_counts'], ref['beat_counts'])
    assert np.array_equal(got['lag_n'], ref['lag_n'])
    assert (got['part'][~ok] == CANARY).all()
    for name, g, r, n in (('lag_sums', got['lag_sums'], ref['lag_sums'], ref['lag_n'][..., None]),
                          ('part', got['part'][ok], ref['part'][ok], None)):
        if n is None:
            T = ref['onset'].shape[1]
            L = r.shape[1]
            n = np.array([max(T - 1 - abs(i - L // 2), 0) for i in range(L)], np.float64)[None, :, None]
        tol = np.zeros_like(r) if exact else S.sum_tol(n + C + 2 * K, np.abs(r))
        err = np.abs(g - r)
        worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size and not exact else 0.0
        print(f'SYNC-EVAL {name}: max err {float(err.max()) if err.size else 0.0:.3e}, worst err / tol {worst:.3f}')
        assert (err <= tol).all(), f'{name}: err / tol up to {worst:.3f}'
    for name, g, r in (('onset', got['onset'], ref['onset']), ('speed', got['speed'], ref['speed'])):
        tol = np.zeros_like(r) if exact else S.series_tol(C, K, r)
        err = np.abs(g - r)
        print(f'SYNC-EVAL {name}: max err {float(err.max()):.3e}')
        assert (err <= tol).all(), name
        assert not g[..., 0].any()


# ------------------------------------------------------------------------------ the kernels
@pytest.mark.parametrize('with_std', [False, True], ids=['raw', 'std'])
@pytest.mark.parametrize('shape', S.RANDOM_SHAPES, ids=_mid)
def test_eval_sync_against_reference(shape, with_std):
    """T = 1, 2, 3: nothing counted, lag_n by its formula; T = 4: the only candidate frame is 2; C = 1 and
    K = 5: one audio column, ragged keypoint quads; C = 80, T = 67: no multiple of the wave or of a wave's run
    of frames; T = 480: the long form; T = 2048: the LDS bound.  Styles 0 and 2 of 3 (1 absent), one clip out
    of range (-1 or n_styles).  The speeds' sums also meet eval_clip's within the series bound."""
    from a2m import functional as F
    B, T, C, K = shape
    case = _case(shape)
    std = case['std'] if with_std else None
    audio, fake, real, style = case['audio'], case['fake'], case['real'], case['style']
    ref = S.sync_sums(audio, fake, real, style, N_STYLES, audio_std=std)
    assert ref['margin'] >= 1e-9
    got = _run(audio, fake, real, style, std)
    _compare(got, ref, style, C, K)
    ok = (style >= 0) & (style < N_STYLES)
    assert ok.sum() == B - (B >= 2) and not ref['lag_n'][1].any()
    want_n = np.array([max(T - 1 - abs(l), 0) for l in range(-4, 5)])
    assert np.array_equal(ref['lag_n'][0], want_n * (style == 0).sum())
    if T < 4:
        assert not ref['beat_dist'].any() and not ref['beat_counts'].any()
    if T == 4:
        assert all(not f[:, [0, 1, 3]].any() for f in ref['flags'])
    if T >= 64:
        assert (ref['beat_counts'][0] > 0).all() and ref['beat_dist'][0].sum(-1).all()
    # eval_clip's speed sums: the generated pose de-normalised with mean 0, std 1 is itself
    hist = torch.zeros(N_STYLES, 4, 8, dtype=torch.int64, device=DEV)
    dev = [torch.from_numpy(a).to(DEV) for a in (fake, real, style)]
    zero, one = torch.zeros(2 * K, device=DEV), torch.ones(2 * K, device=DEV)
    _, part, _ = F.eval_clip(*dev, zero, one, N_STYLES, 0.2, 1.0, 1.0, hist)
    clip = _np(part)[ok][:, 1:3]
    mine = got['speed'][ok].sum(-1)
    print(f'SYNC-EVAL speed sums against eval_clip: max err {float(np.abs(mine - clip).max()):.3e}')
    assert (np.abs(mine - clip) <= S.series_tol(C, K, clip)).all()


@pytest.mark.parametrize('param', [dict(n_lags=0), dict(n_lags=16, shape=(3, 5, 1, 5)), dict(n_dist=2)],
                         ids=['lags0', 'lags16xT5', 'dist2'])
def test_eval_sync_parameters(param):
    """n_lags = 0: the one lag; n_lags = 16 with T = 5: the lags beyond +-3 have no pairs, lag_n = 0 and r NaN;
    n_dist = 2: everything at distance >= 1 in the catch-all bin; and another onset_delta."""
    from a2m.evaluation import _sync_metrics
    param = dict(param)
    shape = param.pop('shape', (5, 64, 128, 52))
    B, T, C, K = shape
    case = _case(shape)
    audio, fake, real, style = case['audio'], case['fake'], case['real'], case['style']
    for delta in (1.0, 1.25):
        ref = S.sync_sums(audio, fake, real, style, N_STYLES, audio_std=case['std'], onset_delta=delta, **param)
        assert ref['margin'] >= 1e-9
        got = _run(audio, fake, real, style, case['std'], onset_delta=delta, **param)
        _compare(got, ref, style, C, K)
    if param.get('n_lags') == 16:
        assert not got['lag_n'][:, :13].any() and not got['lag_n'][:, 20:].any() and got['lag_n'][0, 13:20].all()
        assert not got['lag_sums'][:, :13].any() and not got['lag_sums'][:, 20:].any()
        m = _sync_metrics(got['beat_dist'][0], got['beat_counts'][0], got['lag_sums'][0], got['lag_n'][0], 1.0)
        r = np.array(m['sync_corr_real'])
        assert len(r) == 33 and np.isnan(r[:13]).all() and np.isnan(r[20:]).all()
    if param.get('n_dist') == 2:
        full = S.sync_sums(audio, fake, real, style, N_STYLES, audio_std=case['std'], onset_delta=delta)['beat_dist']
        assert np.array_equal(got['beat_dist'][..., 0], full[..., 0])
        assert np.array_equal(got['beat_dist'][..., 1], full[..., 1:].sum(-1)) and got['beat_dist'][..., 1].sum() > 0


def _from_series(o, s_real, s_fake, C=4, K=5):
    """audio [T, C] and x-only poses [T, 2K] of small integers whose onset is o[1:] (>= 0) and whose speeds are
    s_real[1:], s_fake[1:]: every column steps up by o[t], every joint moves s[t] in x."""
    audio = np.repeat(np.cumsum(o)[:, None], C, 1).astype(np.float32)
    poses = []
    for s in (s_real, s_fake):
        p = np.zeros((len(s), 2 * K), np.float32)
        p[:, :K] = np.cumsum(s)[:, None] + 7.0 * np.arange(K)[None, :]
        p[:, K:] = 3.0 * np.arange(K)[None, :]
        poses.append(p)
    return audio, poses[0], poses[1]


def test_eval_sync_exact_ties():
    """Small-integer audio with C = 4 and x-only integer motion with K = 5: every onset and speed is exact in
    any summation order, so everything equals the reference exactly, sums included.  Clip 0 holds plateaus on
    both sides of a peak and of a dip and a peak exactly on the threshold (mean 2, onset_delta 1); clip 1 has
    constant audio; clips 2 and 3 are random small integers, full of ties."""
    g = np.random.default_rng(12)
    o0 = np.array([0, 0, 2, 2, 0, 1, 3, 3, 3, 1, 0, 2, 1, 1, 2, 4, 7], np.float64)
    s0 = np.array([0, 3, 1, 1, 3, 2, 2, 1, 4, 4, 2, 3, 3, 1, 1, 1, 2], np.float64)
    T = len(o0)
    assert o0[1:].sum() == 2 * (T - 1)
    clips = [_from_series(o0, s0, s0[::-1].copy()), _from_series(np.zeros(T), s0, np.roll(s0, 3))]
    for _ in range(2):
        clips.append(_from_series(g.integers(0, 4, T).astype(np.float64), g.integers(1, 4, T).astype(np.float64),
                                  g.integers(1, 4, T).astype(np.float64)))
    audio, real, fake = (np.stack([c[i] for c in clips]) for i in range(3))
    style = np.array([0, 1, 2, 2], np.int32)
    for std in (None, np.full(4, 2.0, np.float32)):
        ref = S.sync_sums(audio, fake, real, style, N_STYLES, n_lags=3, n_dist=4, audio_std=std)
        o, s = ref['onset'], ref['speed'][:, 0]
        scale = 1.0 if std is None else 2.0
        assert np.array_equal(o[0], o0 * scale) and np.array_equal(s[0], s0)
        fa, fr, _ = ref['flags']
        t = np.arange(2, T - 1)
        # each side of each comparison is pinned by a frame of clip 0 that sits on the tie
        assert (fa[0, t] & (o[0, t] == o[0, t + 1])).any() and (~fa[0, t] & (o[0, t] == o[0, t - 1]) & (o[0, t] > o[0, t + 1])).any()
        assert (fr[0, t] & (s[0, t] == s[0, t + 1])).any() and (~fr[0, t] & (s[0, t] == s[0, t - 1]) & (s[0, t] < s[0, t + 1])).any()
        thr = o[0, 1:].mean()
        assert thr == 2.0 * scale and (~fa[0, t] & (o[0, t] == thr) & (o[0, t] > o[0, t - 1]) & (o[0, t] >= o[0, t + 1])).any()
        n1 = ref['beat_counts'][1]
        assert n1[0] == 0 and n1[1] > 0 and n1[2] > 0
        assert np.array_equal(ref['beat_dist'][1, :, 0, -1], n1[1:]) and ref['beat_dist'][1].sum() == n1[1:].sum()
        got = _run(audio, fake, real, style, std, n_lags=3, n_dist=4)
        _compare(got, ref, style, 4, 5, exact=True)


def test_wrappers_refuse_wrong_dtypes():
    """Device tensors of the wrong dtype are a TypeError before any launch: the accumulators keep their zeros."""
    from a2m import functional as F
    B, T, C, Fd, L = 2, 8, 16, 10, 9
    z = functools.partial(torch.zeros, device=DEV)
    audio, pose, style = z(B, T, C), z(B, T, Fd), z(B, dtype=torch.int32)
    dist, counts = z(N_STYLES, 2, 2, 32, dtype=torch.int64), z(N_STYLES, 3, dtype=torch.int64)
    part, sums, n = z(B, L, 8, dtype=torch.float64), z(N_STYLES, L, 8, dtype=torch.float64), z(N_STYLES, L, dtype=torch.int64)
    bad_sync = [dict(audio=audio.double()), dict(fake_px=pose.double()), dict(style=style.long()),
                dict(beat_dist=dist.int()), dict(beat_counts=counts.double()), dict(audio_std=z(C, dtype=torch.float64)),
                dict(part=part.float()), dict(onset_out=z(B, T)), dict(speed_out=z(B, 2, T))]
    for bad in bad_sync:
        kw = dict(audio=audio, fake_px=pose, real_px=pose, style=style, beat_dist=dist, beat_counts=counts)
        kw.update(bad)
        with pytest.raises(TypeError):
            F.eval_sync(**kw)
    for bad in (dict(part=part.float()), dict(style=style.long()), dict(lag_sums=sums.float()), dict(lag_n=n.int())):
        kw = dict(part=part, style=style, T=T, lag_sums=sums, lag_n=n)
        kw.update(bad)
        with pytest.raises(TypeError):
            F.eval_sync_finish(**kw)
    assert not dist.any() and not counts.any() and not sums.any() and not n.any()


# ------------------------------------------------------------------------------ the evaluator
def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


@pytest.mark.parametrize('late', [0, 2])
def test_planted_signal_through_the_evaluator(late):
    """The planted signal of test_sync_ref_cpu.py: every beat distance is `late`, beat_align = beat_recall =
    exp(-late^2 / 2) (1 for late = 0), the most negative lag is `late`; the inputs are small integers, so
    result() equals the reference's host formulas on the reference's sums."""
    from a2m.evaluation import SYNC_METRICS, AudioSyncEvaluator
    audio, pose, on = S.planted(late)
    style = np.array([0, 1], np.int32)
    ev = AudioSyncEvaluator(2, device=DEV)
    ev.update(*[torch.from_numpy(a).to(DEV) for a in (audio, pose, pose, style)])
    res = ev.result()
    assert sorted(res, key=str) == [0, 1, 'all']
    ref = S.sync_sums(audio, pose, pose, style, 2)
    for key, sel in ((0, 0), (1, 1), ('all', None)):
        m = res[key]
        assert sorted(m) == sorted(SYNC_METRICS)
        acc = [ref[k][sel] if sel is not None else ref[k].sum(0) for k in ('beat_dist', 'beat_counts', 'lag_sums', 'lag_n')]
        want = S.metrics(*acc)
        for k in SYNC_METRICS:
            assert np.allclose(m[k], want[k], rtol=1e-13, atol=0, equal_nan=True), k
        n = len(on) * (2 if key == 'all' else 1)
        assert (m['n_audio_beats'], m['n_motion_beats_real'], m['n_motion_beats_fake']) == (n, n, n)
        for k in ('beat_align_real', 'beat_align_fake', 'beat_recall_real', 'beat_recall_fake'):
            assert m[k] == pytest.approx(np.exp(-late ** 2 / 2.0), rel=1e-15) and (late or m[k] == 1.0)
        r = np.array(m['sync_corr_fake'])
        assert int(np.argmin(r)) - 4 == late and r.min() < -0.9 and m['beat_far_share'] == 0.0
    assert np.array_equal(_np(ev.state()['beat_dist'])[..., late], np.full((2, 2, 2), len(on)))
    assert ev.result(beat_sigma=2.0)[0]['beat_align_real'] == pytest.approx(np.exp(-late ** 2 / 8.0), rel=1e-15)


def test_evaluator_is_deterministic_and_pools_all():
    """Two identical two-batch passes, reset() in between, leave byte-identical arenas; the pass as one batch
    leaves the same integer accumulators (and sums within their tolerance); 'all' is the sum over the styles:
    what one evaluator fed every counted clip as a single style gives."""
    from a2m.evaluation import AudioSyncEvaluator
    shape = (5, 64, 128, 52)
    B, T, C, K = shape
    case = _case(shape)
    host = [case[k] for k in ('audio', 'fake', 'real', 'style')]
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    ev = AudioSyncEvaluator(N_STYLES, audio_std=case['std'], device=DEV)
    arenas = []
    for _ in range(2):
        ev.reset()
        ev.update(*[a[:3] for a in dev])
        ev.update(*[a[3:] for a in dev])
        arenas.append(ev._arena.clone().view(torch.int64))
    assert torch.equal(arenas[0], arenas[1]) and arenas[0].any()
    split = {k: _np(v).copy() for k, v in ev.state().items()}
    res = ev.result()
    ev.reset()
    ev.update(*dev)
    whole = {k: _np(v) for k, v in ev.state().items()}
    ref = S.sync_sums(*host, N_STYLES, audio_std=case['std'])
    for k in ('beat_dist', 'beat_counts', 'lag_n'):
        assert np.array_equal(split[k], whole[k]) and np.array_equal(whole[k], ref[k]), k
    tol = S.sum_tol(ref['lag_n'][..., None] + C + 2 * K, ref['lag_abs'])
    assert (np.abs(split['lag_sums'] - ref['lag_sums']) <= tol).all() and (np.abs(whole['lag_sums'] - ref['lag_sums']) <= tol).all()
    ok = (host[3] >= 0) & (host[3] < N_STYLES)
    keep = torch.from_numpy(np.flatnonzero(ok)).to(DEV)
    pooled = AudioSyncEvaluator(1, audio_std=case['std'], device=DEV)
    pooled.update(*[a[keep] for a in dev[:3]], torch.zeros(len(keep), dtype=torch.int32, device=DEV))
    want = pooled.result()[0]
    assert res[1]['n_audio_beats'] == 0 and np.isnan(res[1]['beat_align_real']) and np.isnan(res[1]['sync_corr_real']).all()
    for k, v in want.items():
        if k.startswith('sync_corr'):
            # r from sums that differ by their tolerance (about 200 u relative); the variances cancel a digit or two
            assert np.allclose(res['all'][k], v, rtol=0, atol=1e-10), k
        else:
            assert _same(res['all'][k], v), k                                 # integers underneath
    for k in ('n_audio_beats', 'n_motion_beats_real', 'n_motion_beats_fake'):
        assert res['all'][k] == res[0][k] + res[1][k] + res[2][k] > 0


# ------------------------------------------------------------------------------ end to end
SPEAKERS = ['seth', 'oliver']     # A, B speak as oliver (style 1), C, D as seth (style 0)
ARR = P.arrays()
N_BINS, SPEED_MAX, ACCEL_MAX = 64, 16.0, 32.0
E2E = dict(n_bins=N_BINS, speed_max=SPEED_MAX, accel_max=ACCEL_MAX)


def _loader(batch_size=4):
    from a2m.data import PatsLoader
    table = [P.row('test', i, 'oliver' if i in 'AB' else 'seth') for i in 'ABCD']
    return PatsLoader(ARR, table, SPEAKERS, time=P.TIME, fs_new=P.FS_NEW, window_hop=5, shuffle=False, device=DEV,
                      batch_size=batch_size)


def _stats(seed=11):
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    return [torch.from_numpy(a).to(DEV) for a in (pm, ps, am, asd)]


def test_sync_pass_does_not_synchronise():
    """What evaluate(..., sync=True) loops over -- the loader's batches with styles, the generator, both
    evaluators' update -- under torch's sync debug mode 'error' from after iter() up to result(), after a
    first pass has created the buffers and code objects.  The two passes leave equal accumulators."""
    from a2m.evaluation import AudioSyncEvaluator, PoseEvaluator
    g, _ = _models(DEV)
    g.eval()
    loader = _loader()
    pm, ps, am, asd = _stats()
    ev = PoseEvaluator(pm, ps, 2, device=DEV, **E2E)
    sev = AudioSyncEvaluator(2, audio_std=asd, device=DEV)
    pairs = loader.pairs('test', torch.zeros_like(pm), torch.ones_like(ps), am, asd, with_style=True)

    def run(it):
        n = 0
        with torch.no_grad():
            for audio, real, style in it:
                ev.update(g(audio)[0], real, style)
                sev.update(audio, ev.fake_px(*real.shape[:2]), real, style)
                n += 1
        return n

    run(pairs)
    first = sev._arena.clone()
    ev.reset()
    sev.reset()
    it = iter(pairs)
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            probe.item()                     # the mode is honoured: a synchronisation is an error
        n = run(it)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert n == 4
    res = sev.result()
    assert res['all']['n_audio_beats'] > 0 and res['all']['n_motion_beats_fake'] > 0
    assert torch.equal(sev._arena.view(torch.int64), first.view(torch.int64))


def test_evaluate_with_sync_end_to_end():
    """evaluate(..., sync=True) over the 13-clip test split of two speakers: every entry holds METRICS +
    SYNC_METRICS, the METRICS values are bitwise those of evaluate(..., sync=False), and the sync values match
    sync_ref fed from the public ops (the loader's standardised audio with its audio_std, the generator's
    output de-normalised); the correlations there pass within 512 x the onset tolerance 8 (C + 2K) u, absolute
    (the summation orders differ and the variances under r cancel a digit or two).  Standardising the audio
    does not move the onsets: with mean 0 and a std of powers of two (an exact standardisation in float32; a
    general std rounds at 2^-24) the audio and real-pose results, correlations included, equal those of the raw
    pass bit for bit.  The generated pose's are not compared: the generator's input differs."""
    from a2m.evaluation import METRICS, SYNC_METRICS, evaluate
    from a2m.normalization import denormalize
    g, _ = _models(DEV)
    loader = _loader()
    pm, ps, am, asd = _stats()
    kw = dict(pose_mean=pm, pose_std=ps, **E2E)
    got = evaluate(g, loader, 'test', audio_mean=am, audio_std=asd, sync=True, **kw)
    base = evaluate(g, loader, 'test', audio_mean=am, audio_std=asd, **kw)
    assert all(m.training for m in g.modules())
    assert sorted(got) == sorted(base) == ['all', 'dropped', 'oliver', 'seth'] and got['dropped'] == 0
    for name in ('all', 'oliver', 'seth'):
        assert sorted(base[name]) == sorted(METRICS) and sorted(got[name]) == sorted(METRICS + SYNC_METRICS)
        for k in METRICS:
            assert _same(got[name][k], base[name][k]), (name, k)
    # the reference, from the public ops
    audios, fakes, reals, styles = [], [], [], []
    g.eval()
    with torch.no_grad():
        zero, one = torch.zeros_like(pm), torch.ones_like(ps)
        for audio, real, style in loader.pairs('test', zero, one, am, asd, with_style=True):
            audios.append(_np(audio))
            fakes.append(_np(denormalize(g(audio)[0], pm, ps)))
            reals.append(_np(real))
            styles.append(_np(style))
    g.train()
    audio, fake, real, style = (np.concatenate(a) for a in (audios, fakes, reals, styles))
    C, K = audio.shape[2], 52
    per = S.sync_sums(audio, fake, real, style, 2, audio_std=_np(asd))
    pooled = S.sync_sums(audio, fake, real, np.zeros_like(style), 1, audio_std=_np(asd))
    assert per['margin'] >= 1e-9, 'the reference sits on a tie: draw other weights'
    r_tol = 512 * 8 * (C + 2 * K) * S.U
    keys = ('beat_dist', 'beat_counts', 'lag_sums', 'lag_n')
    for name, ref, s in (('seth', per, 0), ('oliver', per, 1), ('all', pooled, 0)):
        want = S.metrics(*(ref[k][s] for k in keys))
        assert want['n_audio_beats'] > 0 and want['n_motion_beats_fake'] > 0
        for k in SYNC_METRICS:
            if k.startswith('sync_corr'):
                err = np.abs(np.array(got[name][k]) - np.array(want[k])).max()
                print(f'SYNC-EVAL {name} {k}: max err {err:.3e} (bound {r_tol:.3e})')
                assert err <= r_tol, (name, k)
            else:
                assert _same(got[name][k], want[k]), (name, k)
    # raw audio against an exact standardisation
    p2 = torch.from_numpy(np.random.default_rng(2).choice([0.5, 1.0, 2.0, 4.0], C).astype(np.float32)).to(DEV)
    raw = evaluate(g, loader, 'test', sync=True, **kw)
    scaled = evaluate(g, loader, 'test', audio_mean=torch.zeros_like(p2), audio_std=p2, sync=True, **kw)
    for name in ('all', 'oliver', 'seth'):
        # (a / p) * p gives the raw differences back exactly, the same terms in the same order: equal bits
        for k in ('n_audio_beats', 'n_motion_beats_real', 'beat_align_real', 'beat_recall_real', 'sync_lag_real',
                  'sync_corr_real'):
            assert _same(raw[name][k], scaled[name][k]), (name, k)
