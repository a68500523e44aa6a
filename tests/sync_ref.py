"""The audio-motion synchrony metrics of a2m.evaluation.AudioSyncEvaluator restated in float64 numpy
(DESIGN.md 7.7).

audio is [B, T, C] float32, the poses [B, T, 2K] float32 in pixels (a frame being its x row then its
y row), style [B].  Next to each result comes what its tolerance needs: per lag sum the term count
and the sum of the terms' magnitudes (eval_ref.sum_tol), and `margin`, the smallest relative gap
|x - y| / max(|x|, |y|) over every beat comparison made with unequal operands (o[t] against both
neighbours and the threshold, s[t] against both neighbours): both sides decide a beat in float64 from
values a few ulps apart, so a test's inputs must keep the margin clear of that."""
import numpy as np

from eval_ref import speed_accel, sum_tol  # noqa: F401  (sum_tol: for the tests that import this module)

U = 2.0 ** -53


def series_tol(C, K, value):
    """8 (C + 2K) u |value|: an onset is a sum of C terms, a speed one of K - 1 square roots of a sum of two
    squares; the factor 8 covers the roundings inside a term and the division."""
    return 8.0 * (C + 2 * K) * U * np.abs(np.asarray(value, np.float64))


def onset_strength(audio, audio_std=None):
    """o [B, T]: o[t] = (1/C) sum_c max(0, (a[t,c] - a[t-1,c]) sigma_c) for t >= 1, o[0] = 0."""
    a = np.asarray(audio)
    assert a.dtype == np.float32 and a.ndim == 3
    a = a.astype(np.float64)
    B, T, C = a.shape
    sigma = np.ones(C) if audio_std is None else np.asarray(audio_std, np.float32).astype(np.float64)
    o = np.zeros((B, T))
    if T > 1:
        o[:, 1:] = np.maximum((a[:, 1:] - a[:, :-1]) * sigma, 0.0).sum(-1) / C
    return o


def speeds(px):
    """s [B, T]: eval_ref.speed_accel's speed for t >= 1, s[0] = 0."""
    sp, _ = speed_accel(px)
    return np.concatenate([np.zeros((sp.shape[0], 1)), sp], 1)


def _gap(x, y):
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    ne = x != y
    if not ne.any():
        return np.inf
    return float((np.abs(x - y)[ne] / np.maximum(np.abs(x), np.abs(y))[ne]).min())


def beats(o, s_real, s_fake, onset_delta=1.0):
    """Boolean [B, T] beat flags (audio, real motion, generated motion) and the margin."""
    B, T = o.shape
    fa, fr, ff = (np.zeros((B, T), bool) for _ in range(3))
    if T < 4:
        return fa, fr, ff, np.inf
    thr = onset_delta * o[:, 1:].mean(1, keepdims=True)
    c, lo, hi = slice(2, T - 1), slice(1, T - 2), slice(3, T)      # t in [2, T-2], t - 1, t + 1
    fa[:, c] = (o[:, c] > o[:, lo]) & (o[:, c] >= o[:, hi]) & (o[:, c] > thr)
    margin = min(_gap(o[:, c], o[:, lo]), _gap(o[:, c], o[:, hi]), _gap(o[:, c], thr))
    for s, f in ((s_real, fr), (s_fake, ff)):
        f[:, c] = (s[:, c] < s[:, lo]) & (s[:, c] <= s[:, hi])
        margin = min(margin, _gap(s[:, c], s[:, lo]), _gap(s[:, c], s[:, hi]))
    return fa, fr, ff, margin


def nearest_hist(src, dst, n_dist):
    """int64 [n_dist]: every True of src [T] counted at min(distance to the nearest True of dst, n_dist - 1);
    n_dist - 1 where dst has none."""
    ps, pd = np.flatnonzero(src), np.flatnonzero(dst)
    if not len(ps):
        return np.zeros(n_dist, np.int64)
    d = np.abs(ps[:, None] - pd[None, :]).min(1) if len(pd) else np.full(len(ps), n_dist - 1)
    return np.bincount(np.minimum(d, n_dist - 1), minlength=n_dist).astype(np.int64)


def lag_sums_clip(o, s_real, s_fake, n_lags):
    """[2 n_lags + 1, 8] sums of one clip (o, o^2, then s, s^2, o s for the real and for the generated
    pose) over the pairs (o[t], s[t + l]) with t and t + l in [1, T-1], and the pair counts [2 n_lags + 1]."""
    T = len(o)
    out, n = np.zeros((2 * n_lags + 1, 8)), np.zeros(2 * n_lags + 1, np.int64)
    for i, l in enumerate(range(-n_lags, n_lags + 1)):
        t = np.arange(max(1, 1 - l), min(T - 1, T - 1 - l) + 1)
        n[i] = len(t)
        x, yr, yf = o[t], s_real[t + l], s_fake[t + l]
        out[i] = [x.sum(), (x * x).sum(), yr.sum(), (yr * yr).sum(), (x * yr).sum(), yf.sum(), (yf * yf).sum(),
                  (x * yf).sum()]
    return out, n


def sync_sums(audio, fake_px, real_px, style, n_styles, n_lags=4, n_dist=32, onset_delta=1.0, audio_std=None):
    """Everything a2m_eval_sync_f64 and a2m_eval_sync_finish_f64 accumulate: onset [B, T], speed [B, 2, T]
    (real, generated), flags (audio, real, generated; bool [B, T]), beat_dist [S, 2, 2, n_dist], beat_counts
    [S, 3], part [B, L, 8], lag_sums [S, L, 8] with lag_abs (every term is >= 0, so the same values) and
    lag_n [S, L] (the pair count, also each sum's term count), and margin."""
    style = np.asarray(style)
    o = onset_strength(audio, audio_std)
    sr, sf = speeds(real_px), speeds(fake_px)
    B, T = o.shape
    S, L = n_styles, 2 * n_lags + 1
    fa, fr, ff, margin = beats(o, sr, sf, onset_delta)
    out = dict(onset=o, speed=np.stack([sr, sf], 1), flags=(fa, fr, ff), margin=margin,
               beat_dist=np.zeros((S, 2, 2, n_dist), np.int64), beat_counts=np.zeros((S, 3), np.int64),
               part=np.zeros((B, L, 8)), lag_sums=np.zeros((S, L, 8)), lag_n=np.zeros((S, L), np.int64))
    for b in range(B):
        out['part'][b], n = lag_sums_clip(o[b], sr[b], sf[b], n_lags)
        s = int(style[b])
        if not 0 <= s < S:
            continue
        out['lag_sums'][s] += out['part'][b]
        out['lag_n'][s] += n
        out['beat_counts'][s] += [fa[b].sum(), fr[b].sum(), ff[b].sum()]
        for w, fm in enumerate((fr, ff)):
            out['beat_dist'][s, w, 0] += nearest_hist(fm[b], fa[b], n_dist)
            out['beat_dist'][s, w, 1] += nearest_hist(fa[b], fm[b], n_dist)
    out['lag_abs'] = out['lag_sums'].copy()
    return out


def beat_align(hist, beat_sigma=1.0):
    h = np.asarray(hist, np.float64)
    if h.sum() <= 0:
        return np.nan
    d = np.arange(len(h), dtype=np.float64)
    return float((h * np.exp(-d ** 2 / (2.0 * beat_sigma ** 2))).sum() / h.sum())


def pearson(n, sums5):
    """r from (sum x, sum x^2, sum y, sum y^2, sum x y); NaN where n < 2 or a variance is <= 0."""
    sx, sxx, sy, syy, sxy = (float(v) for v in sums5)
    n = float(n)
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    if n < 2 or vx <= 0 or vy <= 0:
        return np.nan
    return (n * sxy - sx * sy) / np.sqrt(vx * vy)


def metrics(beat_dist, beat_counts, lag_sums, lag_n, beat_sigma=1.0):
    """The host formulas on one style's accumulators: a dict of a2m.evaluation.SYNC_METRICS."""
    L = len(lag_n)
    out = dict(n_audio_beats=int(beat_counts[0]), n_motion_beats_real=int(beat_counts[1]),
               n_motion_beats_fake=int(beat_counts[2]))
    for w, name in enumerate(('real', 'fake')):
        out['beat_align_' + name] = beat_align(beat_dist[w, 0], beat_sigma)
        out['beat_recall_' + name] = beat_align(beat_dist[w, 1], beat_sigma)
        r = [pearson(lag_n[i], [lag_sums[i, 0], lag_sums[i, 1], *lag_sums[i, 2 + 3 * w:5 + 3 * w]]) for i in range(L)]
        out['sync_corr_' + name] = r
        out['sync_lag_' + name] = np.nan if np.isnan(r).all() else int(np.nanargmax(r)) - L // 2
    far, tot = beat_dist[:, 0, -1].sum(), beat_dist[:, 0].sum()
    out['beat_far_share'] = float(far) / float(tot) if tot else np.nan
    return out


# ------------------------------------------------------------------------------------ test inputs
RANDOM_SHAPES = [(3, 1, 128, 52), (3, 2, 128, 52), (3, 3, 8, 52), (3, 4, 128, 52), (3, 5, 1, 5), (5, 64, 128, 52),
                 (4, 67, 80, 52), (2, 480, 128, 52), (1, 2048, 128, 2)]     # (B, T, C, K)
N_STYLES = 3


def styles(B):
    """Styles 0 and 2 of 3 clip by clip; from two clips on the second is out of range (-1 or n_styles)."""
    st = np.array([(0, 2)[b % 2] for b in range(B)], np.int32)
    if B >= 2:
        st[1] = -1 if B % 2 else N_STYLES
    return st


# the seed of each random case.  A seed whose reference comes within 1e-9 relative of a beat decision is
# replaced here by hand (test_sync_ref_cpu.py fails until it is); the bound is never lowered.
SEEDS = {shape: 500 for shape in RANDOM_SHAPES}


def random_case(shape):
    """standard_normal audio, random-walk poses of about 3 px a frame (the generated one with its own walk),
    an audio_std in [0.5, 2.5), from SEEDS[shape]; margin is the smaller of the reference's margins with
    audio_std absent and given."""
    B, T, C, K = shape
    g = np.random.default_rng(SEEDS[shape] + 7 * T + C)
    audio = g.standard_normal((B, T, C)).astype(np.float32)
    real = (g.uniform(-250, 250, (B, 1, 2 * K)) + np.cumsum(g.standard_normal((B, T, 2 * K)) * 3, 1)).astype(np.float32)
    fake = (real + np.cumsum(g.standard_normal((B, T, 2 * K)) * 2, 1)).astype(np.float32)
    std = (g.random(C) * 2 + 0.5).astype(np.float32)
    st = styles(B)
    margin = min(sync_sums(audio, fake, real, st, N_STYLES, audio_std=s)['margin'] for s in (None, std))
    return dict(audio=audio, fake=fake, real=real, std=std, style=st, margin=margin)


def planted(late=0, B=2, T=64, C=128, K=52):
    """Audio onsets every 8 frames from frame 6 (a step up in every column at the onset, back down two
    frames later); all joints move in x alone at 4 px a frame, except for a dip to 1 px a frame at each
    onset frame + `late`.  The generated pose is the real one."""
    audio = np.zeros((B, T, C), np.float32)
    on = np.arange(6, T - 2 - late, 8)
    audio[:, on] = 1.0
    audio[:, on + 1] = 1.0
    speed = np.full(T, 4.0)
    speed[on + late] = 1.0
    speed[0] = 0.0
    x = np.cumsum(speed)
    pose = np.zeros((B, T, 2 * K), np.float32)
    pose[:, :, :K] = x[None, :, None] + np.arange(K)[None, None, :] * 5.0
    pose[:, :, K:] = np.arange(K)[None, None, :] * 3.0
    return audio, pose, on
