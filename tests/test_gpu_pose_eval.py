"""The evaluation pass on the device: csrc/pose_eval.hip's three kernels against tests/eval_ref.py
(float64 numpy), and a2m.evaluation.PoseEvaluator / evaluate on the real generator and a synthetic
PatsLoader against the same reference fed from the public ops.

Integers (PCK hits, histogram counts, clip and frame counts, the de-normalised pose's bits) are
compared for equality.  Both sides decide a hit and a bin in float64 from the same float32 values, a
few ulps of float64 apart, so the inputs are drawn until, in the reference alone, no keypoint distance
lies within 1e-9 relative of its radius and no speed or acceleration within 1e-9 relative of a bin edge
(asserted on the CPU).

Floating sums (L1, speed sums, sum x, the elements of sum x x^T) pass within
|got - ref| <= 8 n 2^-53 sum |terms| (eval_ref.sum_tol: the any-order summation bound of n terms with a
factor for the roundings inside a term).  The project's self-check is kept: every reference recomputed
with one term left out must move by more than 4 x its tolerance, so a bound that could hide a dropped
term fails on the CPU side (in _check_sum).
"""
import numpy as np
import pytest
import torch

import eval_ref as R
import pats_data_ref as P
from test_gpu_configs import _models

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

CLIP_SHAPES = [(1, 1, 52), (2, 2, 52), (2, 3, 52), (3, 65, 52), (2, 33, 5), (130, 4, 48), (1, 512, 4)]
GRAM_CASES = [(1, 1, 104), (1, 3, 104), (1, 5, 8), (64, 64, 104), (130, 4, 96)]   # (B, T, F): B T frames
N_STYLES, ALPHA, N_BINS, SPEED_MAX, ACCEL_MAX = 3, 0.2, 64, 16.0, 32.0
CANARY = -7777.25
ICANARY = -7777


def _mid(shape):
    return 'x'.join(str(s) for s in shape)


def _np(t):
    return t.detach().cpu().numpy()


def _styles(B, ids=(0, 2), bad=5):
    """Clip by clip from `ids` (id 1 of the 3 never appears); from two clips on, one clip is out of range."""
    st = np.array([ids[b % len(ids)] for b in range(B)], np.int32)
    if B >= 2:
        st[B // 2] = bad if B % 2 else -1
    return st


def _poses(B, T, K, seed):
    """real_px: a pose of a few hundred pixels' extent on a random walk of about 3 px a frame;
    fake_norm: the same pose off by tens of pixels a joint (so that PCK hits and misses mix) with a jitter
    whose amplitude changes from frame to frame and puts part of its speeds beyond SPEED_MAX, normalised
    with mean / std."""
    g, gs = np.random.default_rng(seed), np.random.default_rng(9000 + K)   # the statistics depend on K alone
    base = g.uniform(-250, 250, (B, 1, 2 * K))
    real = (base + np.cumsum(g.standard_normal((B, T, 2 * K)) * 3, 1)).astype(np.float32)
    mean = gs.uniform(-200, 200, 2 * K).astype(np.float32)
    std = gs.uniform(5, 60, 2 * K).astype(np.float32)
    jitter = g.standard_normal((B, T, 2 * K)) * 6 * g.uniform(0, 2.5, (B, T, 1))    # a frame's own amplitude
    off = g.standard_normal((B, 1, 2 * K)) * 70 + jitter
    fake_norm = ((real + off - mean) / std).astype(np.float32)
    return fake_norm, real, mean, std


def _clip_case(shape):
    """Inputs whose float64 reference keeps 1e-9 clear of every decision; reseeded until it does."""
    B, T, K = shape
    style = _styles(B)
    sw, aw = SPEED_MAX / N_BINS, ACCEL_MAX / N_BINS
    for seed in range(100, 120):
        fake_norm, real, mean, std = _poses(B, T, K, seed)
        fake_px = R.denormalise(fake_norm, mean, std)
        ref = R.clip_metrics(fake_px, real, style, N_STYLES, ALPHA, N_BINS, sw, aw)
        if ref['margin'] > 1e-9:
            break
    assert ref['margin'] > 1e-9, 'no seed keeps the reference clear of its thresholds'
    return fake_norm, real, mean, std, style, fake_px, ref


def _check_sum(name, got, ref, n_terms, abs_sum, left_out):
    """|got - ref| <= sum_tol, printed first; and the self-check: the reference without one term
    (left_out, that term's value, where it is not zero) moves by more than 4 x the tolerance."""
    got, ref, left_out = (np.asarray(a, np.float64) for a in (got, ref, left_out))
    tol = R.sum_tol(n_terms, abs_sum)
    err = np.abs(got - ref)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if err.size else 0.0
    print(f'POSE-EVAL {name}: max err {float(err.max()) if err.size else 0.0:.3e}, worst err / tol {worst:.3f}')
    live = left_out != 0
    assert (np.abs(left_out) > 4 * tol)[live].all(), f'{name}: the tolerance would hide a dropped term'
    assert (err <= tol).all(), f'{name}: err / tol up to {worst:.3f}'


class _Acc:
    """The accumulators as views of larger canary-filled buffers, optionally from a nonzero start."""

    def __init__(self, Fd, n_styles=N_STYLES, n_bins=N_BINS, start_seed=None):
        S = n_styles
        g = np.random.default_rng(start_seed or 0)
        self.shapes = dict(counts=(3 * S + 1,), sums=(S, 3), hist=(S, 4, n_bins), sx=(S, 2, Fd), gram=(S, 2, Fd, Fd))
        self.buf, self.view, self.start = {}, {}, {}
        for name, shape in self.shapes.items():
            n = int(np.prod(shape))
            integer = name in ('counts', 'hist')
            buf = torch.full((n + 64,), ICANARY if integer else CANARY, dtype=torch.int64 if integer else torch.float64,
                             device=DEV)
            if start_seed is None:
                start = np.zeros(shape, np.int64 if integer else np.float64)
            else:
                start = g.integers(0, 1000, shape) if integer else g.standard_normal(shape) * 1e4
            buf[:n] = torch.from_numpy(start.reshape(-1)).to(DEV)
            self.buf[name], self.view[name], self.start[name] = buf, buf[:n].view(shape), start

    def check_tails(self):
        for name, shape in self.shapes.items():
            n = int(np.prod(shape))
            canary = ICANARY if name in ('counts', 'hist') else CANARY
            assert (self.buf[name][n:] == canary).all(), name


# ------------------------------------------------------------------------------ the per-clip and finish kernels
@pytest.mark.parametrize('shape', CLIP_SHAPES, ids=_mid)
def test_eval_clip_and_finish(shape):
    """T = 1: no speed; T = 2: speeds, no acceleration; T = 3: one acceleration; T = 65: the 64-frame
    loop's second trip, whose rows wrap the LDS ring; T = 512: eight trips; K = 5: ragged keypoint
    quads; B = 130: more clips than the finish kernel has lanes.  Styles 0 and 2 of 3 (1 absent), one clip
    out of range.  Every output sits in a larger buffer whose tail must keep its canary."""
    from a2m import functional as F
    B, T, K = shape
    Fd = 2 * K
    fake_norm, real, mean, std, style, fake_px, ref = _clip_case(shape)
    acc = _Acc(Fd)
    n = B * T * Fd
    fbuf = torch.full((n + 256,), CANARY, device=DEV)
    pbuf = torch.full((3 * B + 16,), CANARY, dtype=torch.float64, device=DEV)
    hbuf = torch.full((B + 16,), ICANARY, dtype=torch.int32, device=DEV)
    dev = [torch.from_numpy(a).to(DEV) for a in (fake_norm, real, style, mean, std)]
    got_px, part, hits = F.eval_clip(*dev, N_STYLES, ALPHA, SPEED_MAX / N_BINS, ACCEL_MAX / N_BINS, acc.view['hist'],
                                     fbuf[:n].view(B, T, Fd), pbuf[:3 * B].view(B, 3), hbuf[:B])
    F.eval_finish(part, hits, dev[2], T, acc.view['counts'], acc.view['sums'])
    torch.cuda.synchronize()
    assert got_px.data_ptr() == fbuf.data_ptr() and part.data_ptr() == pbuf.data_ptr()
    assert (fbuf[n:] == CANARY).all() and (pbuf[3 * B:] == CANARY).all() and (hbuf[B:] == ICANARY).all()
    acc.check_tails()
    assert (acc.view['sx'] == 0).all() and (acc.view['gram'] == 0).all()
    assert np.array_equal(_np(got_px), fake_px)                       # every clip, the dropped one included
    ok = (style >= 0) & (style < N_STYLES)
    assert ref['dropped'] == (B >= 2) and ok.sum() == B - ref['dropped']
    assert np.array_equal(_np(hits)[ok], ref['hits'][ok])
    assert np.array_equal(_np(acc.view['hist']), ref['hist'])
    assert ref['hist'].sum() == ok.sum() * 2 * (max(T - 1, 0) + max(T - 2, 0))
    if T >= 33:
        assert ref['hist'][:, :, -1].sum() > 0 and ref['hist'][:, :, :-1].sum() > 0   # the catch-all bin is in play
    counts = _np(acc.view['counts'])
    assert np.array_equal(counts[:-1].reshape(N_STYLES, 3), ref['counts']) and counts[-1] == ref['dropped']
    assert not ref['counts'][1].any() and ref['counts'][0, 0] > 0
    # per clip: the sums of one clip; the term left out is the first one of each sum
    sr, sf = ref['speed']
    first = np.stack([np.abs(fake_px.astype(np.float64) - real.astype(np.float64))[:, 0, 0],
                      sr[:, 0] if T > 1 else np.zeros(B), sf[:, 0] if T > 1 else np.zeros(B)], 1)
    _check_sum('part', _np(part)[ok], ref['part'][ok], ref['part_n'][ok], ref['part_abs'][ok], first[ok])
    # per style: the clips' sums; the term left out is the first clip's first term
    lead = np.zeros((N_STYLES, 3))
    for s in range(N_STYLES):
        if (style == s).any():
            lead[s] = first[np.flatnonzero(style == s)[0]]
    _check_sum('sums', _np(acc.view['sums']), ref['sums'], ref['n_terms'], ref['abs_sums'], lead)
    assert not _np(acc.view['sums'])[1].any()


# ------------------------------------------------------------------------------ the Gram kernel
@pytest.mark.parametrize('case', GRAM_CASES, ids=_mid)
def test_eval_gram(case):
    """1, 3 and 5 frames: fewer than one step of 4 and a ragged second step; F = 104: 6 1/2 tiles; F = 8:
    half a tile; 64 x 64 x 104: the flagship batch; 130 x 4 x 96: many short clips.  Four styles with id 1
    empty, the others interleaved clip by clip, one clip out of range; two successive batches on top of a
    nonzero accumulator.  Every element on and above the tile diagonal is held to the sum rule (an f32
    C/D row map would misplace three rows of four in every tile), everything below it must keep its start
    bit for bit, and the mirrored matrix must be symmetric."""
    from a2m import functional as F
    from a2m.evaluation import mirror_gram
    B, T, Fd = case
    S = 4
    acc = _Acc(Fd, n_styles=S, start_seed=77)
    g = np.random.default_rng(1000 + B + T + Fd)
    refs, first = [], None
    for k in range(2):
        real = (g.standard_normal((B, T, Fd)) * 40 + g.uniform(-300, 300, Fd)).astype(np.float32)
        fake = (real + g.standard_normal((B, T, Fd)) * 25).astype(np.float32)
        style = _styles(B, ids=(0, 2, 3), bad=S + k)
        refs.append(R.gram_sums(fake, real, style, S))
        if first is None:
            first = (fake, real, style)
        F.eval_gram(*[torch.from_numpy(a).to(DEV) for a in (fake, real, style)], acc.view['sx'], acc.view['gram'])
    torch.cuda.synchronize()
    acc.check_tails()
    assert np.array_equal(_np(acc.view['counts']), acc.start['counts']) and np.array_equal(_np(acc.view['hist']), acc.start['hist'])
    n = refs[0]['n'] + refs[1]['n']
    assert n[1] == 0 and n[0] > 0
    # the term left out: the first frame of each style's first clip in the first batch (the start is a term too)
    fake, real, style = first
    x0 = np.zeros((S, 2, Fd))
    for s in range(S):
        if (style == s).any():
            b = np.flatnonzero(style == s)[0]
            x0[s] = [real[b, 0].astype(np.float64), fake[b, 0].astype(np.float64)]
    for name, lead in (('sx', x0), ('gram', x0[..., :, None] * x0[..., None, :])):
        ref = acc.start[name] + refs[0][name] + refs[1][name]
        mag = np.abs(acc.start[name]) + refs[0]['abs_' + name] + refs[1]['abs_' + name]
        terms = np.broadcast_to((n + 1).reshape(S, *[1] * (ref.ndim - 1)), ref.shape)
        got = _np(acc.view[name])
        if name == 'gram':
            tile = np.arange(Fd) // 16
            upper = np.broadcast_to(tile[:, None] <= tile[None, :], ref.shape)
            assert np.array_equal(got[~upper], acc.start[name][~upper])          # below the tile diagonal: untouched
            _check_sum('gram', got[upper], ref[upper], terms[upper], mag[upper], lead[upper])
            full = mirror_gram(got)
            assert np.array_equal(full, np.swapaxes(full, -1, -2))
            iu = np.broadcast_to(np.triu(np.ones((Fd, Fd), bool)), ref.shape)
            _check_sum('gram mirrored', np.swapaxes(full, -1, -2)[iu], ref[iu], terms[iu], mag[iu], lead[iu])
        else:
            _check_sum('sx', got, ref, terms, mag, lead)
    assert np.array_equal(_np(acc.view['sx'])[1], acc.start['sx'][1])              # the empty style


# ------------------------------------------------------------------------------ the evaluator
def _fd_of(n, sx, gram):
    from a2m.evaluation import frechet_distance
    return frechet_distance(n, sx[0], gram[0], n, sx[1], gram[1])


def _fd_bound(gr, s, x0, rng, name):
    """fd of style s of the reference sums gr, and its bound: 4 x the largest shift of frechet_distance
    when the sums are perturbed by +- their own tolerance (random signs, 16 draws).  The self-check: without
    the frame x0 ([2, F]: real, generated) fd must move by more than 4 x that bound."""
    n, sx, gram = gr['n'][s], gr['sx'][s], gr['gram'][s]
    fd = _fd_of(n, sx, gram)
    t_sx, t_gram = R.sum_tol(n, gr['abs_sx'][s]), R.sum_tol(n, gr['abs_gram'][s])
    shift = 0.0
    for _ in range(16):
        e = rng.choice([-1.0, 1.0], gram.shape) * t_gram
        e = np.triu(e) + np.swapaxes(np.triu(e, 1), -1, -2)
        shift = max(shift, abs(_fd_of(n, sx + rng.choice([-1.0, 1.0], sx.shape) * t_sx, gram + e) - fd))
    x0 = np.asarray(x0, np.float64)
    loo = abs(_fd_of(n - 1, sx - x0, gram - x0[:, :, None] * x0[:, None, :]) - fd)
    print(f'POSE-EVAL {name} fd {fd:.6e}: perturbation shift {shift:.3e} ({shift / abs(fd):.2e} rel), '
          f'leave-one-frame-out {loo:.3e} ({loo / abs(fd):.2e} rel)')
    assert loo > 4 * (4 * shift), 'the fd bound would hide a dropped frame'
    return fd, 4 * shift


def _run_pass(ev, batches):
    ev.reset()
    for fake_norm, real, style in batches:
        ev.update(fake_norm, real, style)
    return {k: v.clone() for k, v in ev.state().items()}


def test_evaluator_is_deterministic_and_pools_all():
    """The same two-batch pass (6 clips, then 3) run twice, reset() in between, leaves equal accumulators;
    result() matches the reference style by style; and 'all' is what one evaluator fed every counted clip
    as a single style gives (the pooled distribution), which the reference pooled the same way confirms.
    fd is held to _fd_bound; with 63 frames of 104 features the covariances are rank-deficient."""
    from a2m.evaluation import PoseEvaluator
    K, T = 52, 9
    host = []
    for k, B in enumerate((6, 3)):
        fake_norm, real, mean, std = _poses(B, T, K, 300 + k)
        host.append((fake_norm, real, _styles(B)))
    batches = [tuple(torch.from_numpy(a).to(DEV) for a in b) for b in host]
    ev = PoseEvaluator(mean, std, N_STYLES, ALPHA, N_BINS, SPEED_MAX, ACCEL_MAX, device=DEV)
    one, two = _run_pass(ev, batches), _run_pass(ev, batches)
    assert sorted(one) == ['counts', 'gram', 'hist', 'sums', 'sx']
    for name in one:
        assert torch.equal(one[name], two[name]), name
    assert one['counts'][0] > 0 and one['gram'].abs().sum() > 0
    res = ev.result()
    assert sorted(res, key=str) == [0, 1, 2, 'all', 'dropped'] and res['dropped'] == 2
    assert res[1]['n_clips'] == 0 and np.isnan(res[1]['pck']) and np.isnan(res[1]['fd'])
    pooled = PoseEvaluator(mean, std, 1, ALPHA, N_BINS, SPEED_MAX, ACCEL_MAX, device=DEV)
    for f, r, s in batches:
        keep = ((s >= 0) & (s < N_STYLES)).nonzero().reshape(-1)
        pooled.update(f[keep], r[keep], torch.zeros(len(keep), dtype=torch.int32, device=DEV))
    want = pooled.result()[0]
    assert res['all']['n_clips'] == want['n_clips'] == 7 and res['all']['n_frames'] == want['n_frames'] == 7 * T
    for key in ('pck', 'w1_speed', 'w1_accel', 'speed_overflow', 'accel_overflow'):
        assert res['all'][key] == want[key], key                              # integers underneath
    # against the reference, style by style and pooled
    sw, aw = SPEED_MAX / N_BINS, ACCEL_MAX / N_BINS
    fake_px = np.concatenate([R.denormalise(f, mean, std) for f, _, _ in host])
    real = np.concatenate([r for _, r, _ in host])
    style = np.concatenate([s for _, _, s in host])
    ok = (style >= 0) & (style < N_STYLES)
    ref = R.clip_metrics(fake_px, real, style, N_STYLES, ALPHA, N_BINS, sw, aw)
    gr = R.gram_sums(fake_px, real, style, N_STYLES)
    ref_all = R.clip_metrics(fake_px[ok], real[ok], np.zeros(ok.sum(), np.int32), 1, ALPHA, N_BINS, sw, aw)
    gr_all = R.gram_sums(fake_px[ok], real[ok], np.zeros(ok.sum(), np.int32), 1)
    assert ref['margin'] > 1e-9
    assert np.array_equal(_np(one['hist']), ref['hist'])
    assert np.array_equal(_np(one['counts'])[:-1].reshape(-1, 3), ref['counts'])
    rng = np.random.default_rng(6)
    for name, rf, g_, s, sel in ((0, ref, gr, 0, style == 0), (2, ref, gr, 2, style == 2), ('all', ref_all, gr_all, 0, ok)):
        m = res[name]
        n_clips, n_frames, hits = rf['counts'][s]
        assert m['pck'] == hits / (n_frames * K) and m['n_frames'] == n_frames
        b0 = np.flatnonzero(sel)[0]
        lead = [abs(float(fake_px[b0, 0, 0]) - float(real[b0, 0, 0])), rf['speed'][0][0, 0] if name == 'all' else
                ref['speed'][0][b0, 0], rf['speed'][1][0, 0] if name == 'all' else ref['speed'][1][b0, 0]]
        div = np.array([n_frames * 2 * K, n_clips * (T - 1), n_clips * (T - 1)], np.float64)
        _check_sum(f'{name} l1 / mean speeds', np.array([m['l1'], m['mean_speed_real'], m['mean_speed_fake']]) * div,
                   rf['sums'][s], rf['n_terms'][s], rf['abs_sums'][s], lead)
        fd, bound = _fd_bound(g_, s, np.stack([real[b0, 0], fake_px[b0, 0]]), rng, name)
        print(f'POSE-EVAL {name} fd err {abs(m["fd"] - fd):.3e} (bound {bound:.3e})')
        assert abs(m['fd'] - fd) <= bound
        if name == 'all':
            assert abs(want['fd'] - fd) <= bound


# ------------------------------------------------------------------------------ the loader
SPEAKERS = ['seth', 'oliver']     # A, B speak as oliver (style 1), C, D as seth (style 0)
ARR = P.arrays()


def _loader(batch_size=4):
    from a2m.data import PatsLoader
    table = [P.row('test', i, 'oliver' if i in 'AB' else 'seth') for i in 'ABCD']
    return PatsLoader(ARR, table, SPEAKERS, time=P.TIME, fs_new=P.FS_NEW, window_hop=5, shuffle=False, device=DEV,
                      batch_size=batch_size)


def test_pairs_with_style_yields_the_styles_of_test():
    loader = _loader()
    dicts = list(loader.test)
    plain = list(loader.pairs('test', copy=True))
    styled = list(loader.pairs('test', copy=True, with_style=True))
    assert len(dicts) == len(plain) == len(styled) == 4
    seen = set()
    for d, p, s in zip(dicts, plain, styled):
        assert len(p) == 2 and len(s) == 3
        assert torch.equal(p[0], s[0]) and torch.equal(p[1], s[1])
        assert s[2].dtype == torch.int32 and s[2].is_cuda and s[2].shape == (len(p[0]),)
        assert torch.equal(s[2].float(), d['style'][:, 0])
        seen |= set(s[2].tolist())
    assert seen == {0, 1}
    reused = [s.data_ptr() for _, _, s in loader.pairs('test', with_style=True)]
    assert reused[0] == reused[1] == reused[2] != reused[3]


# ------------------------------------------------------------------------------ end to end
def _stats(seed=11):
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    return [torch.from_numpy(a).to(DEV) for a in (pm, ps, am, asd)]


E2E = dict(n_bins=N_BINS, speed_max=SPEED_MAX, accel_max=ACCEL_MAX)


def test_evaluation_pass_does_not_synchronise():
    """What evaluate() loops over -- the loader's batches with styles, the generator in eval mode under
    no_grad, PoseEvaluator.update -- under torch's sync debug mode 'error' from after iter() (the draw and
    the one upload, as tests/test_gpu_data.py has it) up to result(), after a first pass has created the
    buffers and code objects.  The two passes leave equal accumulators."""
    from a2m.evaluation import PoseEvaluator
    g, _ = _models(DEV)
    g.eval()
    loader = _loader()
    pm, ps, am, asd = _stats()
    ev = PoseEvaluator(pm, ps, 2, device=DEV, **E2E)
    pairs = loader.pairs('test', torch.zeros_like(pm), torch.ones_like(ps), am, asd, with_style=True)
    with torch.no_grad():
        for audio, real, style in pairs:
            ev.update(g(audio)[0], real, style)
    first = {k: v.clone() for k, v in ev.state().items()}
    ev.reset()
    it = iter(pairs)
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
            with torch.no_grad():
                n = 0
                for audio, real, style in it:
                    ev.update(g(audio)[0], real, style)
                    n += 1
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("the installed ROCm torch does not honour torch.cuda.set_sync_debug_mode('error')")
    assert n == 4
    res = ev.result()
    assert res['all']['n_clips'] == 13 and res['dropped'] == 0
    for k, v in ev.state().items():
        assert torch.equal(v, first[k]), k


def test_evaluate_end_to_end():
    """evaluate() on the real generator over a 13-clip test split of two speakers (batches of 4, 4, 4, 1)
    against eval_ref fed from the public ops: generator(audio) read back, denormalize, the loader's own
    batches and styles.  Integer metrics are exact; pck / l1 / mean speeds fall under the sum rule; w1 is
    exact given exact histograms (the same host function); the entries are keyed by speaker name, and
    'all' is held to the reference pooled as one style.

    fd is held to _fd_bound: 4 x the largest shift under a perturbation of the reference sums by their
    own tolerance.  Measured with these inputs (MI355X generator output, the shifts on the CPU), relative to
    fd of about 5e5: seth (9 clips over at most 175 distinct frames, full-rank covariances) largest shift 7.9e-12,
    error 2.7e-15; oliver (4 clips over at most 80 distinct frames, rank-deficient, where the matrix square root
    is sensitive) shift 2.2e-9, error 0; all shift 7.7e-12, error 9.2e-12 (bound 3.1e-11); leaving one
    frame out moves fd by 4e-4 to 3e-3."""
    from a2m.evaluation import METRICS, evaluate, w1_from_histograms
    from a2m.normalization import denormalize
    g, _ = _models(DEV)
    loader = _loader()
    pm, ps, am, asd = _stats()
    got = evaluate(g, loader, 'test', pose_mean=pm, pose_std=ps, audio_mean=am, audio_std=asd, **E2E)
    assert all(m.training for m in g.modules())            # the training flags are back
    assert sorted(got) == ['all', 'dropped', 'oliver', 'seth'] and got['dropped'] == 0
    assert all(sorted(got[k]) == sorted(METRICS) for k in ('all', 'oliver', 'seth'))
    # the reference, from the public ops
    fakes, reals, styles = [], [], []
    g.eval()
    with torch.no_grad():
        zero, one = torch.zeros_like(pm), torch.ones_like(ps)
        for (audio, real, style), d in zip(loader.pairs('test', zero, one, am, asd, with_style=True), loader.test):
            fakes.append(_np(denormalize(g(audio)[0], pm, ps)))
            reals.append(_np(real))
            styles.append(_np(style))
            assert np.array_equal(_np(real), P.necksub(_np(d[P.POSE])))
    fake_px, real, style = np.concatenate(fakes), np.concatenate(reals), np.concatenate(styles)
    assert len(style) == 13 and fake_px.dtype == np.float32 and set(style.tolist()) == {0, 1}
    K, S, T = 52, 2, 64
    sw, aw = SPEED_MAX / N_BINS, ACCEL_MAX / N_BINS
    one_style = np.zeros_like(style)
    per = R.clip_metrics(fake_px, real, style, S, ALPHA, N_BINS, sw, aw)
    pooled = R.clip_metrics(fake_px, real, one_style, 1, ALPHA, N_BINS, sw, aw)
    assert per['margin'] > 1e-9, 'the reference sits on a threshold: draw other weights'
    gper, gpool = R.gram_sums(fake_px, real, style, S), R.gram_sums(fake_px, real, one_style, 1)
    rng = np.random.default_rng(5)
    for name, ref, gr, s in (('seth', per, gper, 0), ('oliver', per, gper, 1), ('all', pooled, gpool, 0)):
        m = got[name]
        n_clips, n_frames, hits = ref['counts'][s]
        assert (m['n_clips'], m['n_frames']) == (n_clips, n_frames) and n_frames == n_clips * T > 0
        assert m['pck'] == hits / (n_frames * K)
        h = ref['hist'][s]
        assert m['w1_speed'] == w1_from_histograms(h[0], h[1], sw) and m['w1_accel'] == w1_from_histograms(h[2], h[3], aw)
        assert m['speed_overflow'] == h[:2, -1].sum() / h[:2].sum() and m['accel_overflow'] == h[2:, -1].sum() / h[2:].sum()
        sel = (style == s) if name != 'all' else np.ones_like(style, bool)
        b0 = np.flatnonzero(sel)[0]
        lead = [abs(float(fake_px[b0, 0, 1]) - float(real[b0, 0, 1])), per['speed'][0][b0, 0], per['speed'][1][b0, 0]]
        div = np.array([n_frames * 2 * K, n_clips * (T - 1), n_clips * (T - 1)], np.float64)
        _check_sum(f'{name} l1 / mean speeds', np.array([m['l1'], m['mean_speed_real'], m['mean_speed_fake']]) * div,
                   ref['sums'][s], ref['n_terms'][s], ref['abs_sums'][s], lead)
        fd, bound = _fd_bound(gr, s, np.stack([real[b0, 0], fake_px[b0, 0]]), rng, name)
        print(f'POSE-EVAL {name} fd err {abs(m["fd"] - fd):.3e} (bound {bound:.3e})')
        assert abs(m['fd'] - fd) <= bound
