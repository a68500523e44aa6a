"""The sample-level set metrics on the device (csrc/coverage.hip, a2m.evaluation.CoverageEvaluator, DESIGN.md
7.12) against tests/coverage_ref.py.

Distances, exact: integer-valued floats with |x| <= 8 (16 for frame differences) at D <= 832: every product
and partial sum is an integer below 2^24, exact in fp32 in any order, so the slab must equal the integer
distances bit for bit, and so must every radius, count and flag derived from it.

Distances, floats: |a|^2, |b|^2 and a.b are each an fp32 sum of D terms (an fma chain, or chains and a tree),
each within D 2^-24 of the sum of its terms' magnitudes, and |a.b| <= (|a|^2 + |b|^2) / 2, so the computed
(|a|^2 + |b|^2) - 2 a.b is within tol(a,b) = 4 D 2^-24 (|a|^2 + |b|^2) of the exact value.

Counts and flags on floats are held to an interval, not excluded: a comparison d2(a,b) <= r_k2(b) is decided
wrongly only within m(a,b) = tol(a,b) + max_j tol(b,j) of equality (the second term bounds the radius's own
error: the k-th smallest of perturbed values is within the largest perturbation of the true k-th smallest).
Each device count must lie between #{d2 <= r2 - m} and #{d2 <= r2 + m} of the float64 reference, each flag
may differ only where those two disagree, and the inputs must keep the undecided pairs under 0.5 % and the
rows with an undecided flag under 5 % per direction (asserted on the reference alone, before comparing).

The selection and the row passes are exact: compared with numpy on the same float32 values, the fp64 row sums
within n 2^-52 relative of math.fsum (n correctly rounded roots, each lane's chain and a six-step tree)."""
import math

import numpy as np
import pytest
import torch

import coverage_ref as R
import pats_data_ref as P

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)
CANARY = -7777.25
INF = np.float32(np.inf)


def _np(t):
    return t.detach().cpu().numpy()


def _dev(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _canaried(n, dtype=torch.float32, pad=64):
    """A view of n elements inside a canary-filled buffer, and the check that the rest kept the canary."""
    buf = torch.full((n + 2 * pad,), CANARY if dtype.is_floating_point else -7777, dtype=dtype, device=DEV)
    keep = buf.clone()

    def check():
        assert torch.equal(buf[:pad], keep[:pad]) and torch.equal(buf[pad + n:], keep[pad + n:])
    return buf[pad:pad + n], check


# ------------------------------------------------------------------------------ pair_dist2, exact
DIMS = [4, 60, 64, 68, 104, 728, 832]       # below the 64-float chunk, one chunk, 1 + 4, 1 + 40, 11 x 64 + 24, 13 x 64
SIZES = [(1, 65), (63, 64), (64, 130), (65, 63), (130, 1)]
CAP = 140
_INT = {}


def _int_case(D):
    if D not in _INT:
        g = np.random.default_rng(100 + D)
        fa, fb = (g.integers(-8, 9, (CAP, D)).astype(np.float32) for _ in range(2))
        _INT[D] = (fa, fb, *_dev(fa, fb))
    return _INT[D]


def _row_list(kind, n, g):
    if kind == 'perm':
        return g.permutation(CAP)[:n].astype(np.int32)
    if kind == 'stride':
        return ((3 + 2 * np.arange(n)) % CAP).astype(np.int32) if n <= CAP // 2 else (np.arange(n) + 5).astype(np.int32)
    return g.integers(0, 7, n).astype(np.int32) * 19                   # 'repeat': seven rows, each many times


@pytest.mark.parametrize('nA,nB', SIZES)
@pytest.mark.parametrize('D', DIMS)
def test_pair_dist2_exact_on_integers(D, nA, nB):
    from a2m import functional as F
    fa, fb, da, db = _int_case(D)
    g = np.random.default_rng(D * 1000 + nA)
    kinds = ['perm', 'stride', 'repeat']
    ka, kb = kinds[(D + nA) % 3], kinds[(D + nB + 1) % 3]
    ra, rb = _row_list(ka, nA, g), _row_list(kb, nB, g)
    ref = R.dist2(fa[ra], fb[rb])
    assert ref.max() < 2 ** 24 and np.array_equal(ref, np.round(ref))
    out, check = _canaried(nA * nB)
    got = F.pair_dist2(da, *_dev(ra), db, *_dev(rb), out=out.view(nA, nB))
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(_np(got).astype(np.float64), ref)
    check()
    if nA > nB:
        return
    # one set against itself: rows_a the sub-list of rows_b at diag0; the diagonal is +inf by position,
    # a repeated row elsewhere in the list is a neighbour at exactly 0
    diag0 = nB - nA
    ref = R.dist2(fb[rb[diag0:]], fb[rb])
    ref[np.arange(nA), diag0 + np.arange(nA)] = np.inf
    out, check = _canaried(nA * nB)
    drb, = _dev(rb)
    got = _np(F.pair_dist2(db, drb[diag0:], db, drb, True, diag0, out.view(nA, nB))).astype(np.float64)
    assert np.array_equal(got, ref)
    check()
    if kb == 'repeat' and nB > 8:
        assert (got == 0).any()


def test_pair_dist2_reads_no_row_outside_the_buffers():
    """Row numbers outside [0, cap) are read as the nearest valid row."""
    from a2m import functional as F
    fa, fb, da, db = _int_case(104)
    ra = np.array([-5, 0, CAP - 1, CAP + 3, 2 ** 31 - 1, -2 ** 31], np.int32)
    got = _np(F.pair_dist2(da, *_dev(ra), db, *_dev(ra)))
    clamp = np.clip(ra.astype(np.int64), 0, CAP - 1)
    assert np.array_equal(got.astype(np.float64), R.dist2(fa[clamp], fb[clamp]))


# ------------------------------------------------------------------------------ pair_dist2, floats
@pytest.mark.parametrize('D', [4, 104, 728, 832])
def test_pair_dist2_floats_within_the_sum_bound(D):
    from a2m import functional as F
    g = np.random.default_rng(7 + D)
    a, b = g.standard_normal((130, D)).astype(np.float32), g.standard_normal((66, D)).astype(np.float32)
    b[65] = a[3]                                                       # an identical clip: within tol of 0
    ra, rb = np.arange(130, dtype=np.int32), np.arange(66, dtype=np.int32)
    da, db, dra, drb = _dev(a, b, ra, rb)
    got = _np(F.pair_dist2(da, dra, db, drb))
    ref, tol = R.dist2(a, b), R.tol(a, b)
    err = np.abs(got.astype(np.float64) - ref)
    print(f'COVERAGE pair_dist2 floats D={D}: worst err / tol = {(err / tol).max():.3e}, d2(x, x) = {got[3, 65]:.3e} '
          f'(tol {tol[3, 65]:.3e})')
    assert (got >= 0).all() and np.all(err <= tol)
    # a function of the two vectors alone: the transposed slab, and equal vectors wherever they sit
    back = _np(F.pair_dist2(db, drb, da, dra))
    assert np.array_equal(back.T, got)
    rep = np.array([3, 77, 3, 129, 77], np.int32)
    again = _np(F.pair_dist2(da, *_dev(rep), db, drb))
    assert np.array_equal(again, got[rep])


# ------------------------------------------------------------------------------ the row passes
WIDTHS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 4096, 4097]
N_ROWS = 9                                   # three workgroups of four waves, the last with one


def _slab_rows(nB, seed):
    """Nine rows of non-negative floats: squared normals, heavy ties, all equal, one +inf (a row's own
    place), many +inf, zeros and subnormals, a row of zeros, large values, small integers."""
    g = np.random.default_rng(seed)
    rows = [g.standard_normal(nB) ** 2, g.integers(0, 4, nB), np.full(nB, 2.5), g.random(nB) * 50,
            np.where(g.random(nB) < 0.5, np.inf, g.random(nB)), g.integers(0, 3, nB) * 1e-42, np.zeros(nB),
            g.random(nB) * 1e30, g.integers(0, 40, nB)]
    slab = np.stack(rows).astype(np.float32)
    slab[3, g.integers(0, nB)] = INF
    assert slab.shape == (N_ROWS, nB) and (slab >= 0).all()
    return slab


@pytest.mark.parametrize('nB', WIDTHS)
def test_row_kth_and_sums(nB):
    from a2m import functional as F
    slab = _slab_rows(nB, nB)
    ds, = _dev(slab)
    assert (slab[5] > 0).sum() == 0 or slab[5][slab[5] > 0].max() < 1.2e-38    # subnormals
    order = np.sort(slab, axis=1)
    for k in (1, 3, 8, 32):
        if k > nB:
            with pytest.raises(ValueError, match='row_kth'):
                F.row_kth(ds, k)
            continue
        kth, ck = _canaried(N_ROWS)
        sums, cs = _canaried(N_ROWS, torch.float64)
        F.row_kth(ds, k, False, kth, sums)
        got, gs = _np(kth), _np(sums)
        ck()
        cs()
        assert np.array_equal(got.view(np.uint32), order[:, k - 1].view(np.uint32)), (k, got, order[:, k - 1])
        for r in range(N_ROWS):
            want = math.fsum(math.sqrt(float(v)) for v in slab[r] if np.isfinite(v))
            assert abs(gs[r] - want) <= nB * 2.0 ** -52 * want, (r, gs[r], want)
    if nB <= 32:                                                       # exclude_self only limits k: k < nB
        with pytest.raises(ValueError, match='row_kth'):
            F.row_kth(ds, nB, True)


@pytest.mark.parametrize('nB', WIDTHS)
def test_row_cover(nB):
    from a2m import functional as F
    slab = _slab_rows(nB, 50 + nB)
    g = np.random.default_rng(nB)
    for r2 in (slab[g.integers(0, N_ROWS, nB), np.arange(nB)], np.full(nB, 2.5, np.float32),
               np.zeros(nB, np.float32), np.full(nB, INF)):
        count, cc = _canaried(N_ROWS, torch.int32)
        low, cl = _canaried(N_ROWS)
        F.row_cover(*_dev(slab, r2), count, low)
        cc()
        cl()
        assert np.array_equal(_np(count), (slab <= r2[None, :]).sum(1))
        assert np.array_equal(_np(low).view(np.uint32), slab.min(1).view(np.uint32))


# ------------------------------------------------------------------------------ the evaluator, exact
N_STYLES, K = 3, 3
BATCHES = (16, 16, 13)


def _int_clips(T, Fd, seed):
    """45 clips in batches of 16, 16, 13 whose normalised values are small integers: the real clips in [-3, 3],
    a generated clip a real clip of its own speaker plus integer noise in [-1, 1] whose density grows with
    the clip (from a near copy to something far off), five generated clips one repeated clip.  real_px = v
    std + mean with std a power of two and mean an integer, so that (real_px - mean) / std is v exactly.
    Styles: 27 clips of speaker 0, 15 of speaker 1, 2 of speaker 2 (fewer than k + 1: NaN), 1 out of range."""
    g = np.random.default_rng(seed)
    n = sum(BATCHES)
    style = np.array([0] * 27 + [1] * 15 + [2] * 2 + [7], np.int32)[g.permutation(n)]
    v = g.integers(-3, 4, (n, T, Fd)).astype(np.float32)
    fake = np.empty_like(v)
    for i in range(n):
        src = g.choice(np.flatnonzero(style == style[i]))
        fake[i] = v[src] + g.integers(-1, 2, (T, Fd)) * (g.random((T, Fd)) < (i + 1) / n)
    fake[g.permutation(n)[:5]] = fake[0]
    mean = g.integers(-40, 41, Fd).astype(np.float32)
    std = (2.0 ** g.integers(0, 5, Fd)).astype(np.float32)
    std[1] = 1e-8                                                      # below the guard: divides by 1
    real_px = (v * np.where(std < 1e-7, 1, std) + mean).astype(np.float32)
    assert np.array_equal(R.standardise(real_px, mean, std), v)
    return fake, real_px, style, mean, std


def _feed(ev, fake, real_px, style):
    b0 = 0
    for n in BATCHES:
        ev.update(*_dev(fake[b0:b0 + n], real_px[b0:b0 + n], style[b0:b0 + n]))
        b0 += n


def _same(a, b):
    return a == b or (isinstance(a, float) and math.isnan(a) and math.isnan(b))


@pytest.mark.parametrize('T,feature,block_rows', [(8, 'pose', 4096), (8, 'pose', 16), (8, 'motion', 4096),
                                                  (2, 'motion', 10)])
def test_evaluator_exact_on_integers(T, feature, block_rows):
    """D = 832, 728 and 104.  Every distance is an exact integer on both sides, so the radii, the counts, the
    flags and with them precision, recall, density and coverage equal the reference's; the diversities are
    fp64 sums of the same correctly rounded roots in another order, held to 1e-13 relative.  block_rows 16 and
    10: slabs of a set's rows 0..15, 16..31, ..., the diagonal at an offset."""
    from a2m.evaluation import COVERAGE_METRICS, CoverageEvaluator
    fake, real_px, style, mean, std = _int_clips(T, 104, 40 + T)
    ev = CoverageEvaluator(mean, std, N_STYLES, 48, T, k=K, feature=feature, device=DEV, block_rows=block_rows)
    _feed(ev, fake, real_px, style)
    G, Rr = R.features(fake, real_px, mean, std, feature)
    st = ev.state()
    assert st['n'] == 45 and np.array_equal(_np(st['feat_fake']), G) and np.array_equal(_np(st['feat_real']), Rr)
    assert np.array_equal(_np(st['styles']), style) and G.shape[1] == ev.D == (T - (feature == 'motion')) * 104
    got, rows = ev.result(per_row=True)
    want = R.by_style(G, Rr, style, N_STYLES, K)
    assert sorted(got, key=str) == [0, 1, 2, 'all'] and sorted(rows, key=str) == [0, 1, 'all']
    for key in want:
        assert sorted(got[key]) == sorted(COVERAGE_METRICS)
        for name in COVERAGE_METRICS:
            if name.startswith('diversity') and not math.isnan(want[key][name]):
                assert got[key][name] == pytest.approx(want[key][name], rel=1e-13), (key, name)
            else:
                assert _same(got[key][name], want[key][name]), (key, name, got[key][name], want[key][name])
    assert got[2]['n_coverage'] == 2 and math.isnan(got[2]['recall']) and got['all']['n_coverage'] == 44
    assert 0 < got['all']['recall'] < 1 and 0 < got['all']['coverage'] < 1 and got['all']['density'] > 0
    sel = np.flatnonzero((style >= 0) & (style < N_STYLES))
    c = R.counts(G[sel], Rr[sel], K)
    assert np.array_equal(rows['all']['rows'], sel)
    assert np.array_equal(rows['all']['kth_real'].astype(np.float64), c['r2_real'])
    assert np.array_equal(rows['all']['kth_fake'].astype(np.float64), c['r2_fake'])
    assert np.array_equal(rows['all']['cnt_prec'], c['cnt_prec']) and np.array_equal(rows['all']['cnt_rec'], c['cnt_rec'])
    assert np.array_equal(rows['all']['min_rg'].astype(np.float64), c['d_gr'].min(0))


def test_evaluator_twice_capacity_and_no_synchronisation():
    """Two passes (reset() in between) leave byte-identical state() and result(); a pass of update() runs under
    torch's sync debug mode 'error'; an update beyond capacity raises before any launch."""
    from a2m.evaluation import CoverageEvaluator
    fake, real_px, style, mean, std = _int_clips(8, 104, 48)
    fake = (fake + 0.37 * np.random.default_rng(2).standard_normal(fake.shape)).astype(np.float32)   # floats
    ev = CoverageEvaluator(mean, std, N_STYLES, 45, 8, k=K, device=DEV)
    _feed(ev, fake, real_px, style)
    first = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in ev.state().items()}
    res = ev.result()
    with pytest.raises(ValueError, match='capacity'):
        ev.update(*_dev(fake[:1], real_px[:1], style[:1]))
    ev.reset()
    assert ev.state()['n'] == 0
    batches, b0 = [], 0
    for n in BATCHES:
        batches.append(_dev(fake[b0:b0 + n], real_px[b0:b0 + n], style[b0:b0 + n]))
        b0 += n
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
            for b in batches:
                ev.update(*b)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("the installed ROCm torch does not honour torch.cuda.set_sync_debug_mode('error')")
    second = ev.state()
    assert second['n'] == first['n'] == 45
    for name in ('feat_fake', 'feat_real', 'styles'):
        assert torch.equal(first[name], second[name]), name
    again = ev.result()
    assert repr(again) == repr(res)
    # beyond capacity: refused on the host, the buffers and the count stay
    with pytest.raises(ValueError, match='capacity'):
        ev.update(*batches[0])
    assert ev.state()['n'] == 45 and torch.equal(ev.state()['feat_fake'], first['feat_fake'])
    with pytest.raises(ValueError, match='built for'):
        ev.update(*_dev(fake[:2, :4], real_px[:2, :4], style[:2]))


# ------------------------------------------------------------------------------ floats: the interval
def _device_rows(G, Rr, k, block=64):
    """What CoverageEvaluator.result() runs, on two sets of any sizes through the public ops, in blocks of
    `block` rows: the radii of both sets, the counts of both directions and the R|G minima."""
    from a2m import functional as F
    dg, dr = _dev(G, Rr)
    rows_g, rows_r = (torch.arange(len(x), dtype=torch.int32, device=DEV) for x in (G, Rr))
    out = {}
    for name, feat, rows in (('real', dr, rows_r), ('fake', dg, rows_g)):
        kth, sums = torch.empty(len(rows), device=DEV), torch.empty(len(rows), dtype=torch.float64, device=DEV)
        for a0 in range(0, len(rows), block):
            slab = F.pair_dist2(feat, rows[a0:a0 + block], feat, rows, True, a0)
            F.row_kth(slab, k, True, kth[a0:a0 + block], sums[a0:a0 + block])
        out['r2_' + name], out['sum_' + name] = kth, sums
    for name, fa, ra, fb, rb, r2 in (('prec', dg, rows_g, dr, rows_r, out['r2_real']),
                                     ('rec', dr, rows_r, dg, rows_g, out['r2_fake'])):
        cnt, low = torch.empty(len(ra), dtype=torch.int32, device=DEV), torch.empty(len(ra), device=DEV)
        for a0 in range(0, len(ra), block):
            F.row_cover(F.pair_dist2(fa, ra[a0:a0 + block], fb, rb), r2, cnt[a0:a0 + block], low[a0:a0 + block])
        out['cnt_' + name], out['min_' + name] = cnt, low
    return {k_: _np(v) for k_, v in out.items()}


def _diversity_bound(X):
    """(sum of sqrt d2 over the ordered pairs of X, its bound): each root is off by at most
    tol / (sqrt d2 + sqrt max(d2 - tol, 0))."""
    dd, t = R.dist2(X, X), R.tol(X, X)
    off = ~np.eye(len(X), dtype=bool)
    bound = (t[off] / (np.sqrt(dd[off]) + np.sqrt(np.maximum(dd[off] - t[off], 0)))).sum()
    return float(np.sqrt(dd[off]).sum()), float(bound)


def _interval_check(name, G, Rr, k, got):
    """got: the per-row vectors of the device (cnt_prec [nG], cnt_rec [nR], min_rg [nR], kth_real [nR], sum_real,
    sum_fake).  The caps on the inputs first, on the reference alone; then the intervals."""
    d = R.dist2(G, Rr)                                                 # [nG, nR]
    t_gr, t_rr, t_gg = R.tol(G, Rr), R.tol(Rr, Rr), R.tol(G, G)
    r2_real, r2_fake = R.radii(R.dist2(Rr, Rr), k), R.radii(R.dist2(G, G), k)
    flags = {}
    for key, dist, r2, m in (('prec', d, r2_real, t_gr + t_rr.max(1)[None, :]),
                             ('rec', d.T, r2_fake, t_gr.T + t_gg.max(1)[None, :])):
        lo, hi = dist <= r2[None, :] - m, dist <= r2[None, :] + m
        undecided = int((lo != hi).sum())
        flag_open = lo.any(1) != hi.any(1)
        print(f'COVERAGE {name} {key}: {undecided} undecided pairs of {lo.size}, {int(flag_open.sum())} undecided '
              f'flags of {len(flag_open)}')
        assert undecided <= 0.005 * lo.size and flag_open.sum() <= 0.05 * len(flag_open), 'the inputs are too close to call'
        cnt = got['cnt_' + key]
        assert np.all(lo.sum(1) <= cnt) and np.all(cnt <= hi.sum(1)), key
        assert np.array_equal((cnt > 0)[~flag_open], lo.any(1)[~flag_open]), key
        flags[key] = (lo.any(1), hi.any(1))
    # coverage: min_g d2(r,g) <= r_k2(r); the minimum is off by at most its row's largest tolerance
    m = t_gr.max(0) + t_rr.max(1)
    low = d.min(0)
    lo, hi = low <= r2_real - m, low <= r2_real + m
    print(f'COVERAGE {name} coverage: {int((lo != hi).sum())} undecided of {len(lo)}')
    assert (lo != hi).sum() <= 0.05 * len(lo)
    covered = got['min_rg'] <= got['kth_real']
    assert np.array_equal(covered[lo == hi], lo[lo == hi])
    assert np.all(np.abs(got['min_rg'] - low) <= t_gr.max(0)) and np.all(np.abs(got['kth_real'] - r2_real) <= t_rr.max(1))
    # diversity: each root is off by at most tol / (sqrt d2 + sqrt max(d2 - tol, 0))
    for key, X in (('real', Rr), ('fake', G)):
        total, bound = _diversity_bound(X)
        err = abs(float(np.sum(got['sum_' + key])) - total)
        print(f'COVERAGE {name} diversity_{key}: sum err {err:.3e}, bound {bound:.3e}')
        assert err <= bound
    return (flags['prec'], flags['rec']), (lo, hi)


def _recipe(variant):
    g = np.random.default_rng(1)
    Rr = g.standard_normal((150, 832)).astype(np.float32)
    G = g.standard_normal((130, 832)).astype(np.float32)
    if variant == 'near':
        G = (Rr[g.integers(0, 150, 130)] + np.float32(0.7) * G).astype(np.float32)
    elif variant == 'collapsed':
        G = (np.float32(0.05) * G).astype(np.float32)
    return G, Rr


@pytest.mark.parametrize('variant', ['independent', 'near', 'collapsed'])
def test_counts_and_flags_on_floats_lie_in_the_interval(variant):
    """default_rng(1): R = standard_normal((150, 832)), then G = standard_normal((130, 832)), k = 3; and G = R[idx]
    + 0.7 noise (near the real clips) and G = 0.05 noise (collapsed at the origin)."""
    G, Rr = _recipe(variant)
    got = _device_rows(G, Rr, 3)
    got = dict(got, kth_real=got['r2_real'], min_rg=got['min_rec'])
    (prec, rec), cov = _interval_check(variant, G, Rr, 3, got)
    p = float((got['cnt_prec'] > 0).mean())
    print(f'COVERAGE {variant}: precision {p:.3f}, recall {float((got["cnt_rec"] > 0).mean()):.3f}')
    assert prec[0].mean() <= p <= prec[1].mean()
    if variant == 'collapsed':
        assert not (got['cnt_rec'] > 0).any()                          # no real clip inside a collapsed ball


def test_evaluator_on_floats_lies_in_the_interval():
    """CoverageEvaluator on float clips (T = 8, D = 832), 150 clips of one speaker in batches of 64, 64, 22:
    the real clips standard normal after normalisation, the generated ones near real clips."""
    from a2m.evaluation import CoverageEvaluator
    g = np.random.default_rng(11)
    mean = (g.standard_normal(104) * 30).astype(np.float32)
    std = (g.random(104) * 50 + 5).astype(np.float32)
    real_px = (g.standard_normal((150, 8, 104)) * std + mean).astype(np.float32)
    fake = (R.standardise(real_px, mean, std)[g.permutation(150)] + 0.7 * g.standard_normal((150, 8, 104))).astype(np.float32)
    style = np.zeros(150, np.int32)
    ev = CoverageEvaluator(mean, std, 1, 150, 8, k=3, device=DEV, block_rows=64)
    for b0 in (0, 64, 128):
        ev.update(*_dev(fake[b0:b0 + 64], real_px[b0:b0 + 64], style[b0:b0 + 64]))
    res, rows = ev.result(per_row=True)
    G, Rr = R.features(fake, real_px, mean, std)
    (prec, rec), (clo, chi) = _interval_check('evaluator', G, Rr, 3, rows[0])
    m = res[0]
    assert res['all'] == m and m['n_coverage'] == 150
    assert prec[0].mean() <= m['precision'] <= prec[1].mean() and rec[0].mean() <= m['recall'] <= rec[1].mean()
    assert clo.mean() <= m['coverage'] <= chi.mean()
    assert m['density'] == rows[0]['cnt_prec'].sum() / (3 * 150)
    assert m['diversity_real'] == float(np.sum(rows[0]['sum_real'])) / (150 * 149)


# ------------------------------------------------------------------------------ evaluate()
SPEAKERS = ['seth', 'oliver']
LENGTHS = {'A': 40, 'B': 23, 'C': 31, 'D': 50, 'E': 36}                # pose rows; six audio rows a pose row
TIME = 0.54                                                            # 8 pose rows, 48 audio rows at interval 6


class _Scaled(torch.nn.Module):
    """A generator for the test: the first 104 audio columns, scaled; a float function of the audio."""

    def forward(self, audio, real_pose=None):
        return (audio[..., :104] * 0.5 + 1.0).contiguous(), None


def _loader(batch_size=4):
    """Test: A (oliver, 7 clips), B and C (seth, 3 + 5): batches of 4, 4, 4, 3.  Train: D (oliver), E (seth)."""
    from a2m.data import PatsLoader
    g = np.random.default_rng(21)
    arr = {i: {P.POSE: (g.standard_normal((n, 104)) * 40 + 300).astype(np.float32),
               P.AUDIO: (g.standard_normal((6 * n, 128)) * 2 - 4).astype(np.float32)} for i, n in LENGTHS.items()}
    table = [P.row('test' if i in 'ABC' else 'train', i, 'oliver' if i in 'AD' else 'seth') for i in LENGTHS]
    return PatsLoader(arr, table, SPEAKERS, time=TIME, fs_new=P.FS_NEW, window_hop=5, shuffle=False, device=DEV,
                      batch_size=batch_size)


def _stats(seed=11):
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    return _dev(pm, ps, am, asd)


def _equal_entries(a, b, keys):
    for k in keys:
        x, y = a[k], b[k]
        assert (np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)), k


def test_evaluate_default_is_untouched_and_coverage_merges(monkeypatch):
    """evaluate() without coverage= constructs and launches nothing of the feature (its entry points raise
    while it runs) and returns METRICS alone; with coverage=True every other metric keeps its bits, and the
    coverage metrics equal a CoverageEvaluator fed the loader's batches by hand, which is checked against the
    float64 reference's intervals above and here by its clip counts."""
    from a2m import evaluation as E
    from a2m import functional as F
    loader = _loader()
    pm, ps, am, asd = _stats()
    gen = _Scaled()
    kw = dict(pose_mean=pm, pose_std=ps, audio_mean=am, audio_std=asd)
    with_cov = E.evaluate(gen, loader, 'test', coverage=True, coverage_kwargs=dict(k=2), **kw)

    def boom(*a, **k):
        raise AssertionError('the default path touched the coverage feature')
    with monkeypatch.context() as mp:
        for name in ('coverage_store', 'pair_dist2', 'row_kth', 'row_cover'):
            mp.setattr(F, name, boom)
        mp.setattr(E, 'CoverageEvaluator', boom)
        plain = E.evaluate(gen, loader, 'test', **kw)
    assert sorted(plain) == sorted(with_cov) == ['all', 'dropped', 'oliver', 'seth']
    for who in ('all', 'oliver', 'seth'):
        assert sorted(plain[who]) == sorted(E.METRICS)
        assert sorted(with_cov[who]) == sorted(E.METRICS + E.COVERAGE_METRICS)
        _equal_entries(plain[who], with_cov[who], E.METRICS)
    assert plain['dropped'] == with_cov['dropped'] == 0
    assert (with_cov['oliver']['n_coverage'], with_cov['seth']['n_coverage'], with_cov['all']['n_coverage']) == (7, 8, 15)
    ev = E.CoverageEvaluator(pm, ps, 2, 15, 8, k=2, device=DEV)
    zero, one = torch.zeros_like(pm), torch.ones_like(ps)
    fakes, reals, styles = [], [], []
    for audio, real, style in loader.pairs('test', zero, one, am, asd, with_style=True):
        ev.update(gen(audio)[0], real, style)
        fakes.append(_np(gen(audio)[0])), reals.append(_np(real)), styles.append(_np(style))
    by_hand = ev.result()
    for who, key in (('seth', 0), ('oliver', 1), ('all', 'all')):
        _equal_entries(with_cov[who], by_hand[key], E.COVERAGE_METRICS)
    G, Rr = R.features(np.concatenate(fakes), np.concatenate(reals), _np(pm), _np(ps))
    want = R.by_style(G, Rr, np.concatenate(styles), 2, 2)
    st = np.concatenate(styles)
    for who, sel in (('seth', st == 0), ('oliver', st == 1), ('all', st >= 0)):
        key = {'seth': 0, 'oliver': 1}.get(who, who)
        assert with_cov[who]['n_coverage'] == want[key]['n_coverage'] == sel.sum()
        for name, X in (('diversity_fake', G[sel]), ('diversity_real', Rr[sel])):
            total, bound = _diversity_bound(X)
            pairs = len(X) * (len(X) - 1)
            assert abs(with_cov[who][name] * pairs - total) <= bound and abs(want[key][name] * pairs - total) < 1e-6
    sync_cov = E.evaluate(gen, loader, 'test', sync=True, coverage=True, coverage_kwargs=dict(k=2), **kw)
    assert sorted(sync_cov['all']) == sorted(E.METRICS + E.SYNC_METRICS + E.COVERAGE_METRICS)
    _equal_entries(sync_cov['all'], with_cov['all'], E.METRICS + E.COVERAGE_METRICS)


def test_baselines_with_coverage():
    """evaluate_baselines(..., coverage=True): the median pose is one clip for every audio window: no real clip
    lies in a generated ball (recall 0), and as motion it is the zero vector, whose distances are exactly 0
    (tol(0, 0) = 0): diversity_fake 0.  The real clips' diversity is the same number under all three."""
    from a2m.baselines import MedianPose, evaluate_baselines
    loader = _loader()
    pm, ps, am, asd = _stats()
    gen = torch.Generator(device=DEV)
    g2 = 8 * float((MedianPose(loader, pm, ps).median_norm.double() ** 2).sum())     # |g|^2 of the median clip
    kw = dict(pose_mean=pm, pose_std=ps, audio_mean=am, audio_std=asd, coverage=True)
    for feature in ('pose', 'motion'):
        gen.manual_seed(3)
        three = evaluate_baselines(loader, 'test', generator=gen, coverage_kwargs=dict(k=2, feature=feature), **kw)
        for who in ('all', 'oliver', 'seth'):
            m = three['median'][who]
            assert m['recall'] == 0 and m['n_coverage'] == three['nearest'][who]['n_coverage']
            real = [three[b][who]['diversity_real'] for b in ('median', 'random', 'nearest')]
            assert real[0] == real[1] == real[2] > 0
            if feature == 'motion':
                assert m['diversity_fake'] == 0.0
            else:                                                      # every pair within tol(g, g) of 0
                assert m['diversity_fake'] <= math.sqrt(4 * 832 * 2.0 ** -24 * 2 * g2)
        assert three['random']['all']['diversity_fake'] > 0
