"""tests/coverage_ref.py, the float64 statement of the precision / recall / density / coverage / diversity
metrics, against cases that can be counted by hand; and the host formulas of
a2m.evaluation.CoverageEvaluator.result() against it when fed the reference's own per-row integers.

One value differs from the sentence that announced the feature: with G = R the definitions give
density = (k + 1) / k, not 1.  Every r's ball holds r's own copy in G (distance 0) and its k nearest
neighbours, k + 1 generated points, and the sum is divided by k n (Naeem et al. 2020 note the same: density
is not bounded by 1).  The definitions are what is pinned here."""
import numpy as np
import pytest

import coverage_ref as R


def _col(v):
    return np.asarray(v, np.float32)[:, None] * np.ones((1, 4), np.float32) / 2    # |a - b|^2 = (a - b)^2 in 4 columns


def test_identical_sets():
    g = np.random.default_rng(3)
    X = g.standard_normal((40, 12)).astype(np.float32)
    for k in (1, 3, 5):
        m = R.metrics(X, X, k)
        assert m['precision'] == 1 and m['recall'] == 1 and m['coverage'] == 1
        assert m['density'] == (k + 1) / k                       # no ties among normal draws
        assert m['diversity_fake'] == m['diversity_real'] > 0 and m['n_coverage'] == 40


def test_one_far_point_repeated():
    g = np.random.default_rng(4)
    X = g.standard_normal((30, 8)).astype(np.float32)
    G = np.full((30, 8), 100, np.float32)
    m = R.metrics(G, X, 3)
    assert m['precision'] == 0 and m['recall'] == 0 and m['density'] == 0 and m['coverage'] == 0
    assert m['diversity_fake'] == 0 and m['diversity_real'] > 0


def test_generated_clips_on_one_of_two_clusters():
    """R: the integers 0..9 and, far away, 1000..1004; G: 0..9 and 0.5..4.5.  Every r of the first cluster has
    its copy in G; no generated radius (2 at most) reaches the second cluster, and no r there has a generated
    clip within its own radius of 2."""
    Rr = _col(list(range(10)) + [1000, 1001, 1002, 1003, 1004])
    G = _col(list(range(10)) + [0.5, 1.5, 2.5, 3.5, 4.5])
    m = R.metrics(G, Rr, 2)
    assert m['recall'] == 10 / 15 and m['coverage'] == 10 / 15 and m['precision'] == 1


def test_points_on_a_line_counted_by_hand():
    """k = 2.  R = 0, 1, 3, 6, 10 has radii 3, 2, 3, 4, 7; G = 0.5, 2, 2.5, 7, 20 has radii 2, 1.5, 2, 5, 17.5.
    |g - r| <= r_2(r) holds for 3, 4, 4, 2, 0 of the r per g: g = 2 against r = 6 is a tie at exactly the
    radius (4 <= 4) and counts as inside.  |r - g| <= r_2(g) holds for 1, 3, 4, 2, 2 of the g per r."""
    Rr, G = _col([0, 1, 3, 6, 10]), _col([0.5, 2, 2.5, 7, 20])
    c = R.counts(G, Rr, 2)
    assert np.array_equal(c['r2_real'], np.array([3, 2, 3, 4, 7.]) ** 2)
    assert np.array_equal(c['r2_fake'], np.array([2, 1.5, 2, 5, 17.5]) ** 2)
    assert c['cnt_prec'].tolist() == [3, 4, 4, 2, 0] and c['cnt_rec'].tolist() == [1, 3, 4, 2, 2]
    assert c['d_gr'][1, 3] == c['r2_real'][3] == 16                  # the tie
    assert c['covered'].all()
    m = R.metrics(G, Rr, 2)
    assert m['precision'] == 4 / 5 and m['recall'] == 1 and m['density'] == 13 / 10 and m['coverage'] == 1
    assert m['diversity_real'] == 5.0 and abs(m['diversity_fake'] - 8.8) < 1e-15
    without_tie = R.metrics(G, _col([0, 1, 3, 6.001, 10]), 2)         # r = 6.001: g = 2 is now 4.001 > 4 away
    assert without_tie['density'] == 12 / 10


def test_self_is_left_out_by_position_not_by_value():
    Rr = _col([0, 0, 5, 9, 20])
    r2 = R.radii(R.dist2(Rr, Rr), 1)
    assert r2.tolist() == [0, 0, 16, 16, 121]                         # each 0 has the other as a neighbour at 0
    r2 = R.radii(R.dist2(Rr, Rr), 2)
    assert r2.tolist() == [25, 25, 25, 81, 225]


def test_small_sets_are_nan():
    X = _col([0, 1, 2])
    for k in (3, 4):
        m = R.metrics(X, X, k)
        assert m['n_coverage'] == 3 and all(np.isnan(m[key]) for key in R.METRICS if key != 'n_coverage')
    assert R.metrics(X, X, 2)['precision'] == 1
    by = R.by_style(X, X, np.array([0, 0, 7]), 2, 1)
    assert by[0]['n_coverage'] == 2 and by[1]['n_coverage'] == 0 and by['all']['n_coverage'] == 2
    assert by[0]['recall'] == 1 and np.isnan(by[1]['recall'])


def test_features():
    g = np.random.default_rng(5)
    fake = g.standard_normal((3, 4, 8)).astype(np.float32)
    real = (g.standard_normal((3, 4, 8)) * 40 + 300).astype(np.float32)
    mean, std = g.standard_normal(8).astype(np.float32), (g.random(8) + 0.5).astype(np.float32)
    std[2] = 1e-8                                                      # below the guard: divides by 1
    G, Rr = R.features(fake, real, mean, std)
    assert G.shape == Rr.shape == (3, 32) and np.array_equal(G, fake.reshape(3, 32))
    assert np.array_equal(Rr.reshape(3, 4, 8)[..., 2], real[..., 2] - mean[2])
    Gm, Rm = R.features(fake, real, mean, std, 'motion')
    assert Gm.shape == (3, 24) and np.array_equal(Gm.reshape(3, 3, 8)[:, 1], fake[:, 2] - fake[:, 1])
    still = np.broadcast_to(fake[:, :1], fake.shape)
    assert not R.features(still, real, mean, std, 'motion')[0].any()   # a static clip is the zero vector


@pytest.mark.parametrize('k', [1, 3])
def test_host_formulas_of_the_evaluator_match(k):
    """a2m.evaluation._coverage_metrics on the reference's own per-row vectors gives the reference's metrics:
    the device side only has to deliver the integers, the minima, the radii and the row sums."""
    from a2m.evaluation import COVERAGE_METRICS, _coverage_metrics
    assert COVERAGE_METRICS == R.METRICS
    g = np.random.default_rng(6)
    Rr = g.standard_normal((25, 16)).astype(np.float32)
    G = (Rr[g.permutation(25)] + 0.8 * g.standard_normal((25, 16))).astype(np.float32)
    c = R.counts(G, Rr, k)
    off = ~np.eye(25, dtype=bool)
    rows = [np.sqrt(np.where(off, R.dist2(X, X), 0)).sum(1) for X in (Rr, G)]
    got = _coverage_metrics(k, c['r2_real'], c['cnt_prec'], c['cnt_rec'], c['d_gr'].min(0), rows[0], rows[1])
    want = R.metrics(G, Rr, k)
    for key in R.METRICS:
        assert got[key] == pytest.approx(want[key], rel=1e-14), key
    assert 0 < want['precision'] and want['density'] > 0
    small = _coverage_metrics(3, *(np.zeros(3) for _ in range(6)))
    assert small['n_coverage'] == 3 and np.isnan(small['precision']) and np.isnan(small['diversity_real'])
