"""The float64 restatement of the evaluation metrics (tests/eval_ref.py) and the host formulas of
a2m.evaluation (frechet_distance, w1_from_histograms), without a GPU."""
import numpy as np
import pytest

import eval_ref as R
from conftest import golden


def _data(n, Fd, seed, rank=None):
    """n frames of Fd features shaped like poses: hundreds of pixels, a spread of tens, correlated."""
    g = np.random.default_rng(seed)
    mix = g.standard_normal((rank or Fd, Fd)) * 12
    return g.standard_normal((n, rank or Fd)) @ mix + g.uniform(100, 600, Fd)


def _sums(x):
    return len(x), x.sum(0), x.T @ x


@pytest.mark.parametrize('K', [52, 48])
def test_ref_pck_reproduces_the_reference_outputs(K):
    z = golden('eval_norm.npz')
    for tag, alpha in (('a02', 0.2), ('a01', 0.1)):
        assert np.array_equal(R.pck(z[f'pck{K}_pred'], z[f'pck{K}_gt'], alpha), z[f'pck{K}_{tag}']), (K, tag)


def test_frechet_distance_agrees_with_sqrtm():
    """Against the textbook form tr(S1 + S2 - 2 sqrtm(S1 S2)) with scipy's sqrtm on 104-dimensional
    data.  sqrtm of the non-symmetric product S1 S2 is itself only accurate to about
    sqrt(2^-52) ||S||, hence the 1e-7 relative bar (the two agree far better on this data)."""
    sqrtm = pytest.importorskip('scipy.linalg').sqrtm
    from a2m.evaluation import frechet_distance
    a, b = _data(900, 104, 1), _data(700, 104, 2) * 1.1 + 3.0
    got = frechet_distance(*_sums(a), *_sums(b))
    mu1, mu2 = a.mean(0), b.mean(0)
    c1, c2 = np.cov(a.T, bias=True), np.cov(b.T, bias=True)
    want = ((mu1 - mu2) ** 2).sum() + np.trace(c1) + np.trace(c2) - 2.0 * np.trace(sqrtm(c1 @ c2)).real
    print(f'EVAL frechet vs sqrtm: got {got:.12e}, want {want:.12e}, rel {abs(got - want) / want:.2e}')
    assert abs(got - want) <= 1e-7 * want
    swapped = frechet_distance(*_sums(b), *_sums(a))
    assert abs(got - swapped) <= 1e-9 * got


def test_frechet_distance_is_symmetric_and_zero_on_identical_inputs():
    """Swapping the arguments changes the order of the roundings only.  For identical inputs every
    lambda_i is sigma_i^2 and the terms cancel; an eigenvalue computed with an error of F u ||S||^2
    (u = 2^-52, the backward error of a symmetric eigensolver) has a root that is off by at most
    sqrt(F u) ||S||, so |d^2| <= 2 F sqrt(F u) ||S||_2 bounds the result, attained only by null
    directions (the rank-deficient case below); a full-rank covariance lands near u tr S."""
    from a2m.evaluation import frechet_distance
    for n, rank in ((500, None), (40, None), (300, 30)):
        a = _data(n, 104, 3, rank)
        cov = np.cov(a.T, bias=True)
        d0 = frechet_distance(*_sums(a), *_sums(a))
        bound = 2 * 104 * np.sqrt(104 * 2.0 ** -52) * np.linalg.norm(cov, 2)
        print(f'EVAL frechet self-distance n={n} rank={rank}: {d0:.3e} (bound {bound:.3e}, tr S {np.trace(cov):.3e})')
        assert np.isfinite(d0) and abs(d0) <= bound
    a, b = _data(300, 104, 4), _data(200, 104, 5)
    d_ab, d_ba = frechet_distance(*_sums(a), *_sums(b)), frechet_distance(*_sums(b), *_sums(a))
    assert d_ab > 0 and abs(d_ab - d_ba) <= 1e-9 * d_ab


def test_frechet_distance_survives_rank_deficient_input():
    """Fewer frames than features on one side, one frame (a zero covariance) on the other: no exception,
    a finite value, and with a zero covariance exactly |mu1 - mu2|^2 + tr S1."""
    from a2m.evaluation import frechet_distance
    a, one = _data(7, 104, 6), _data(1, 104, 7)
    d = frechet_distance(*_sums(a), *_sums(_data(9, 104, 8)))
    assert np.isfinite(d) and d > 0
    d1 = frechet_distance(*_sums(a), *_sums(one))
    want = ((a.mean(0) - one[0]) ** 2).sum() + np.trace(np.cov(a.T, bias=True))
    assert abs(d1 - want) <= 1e-9 * want


def test_w1_from_histograms_is_within_a_bin_of_the_exact_w1():
    """Moving every sample to its bin's centre moves it by at most width / 2, so each distribution
    moves by at most width / 2 in W1 and the distance between them by at most one width."""
    from a2m.evaluation import w1_from_histograms
    g = np.random.default_rng(9)
    width, n_bins = 64.0 / 512, 512
    for a, b in ((g.gamma(2.0, 3.0, 4000), g.gamma(3.0, 4.0, 2500)), (g.uniform(0, 60, 300), g.uniform(5, 30, 1000))):
        assert a.max() < 64 and b.max() < 64
        ha, _ = R.histogram(a, width, n_bins)
        hb, _ = R.histogram(b, width, n_bins)
        got, want = w1_from_histograms(ha, hb, width), R.w1_samples(a, b)
        print(f'EVAL w1: histogram {got:.6f}, samples {want:.6f}')
        assert abs(got - want) <= width
    assert w1_from_histograms(ha, ha, width) == 0.0
    assert np.isnan(w1_from_histograms(np.zeros(n_bins), hb, width))


def test_ref_motion_values_on_a_hand_made_clip():
    """Two joints besides the root; joint 1 moves 3 px right and 4 px up per frame (speed 5), joint 2
    accelerates along x (positions 0, 1, 4: speeds 1, 3, acceleration 2); the root's own motion is left out."""
    K = 3
    px = np.zeros((1, 3, 2 * K), np.float32)
    px[0, :, 0] = [0, 100, -50]                              # the root
    px[0, :, 1], px[0, :, K + 1] = [0, 3, 6], [0, 4, 8]
    px[0, :, 2] = [0, 1, 4]
    speed, accel = R.speed_accel(px)
    assert np.array_equal(speed, [[(5 + 1) / 2, (5 + 3) / 2]]) and np.array_equal(accel, [[(0 + 2) / 2]])
    h, gap = R.histogram([0.3, 0.5, 99.0], 0.25, 8)
    assert h.tolist() == [0, 1, 1, 0, 0, 0, 0, 1] and gap == 0.0   # 0.5 sits on an edge
