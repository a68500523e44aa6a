"""tests/baselines_ref.py checks itself (no GPU): the numpy radix select that mirrors
a2m_window_median_f32's rank logic equals np.median bit for bit (compared with ==, so -0.0 and +0.0
agree) at the sizes where the rank logic changes (one element, even / odd, one bucket boundary) and
on the value families that stress a byte-wise select; the key is order preserving; nn_distances is
the plain double loop."""
import numpy as np
import pytest

import baselines_ref as R

SIZES = [1, 2, 3, 4, 255, 256, 257]
FAMILIES = ['normal', 'equal', 'duplicates', 'zeros', 'signed_zero', 'denormal', 'low_byte', 'wide']


@pytest.mark.parametrize('M', SIZES)
@pytest.mark.parametrize('family', FAMILIES)
def test_radix_select_equals_numpy_median(family, M):
    x = R.value_families(M)[family]
    got = R.radix_select_median(x)
    ref = R.median(x[:, None])[0]
    assert got.dtype == np.float32 and np.isfinite(got)
    assert got == ref, (family, M, got, ref)


def test_even_count_adds_in_double():
    """Two finite floats whose float32 sum overflows, and two whose half-sum needs the one rounding."""
    big = np.array([3e38, 3.2e38], np.float32)
    assert R.radix_select_median(big) == np.float32((np.float64(big[0]) + np.float64(big[1])) / 2)
    assert np.isfinite(R.radix_select_median(big))
    pair = np.array([1.0, 1.0 + 2.0 ** -23], np.float32)
    assert R.radix_select_median(pair) == R.median(pair[:, None])[0]


def test_key_is_order_preserving_and_invertible():
    x = np.array([-np.float32(3e38), -1.5, -1e-45, -0.0, 0.0, 1e-45, 1.5, 3e38], np.float32)
    k = R.float_key(x)
    assert np.all(np.diff(k.astype(np.int64)) > 0)
    assert np.array_equal(R.key_float(k).view(np.uint32), x.view(np.uint32))


def test_nn_distances_is_the_double_loop():
    g = np.random.default_rng(3)
    q, w = g.standard_normal((3, 2, 4)).astype(np.float32), g.standard_normal((5, 2, 4)).astype(np.float32)
    d = R.nn_distances(q, w)
    for b in range(3):
        for p in range(5):
            ref = sum((float(q[b, j, c]) - float(w[p, j, c])) ** 2 for j in range(2) for c in range(4))
            assert abs(d[b, p] - ref) <= 1e-12 * ref
    assert np.allclose(R.sq_norms(q), (q.astype(np.float64) ** 2).sum((1, 2)))
