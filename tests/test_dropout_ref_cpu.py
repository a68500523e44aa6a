"""tests/dropout_ref.py, the numpy restatement of csrc/train_norm.hip's dropout hash that the GPU
tests take their masks from: the wrapping uint64 arithmetic against Python's big integers, the
index maps, and the statistics of every (units, p, seed) that tests/test_gpu_train_norm.py uses."""
import math

import numpy as np
import pytest

import dropout_ref as R
import test_gpu_train_norm as G

M64 = (1 << 64) - 1


def _hash_bigint(seed, idx):
    z = (seed + idx * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


@pytest.mark.parametrize('seed', [0, 7, 99, 1234, M64, R.offset_seed(1234, 3)])
def test_hash_wraps_like_big_integers(seed):
    idx = [0, 1, 2, 63, 64, 255, 2 ** 31 - 1, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 3, 2 ** 63 + 11]
    got = R.hash_u32(seed, np.array(idx, dtype=np.uint64))
    assert got.dtype == np.uint32
    assert [int(v) for v in got] == [_hash_bigint(seed, i) for i in idx]


def test_seed_offset_wraps():
    assert R.offset_seed(5, 0) == 5
    assert R.offset_seed(1234, 3) == (1234 + 3 * 0xA0761D6478BD642F) % 2 ** 64
    assert R.offset_seed(M64, 1) == 0xA0761D6478BD642F - 1
    assert 0 <= R.offset_seed(M64, M64) <= M64


def test_uniform_is_24_bits_in_float32():
    u = R.uniform(1234, np.arange(4096))
    assert u.dtype == np.float32 and u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u * 2.0 ** 24, np.floor(u * 2.0 ** 24))
    h = R.hash_u32(1234, np.arange(4096))
    assert np.array_equal((u.astype(np.float64) * 2 ** 24).astype(np.uint32), h >> np.uint32(8))


def test_keep_rule_and_scale():
    # keep iff u >= float32(p): the threshold is p as the kernel holds it, not the double
    seed, n = 7, 1 << 16
    for p in (0.2, 0.25, 0.3, 0.4):
        u = R.uniform(seed, np.arange(n))
        assert np.array_equal(R.keep_mask(seed, n, p), u >= np.float32(p))
        s = R.keep_scale(p)
        assert s.dtype == np.float32 and s == np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert abs(float(s) - 1.0 / (1.0 - p)) <= 2.0 ** -23 * float(s)
    assert R.keep_mask(seed, 100, 0.0).all() and R.keep_scale(0.0) == 1.0
    assert R.keep_mask(seed, 0, 0.3).shape == (0,)


def test_index_maps():
    B, Cc, L = 3, 5, 7
    flat, chan = R.index_flat(B, Cc, L), R.index_channel(B, Cc, L)
    for b in range(B):
        for c in range(Cc):
            for l in range(L):
                assert flat[b, c, l] == (b * Cc + c) * L + l
                assert chan[b, c, l] == b * Cc + c
    seed, p = 99, 0.4
    s = float(R.keep_scale(p))
    pre, post = R.bn_scales(seed, B, Cc, L, p, R.DROP_BEFORE)
    assert np.array_equal(pre.reshape(-1), R.keep_mask(seed, B * Cc * L, p) * s) and (post == 1).all()
    pre, post = R.bn_scales(seed, B, Cc, L, p, R.DROP_AFTER)
    assert np.array_equal(post.reshape(-1), R.keep_mask(seed, B * Cc * L, p) * s) and (pre == 1).all()
    pre, post = R.bn_scales(seed, B, Cc, L, p, R.DROP_BEFORE_CH)
    assert np.array_equal(pre[:, :, 0].reshape(-1), R.keep_mask(seed, B * Cc, p) * s)
    assert (pre == pre[:, :, :1]).all() and (post == 1).all()
    for mode in (R.DROP_NONE, R.DROP_BEFORE):
        pre, post = R.bn_scales(seed, B, Cc, L, 0.0, mode)
        assert (pre == 1).all() and (post == 1).all()
    with pytest.raises(ValueError):
        R.bn_scales(seed, B, Cc, L, p, 4)


USES = sorted(set(G.mask_uses()))


def test_gpu_tests_cover_every_mode_and_size():
    assert any(ch for _, _, _, ch in USES) and any(not ch for _, _, _, ch in USES)
    assert min(n for n, _, _, _ in USES) == 1 and max(n for n, _, _, _ in USES) == 2097230
    assert min(n for n, _, _, ch in USES if ch) >= 20
    assert all(0.2 <= p <= 0.4 for _, p, _, _ in USES)


@pytest.mark.parametrize('n,p,seed,per_channel', USES,
                         ids=[f'n{n}-p{p}-seed{s}' + ('-ch' if ch else '') for n, p, s, ch in USES])
def test_dropped_fraction_of_every_mask_the_gpu_tests_use(n, p, seed, per_channel):
    keep = R.keep_mask(seed, n, p)
    dropped = 1.0 - keep.mean()
    sigma = math.sqrt(p * (1.0 - p) / n)
    assert abs(dropped - p) <= 4.0 * sigma, (dropped, p, sigma)
    if per_channel:
        assert keep.any() and not keep.all()
