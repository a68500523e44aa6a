"""tests/augment_ref.py, the numpy restatement the device augmentation is compared with, checked
on its own: Philox4x32-10 against known answers, the identity settings against pats_data_ref's
plain batches, the ranges and the batch independence of the draw, and the mirror permutation.
No GPU: a2m.data.Augment and a2m.skeleton.mirror_permutation are host code."""
import numpy as np
import pytest

import augment_ref as R
import pats_data_ref as P

ARR = P.arrays()
HOP = 5
SMP = P.samples('ABCD', HOP)
ARENA, START, LAST = R.arena_tables(ARR, HOP)
T = 64
# (seed, pass | call << 32, pos) -> the four words.  The first is Random123's kat_vectors line for
# philox4x32-10 with counter 0 and key 0; all four are the output of rocRAND's
# rocrand_device::philox4x32_10_engine(seed, subsequence, 4 * pos) run on the host, whose key is
# (seed lo, seed hi) and whose counter is (offset / 4 lo, hi, subsequence lo, hi).
KAT = [
    ((0, 0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0x0123456789abcdef, 7 | (1 << 32), 0x100000005), 'd858cbca 6d8c525b ad2963e3 e10d9cce'),
    ((0xffffffffffffffff, 0xffffffff, 12), '0421b722 bd0b5dfa 91fbb871 7aebcdfc'),
    ((3, 0, 1), '44aa54a1 8d31473d 39713e09 9b939f1f'),
]


def _stats(seed=11):
    g = np.random.default_rng(seed)
    pm = (g.standard_normal(104) * 30).astype(np.float32)
    ps = (g.random(104) * 50 + 5).astype(np.float32)
    pm[[0, 52]], ps[[0, 52]] = 0.0, 1.0
    am = (g.standard_normal(128) - 4).astype(np.float32)
    asd = (g.random(128) * 2 + 0.5).astype(np.float32)
    asd[5] = 1e-8
    return pm, ps, am, asd


def _is_identity(params):
    """Nothing on: no mirror, s = g = 1, a zero gain (of either sign) and zero widths; the offsets of
    the empty masks are still drawn and mean nothing."""
    cols = params[:, [R.MIRROR, R.S, R.G, R.GAIN, R.FW, R.TW]]
    return np.array_equal(cols, np.tile(np.float32([0, 1, 1, 0, 0, 0]), (len(params), 1)))


@pytest.mark.parametrize('k', range(len(KAT)))
def test_philox_known_answers(k):
    (seed, sub, pos), want = KAT[k]
    words = R.philox4x32_10([pos & 0xffffffff, pos >> 32, sub & 0xffffffff, sub >> 32],
                            [seed & 0xffffffff, seed >> 32])
    assert ' '.join('%08x' % int(w) for w in words) == want


def test_philox_is_elementwise():
    """An array of counters gives what each counter gives alone, and draw() lays the counter out as
    (pos lo, pos hi, pass, call) under the key (seed lo, seed hi)."""
    (seed, sub, pos), want = KAT[1]
    words = R.philox4x32_10([np.array([0, pos & 0xffffffff]), np.array([0, pos >> 32]), np.array([0, 7]),
                             np.array([0, 1])], [np.array([0, seed & 0xffffffff]), np.array([0, seed >> 32])])
    assert ' '.join('%08x' % int(w[0]) for w in words) == KAT[0][1]
    assert ' '.join('%08x' % int(w[1]) for w in words) == want
    row = R.draw([pos], 7, seed=seed, freq_mask=20, time_mask=10)[0]       # call 1 of pass 7
    v = [np.float32(int(w, 16) >> 8) * np.float32(2.0 ** -24) for w in want.split()]
    fw, tw = np.floor(v[0] * np.float32(21)), np.floor(v[2] * np.float32(11))
    assert row[R.FW] == fw and row[R.TW] == tw
    assert row[R.F0] == np.floor(v[1] * np.float32(128 - int(fw) + 1))
    assert row[R.T0] == np.floor(v[3] * np.float32(64 - int(tw) + 1))


def test_identity_settings_reproduce_the_plain_batches():
    """Augment()'s table (s = g = 1, the rest 0) through the augmenting gather: raw, standardised and
    neck-subtracted batches of pats_data_ref bit for bit, with every role."""
    pm, ps, am, asd = _stats()
    pos = np.arange(13)
    params = R.draw(pos, 0)
    assert _is_identity(params)
    perm = _perm()
    pose, audio = P.stack(ARR, SMP, pos, P.POSE, HOP), P.stack(ARR, SMP, pos, P.AUDIO, HOP)
    for role in (R.NONE, R.AUDIO):
        got = R.gather(ARENA[P.AUDIO], START[P.AUDIO], LAST[P.AUDIO], pos, 6, T, params, role)
        assert np.array_equal(got, audio)
        got = R.gather(ARENA[P.AUDIO], START[P.AUDIO], LAST[P.AUDIO], pos, 6, T, params, role, R.STANDARDISE, am, asd)
        assert np.array_equal(got, P.standardise(audio, am, asd))
    assert np.array_equal(R.gather(ARENA[P.POSE], START[P.POSE], LAST[P.POSE], pos, 1, T, params), pose)
    for role in (R.NONE, R.POSE):
        got = R.gather(ARENA[P.POSE], START[P.POSE], LAST[P.POSE], pos, 1, T, params, role, R.NECKSUB, pm, ps, perm)
        assert np.array_equal(got, P.necksub_normalise(pose, pm, ps))


def test_drawn_values_stay_in_range():
    pos = np.concatenate([np.arange(4000), 2 ** 32 + np.arange(96), [2 ** 40 + 3]])
    for pass_ in (0, 1, 2 ** 32 - 1):
        p = R.draw(pos, pass_, seed=0x9e3779b97f4a7c15, p_mirror=0.5, speed=0.5, scale=0.25, gain=3.,
                   freq_mask=27, time_mask=64, C=128, T=64)
        assert p.dtype == np.float32 and np.isfinite(p).all()
        assert set(np.unique(p[:, R.MIRROR])) == {0., 1.} and 0.4 < p[:, R.MIRROR].mean() < 0.6
        assert 0.5 <= p[:, R.S].min() < 0.55 and 1.45 < p[:, R.S].max() <= 1.5
        assert 0.75 <= p[:, R.G].min() and p[:, R.G].max() <= 1.25
        assert -3. <= p[:, R.GAIN].min() < -2.9 and 2.9 < p[:, R.GAIN].max() <= 3.
        assert np.array_equal(p[:, 4:], np.floor(p[:, 4:])) and p[:, 4:].min() == 0
        assert p[:, R.FW].max() == 27 and p[:, R.TW].max() == 64
        assert (p[:, R.F0] + p[:, R.FW] <= 128).all() and (p[:, R.T0] + p[:, R.TW] <= 64).all()
        assert (p[:, R.F0] + p[:, R.FW]).max() == 128 and (p[:, R.T0] + p[:, R.TW]).max() == 64
    off = R.draw(pos, 0, seed=5)
    assert _is_identity(off)
    sure = R.draw(pos, 0, seed=5, p_mirror=1.)
    assert sure[:, R.MIRROR].all()


def test_params_do_not_depend_on_the_batch():
    """The rows of a pass drawn in one piece, in batches of 5 and of 3, and in reversed order are the
    same rows: a clip's parameters are a function of (seed, pass, pos)."""
    kw = dict(seed=77, p_mirror=0.5, speed=0.3, scale=0.2, gain=1., freq_mask=20, time_mask=10)
    order = np.random.default_rng(0).permutation(13)
    whole = R.draw(order, 2, **kw)
    for size in (5, 3):
        parts = [R.draw(order[b0:b0 + size], 2, **kw) for b0 in range(0, 13, size)]
        assert np.array_equal(np.concatenate(parts), whole)
    assert np.array_equal(R.draw(order[::-1], 2, **kw), whole[::-1])
    assert not np.array_equal(R.draw(order, 3, **kw), whole)
    assert not np.array_equal(R.draw(order, 2, **dict(kw, seed=78)), whole)


def _perm():
    from a2m.skeleton import mirror_permutation
    return np.asarray(mirror_permutation())


def test_mirror_permutation_is_the_name_swap():
    from a2m.skeleton import JOINT_NAMES
    perm = _perm()
    assert perm.shape == (52,) and sorted(perm) == list(range(52))
    assert np.array_equal(perm[perm], np.arange(52))
    want = np.arange(52)
    for a, b in [(1, 4), (2, 5), (3, 6), (8, 9)] + [(10 + k, 31 + k) for k in range(21)]:
        want[a], want[b] = b, a
    assert np.array_equal(perm, want) and perm[0] == 0 and perm[7] == 7
    swap = {'R': 'L', 'L': 'R'}
    for k, name in enumerate(JOINT_NAMES):
        other = JOINT_NAMES[perm[k]]
        assert other == (swap[name[0]] + name[1:] if perm[k] != k else name)
    assert [JOINT_NAMES[k] for k in range(52) if perm[k] == k] == ['Neck', 'Nose']


def test_mirroring_twice_returns_the_input():
    """Mirror a batch with unit statistics, lay the result out as a new arena, mirror that: the raw
    neck-subtracted input, exactly (a permutation, and a negation applied twice)."""
    pos = np.arange(13)
    perm = _perm()
    params = R.draw(pos, 0, p_mirror=1.)
    zero, one = np.zeros(104, np.float32), np.ones(104, np.float32)
    args = dict(role=R.POSE, mode=R.NECKSUB, mean=zero, std=one, perm=perm)
    once = R.gather(ARENA[P.POSE], START[P.POSE], LAST[P.POSE], pos, 1, T, params, **args)
    plain = P.necksub(P.stack(ARR, SMP, pos, P.POSE, HOP))
    assert not np.array_equal(once, plain)
    assert np.array_equal(once[..., :52], -plain[..., :52][..., perm])
    assert np.array_equal(once[..., 52:], plain[..., 52:][..., perm])
    arena2 = once.reshape(13 * T, 104)
    twice = R.gather(arena2, np.arange(13) * T, np.arange(13) * T + T - 1, pos, 1, T, params, **args)
    assert np.array_equal(twice, plain)
