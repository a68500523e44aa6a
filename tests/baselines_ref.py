"""float64 / integer numpy restatements for the evaluation baselines' kernels (csrc/baselines.hip):
the squared distances of the nearest-neighbour search, the median, a radix select that mirrors the
kernel's rank logic, and the value families both median tests lay out."""
import numpy as np


def nn_distances(query, windows):
    """query [B, T, C], windows [N, T, C] -> d [B, N] = sum (q - w)^2, in float64 (a query at a time:
    no [B, N, T*C] array)."""
    q = np.asarray(query, np.float64).reshape(len(query), -1)
    w = np.asarray(windows, np.float64).reshape(len(windows), -1)
    return np.stack([((w - row) ** 2).sum(-1) for row in q])


def sq_norms(x):
    x = np.asarray(x, np.float64).reshape(len(x), -1)
    return (x * x).sum(-1)


def median(population):
    """np.median over axis 0 of float64 copies, rounded once to float32: for an even count the two
    middle elements are added in double (exact for float32 inputs), halved and rounded."""
    return np.median(np.asarray(population, np.float64), axis=0).astype(np.float32)


def float_key(x):
    """The order-preserving uint32 image of float32: bits ^ (sign ? ~0 : 1 << 31)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return u ^ np.where(u >> 31, np.uint32(0xffffffff), np.uint32(0x80000000)).astype(np.uint32)


def key_float(k):
    k = np.asarray(k, np.uint32)
    u = k ^ np.where(k >> 31, np.uint32(0x80000000), np.uint32(0xffffffff)).astype(np.uint32)
    return u.view(np.float32)


def radix_select_median(values):
    """The kernel's select on one channel's values (float32 [M]): ranks (M-1)//2 and M//2 carried at
    once; each of four passes counts the next byte (from the top) of the keys whose higher bytes equal
    the rank's prefix, walks the 256 counts to the bucket that holds the rank and subtracts the
    counts below it.  The prefixes end as the two middle elements."""
    values = np.ascontiguousarray(values, np.float32).reshape(-1)
    keys = float_key(values)
    M = keys.size
    ranks = [(M - 1) // 2, M // 2]
    prefix = [0, 0]
    for p in range(4):
        shift = 24 - 8 * p
        for w in range(2):
            live = keys if p == 0 else keys[(keys >> np.uint32(shift + 8)) == np.uint32(prefix[w])]
            hist = np.bincount(((live >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256)
            rank, b = ranks[w], 0
            while b < 255 and rank >= hist[b]:
                rank -= hist[b]
                b += 1
            prefix[w], ranks[w] = (prefix[w] << 8) | b, int(rank)
    a, b = key_float(np.array(prefix, np.uint32))
    if M % 2:
        return np.float32(a)
    return np.float32((np.float64(a) + np.float64(b)) * 0.5)


def value_families(M, seed=0):
    """{name: float32 [M]}: the value families the median must survive."""
    g = np.random.default_rng(seed + M)
    f32 = np.float32
    base = g.standard_normal(M).astype(f32)
    dup = np.sort(base)
    dup[max(M // 2 - 2, 0):M // 2 + 2] = dup[M // 2]                      # duplicates straddling the middle
    zeros = np.where(g.random(M) < 0.5, f32(-0.0), f32(0.0)).astype(f32)
    signed_zero = np.where(g.random(M) < 0.4, zeros, (g.standard_normal(M) * 1e-3).astype(f32)).astype(f32)
    denormal = (g.integers(-200, 200, M).astype(np.float64) * 1.4e-45).astype(f32)
    low_byte = (np.full(M, 0x3fc00000, np.uint32) + g.integers(0, 256, M).astype(np.uint32)).view(f32)
    wide = (g.choice([-1.0, 1.0], M) * 10.0 ** g.uniform(-30, 29.5, M)).astype(f32)
    out = {'normal': base, 'equal': np.full(M, f32(-2.5)), 'duplicates': g.permutation(dup),
           'zeros': g.permutation(zeros), 'signed_zero': signed_zero, 'denormal': denormal,
           'low_byte': low_byte.copy(), 'wide': wide}
    assert all(v.dtype == f32 and v.shape == (M,) for v in out.values())
    return out
