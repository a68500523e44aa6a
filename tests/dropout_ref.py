"""Numpy restatement of the dropout hash documented at the top of csrc/train_norm.hip, in uint64
arithmetic that wraps, independent of the device:

  z = seed + idx * 0x9E3779B97F4A7C15                    (mod 2^64)
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  z ^= z >> 31
  h = z >> 32                                            (the splitmix64 finaliser's high word)
  u = float32(h >> 8) * 2^-24                            (exact: 24 bits)
  keep iff u >= float32(p);  kept elements are scaled by float32(1) / (float32(1) - float32(p))

p <= 0 keeps everything with scale 1.  With a device step counter registered
(a2m_set_dropout_seed_offset) the seed becomes seed + counter * 0xA0761D6478BD642F (mod 2^64).

The BatchNorm kernels hash a logical element index: the flat (b C + c) L + l of the [B, C, L]
tensor for DROP_BEFORE and DROP_AFTER, and b C + c (one unit per clip and channel) for
DROP_BEFORE_CH.

Shared by the CPU and GPU tests; the tests treat its outputs as read-only.
"""
import numpy as np

GOLDEN_GAMMA = 0x9E3779B97F4A7C15
MIX1 = 0xBF58476D1CE4E5B9
MIX2 = 0x94D049BB133111EB
SEED_OFFSET_K = 0xA0761D6478BD642F
_M64 = (1 << 64) - 1

DROP_NONE, DROP_BEFORE, DROP_BEFORE_CH, DROP_AFTER = 0, 1, 2, 3


def offset_seed(seed, counter):
    """The seed a launch hashes while a device counter holding `counter` is registered."""
    return (int(seed) + int(counter) * SEED_OFFSET_K) & _M64


def hash_u32(seed, idx):
    """High 32 bits of the splitmix64 finaliser of seed + idx * golden gamma; idx any int array."""
    idx = np.asarray(idx).astype(np.uint64)
    with np.errstate(over='ignore'):
        z = np.uint64(int(seed) & _M64) + idx * np.uint64(GOLDEN_GAMMA)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(MIX1)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(MIX2)
        z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(32)).astype(np.uint32)


def uniform(seed, idx):
    """float32 u in [0, 1) of each index."""
    return (hash_u32(seed, idx) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def keep_scale(p):
    """float32 1 / (1 - p), as the kernel rounds it."""
    p = np.float32(p)
    return np.float32(1.0) if p <= 0 else np.float32(1.0) / (np.float32(1.0) - p)


def keep_at(seed, idx, p):
    """bool keep flag of each logical index."""
    idx = np.asarray(idx)
    if np.float32(p) <= 0:
        return np.ones(idx.shape, dtype=bool)
    return uniform(seed, idx) >= np.float32(p)


def keep_mask(seed, n, p):
    """bool [n]: keep flags of indices 0 .. n-1 (a2m_dropout_f32's mask)."""
    return keep_at(seed, np.arange(n, dtype=np.uint64), p)


def index_flat(B, C, L):
    """[B, C, L] logical indices of DROP_BEFORE / DROP_AFTER: (b C + c) L + l."""
    return np.arange(B * C * L, dtype=np.uint64).reshape(B, C, L)


def index_channel(B, C, L):
    """[B, C, L] logical indices of DROP_BEFORE_CH: b C + c, the same for every l."""
    return np.broadcast_to(np.arange(B * C, dtype=np.uint64).reshape(B, C, 1), (B, C, L))


def bn_scales(seed, B, C, L, p, mode):
    """(pre, post) float64 [B, C, L] multipliers of the BatchNorm kernels for a DROP_* mode: the
    input is multiplied by `pre` before the statistics, the activated output by `post`."""
    one = np.ones((B, C, L))
    if mode == DROP_NONE or np.float32(p) <= 0:
        return one, one
    s = float(keep_scale(p))
    if mode == DROP_BEFORE:
        return keep_at(seed, index_flat(B, C, L), p) * s, one
    if mode == DROP_BEFORE_CH:
        return keep_at(seed, index_channel(B, C, L), p) * s, one
    if mode == DROP_AFTER:
        return one, keep_at(seed, index_flat(B, C, L), p) * s
    raise ValueError(f'unknown dropout mode {mode}')
