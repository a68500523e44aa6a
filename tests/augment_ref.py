"""numpy fp32 restatement of csrc/augment.hip for test_augment_ref_cpu.py and test_gpu_augment.py:
Philox4x32-10, the per-clip parameter draw, and the augmenting gather over plain arrays (an arena
[rows, C], start and last tables indexed by table position).  Every float step is one float32
operation in the order the kernels take it, so equality with the device is demanded bit for bit.

arena_tables() lays pats_data_ref's four intervals out as PatsLoader does: concatenated in id
order, a start entry per sample, and beside it the arena row of the last row of the sample's
interval."""
import numpy as np

import pats_data_ref as P

F = np.float32
NONE, POSE, AUDIO = 0, 1, 2                     # roles
RAW, STANDARDISE, NECKSUB = 0, 1, 2             # modes
MIRROR, S, G, GAIN, F0, FW, T0, TW = range(8)   # columns of the parameter table
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 and key: 2 uint32 arrays (or ints) of one shape -> the 4 output words."""
    c = [np.asarray(x, np.uint64) & MASK for x in counter]
    k = [np.asarray(x, np.uint64) & MASK for x in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]            # < 2^64: no wrap
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [x.astype(np.uint32) for x in c]


def unit24(x):
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(F) * F(2.0 ** -24)


def draw(pos, pass_, seed=0, p_mirror=0., speed=0., scale=0., gain=0., freq_mask=0, time_mask=0, C=128, T=64):
    """float32 [n, 8]: the rows a2m_augment_params_f32 writes for the table positions pos."""
    pos = np.asarray(pos, np.int64).astype(np.uint64)
    key = [np.full(pos.shape, seed & 0xFFFFFFFF, np.uint64), np.full(pos.shape, seed >> 32, np.uint64)]
    words = [[pos & MASK, pos >> np.uint64(32), np.full(pos.shape, pass_ & 0xFFFFFFFF, np.uint64),
              np.full(pos.shape, call, np.uint64)] for call in (0, 1)]
    u = [unit24(w) for w in philox4x32_10(words[0], key)]
    v = [unit24(w) for w in philox4x32_10(words[1], key)]

    def spread(r, x):
        return F(r) * (F(2) * x - F(1))

    out = np.empty((len(pos), 8), F)
    out[:, MIRROR] = u[0] < F(p_mirror)
    out[:, S] = F(1) + spread(speed, u[1])
    out[:, G] = F(1) + spread(scale, u[2])
    out[:, GAIN] = spread(gain, u[3])
    fw = np.floor(v[0] * F(freq_mask + 1))
    tw = np.floor(v[2] * F(time_mask + 1))
    out[:, FW], out[:, TW] = fw, tw
    out[:, F0] = np.floor(v[1] * (C - fw.astype(np.int64) + 1).astype(F))
    out[:, T0] = np.floor(v[3] * (T - tw.astype(np.int64) + 1).astype(F))
    assert all(x.dtype == F for x in u + v) and fw.dtype == F
    return out


def rows_read(start, last, interval, T, s):
    """(a, b, f) of one clip: the arena rows [T] and the fraction [T] of every output frame."""
    p = (np.arange(T) * interval).astype(F) * F(s)
    assert p.dtype == F and (p >= 0).all()
    i = np.floor(p)
    f = p - i
    r = start + i.astype(np.int64)
    return np.minimum(r, last), np.minimum(r + 1, last), f


def gather(arena, start, last, pos, interval, T, params, role=NONE, mode=RAW, mean=None, std=None, perm=None,
           mask_fill=0.):
    """float32 [n, T, C]: a2m_batch_gather_aug_f32 for one modality over the table positions pos."""
    arena, params = np.asarray(arena, F), np.asarray(params, F)
    C = arena.shape[1]
    out = np.empty((len(pos), T, C), F)
    with np.errstate(invalid='ignore'):
        for n, (q, par) in enumerate(zip(pos, params)):
            a, b, f = rows_read(start[q], last[q], interval, T, par[S])
            x = arena[a]
            two = f != 0
            # row b is read only where the fraction is not zero
            x[two] = x[two] + f[two, None] * (arena[b[two]] - x[two])
            if mode == NECKSUB:
                x = x.reshape(T, 2, 52)
                neck = x[:, :, :1]
                mir = role == POSE and par[MIRROR] != 0
                d = (x[:, :, perm] if mir else x) - neck
                if mir:
                    d[:, 0] = -d[:, 0]
                if role == POSE:
                    d = d * par[G]
                x = (d.reshape(T, C) - np.asarray(mean, F)) / np.asarray(std, F)
            else:
                if role == AUDIO and par[GAIN] != 0:
                    x = x + par[GAIN]
                if mode == STANDARDISE:
                    x = P.standardise(x, mean, std)
                if role == AUDIO:
                    f0, fw, t0, tw = (int(v) for v in par[F0:])
                    x[:, f0:f0 + fw] = F(mask_fill)
                    x[t0:t0 + tw] = F(mask_fill)
            assert x.dtype == F
            out[n] = x
    return out


def arena_tables(arr, hop, ids='ABCD'):
    """({modality: arena}, {modality: start}, {modality: last}) over the samples of the intervals
    ids, all in one split, as PatsLoader lays them out."""
    smp = P.samples(ids, hop)
    arena, start, last = {}, {}, {}
    for mod in (P.POSE, P.AUDIO):
        row0, at = {}, 0
        for i in ids:
            row0[i] = at
            at += len(arr[i][mod])
        arena[mod] = np.concatenate([arr[i][mod] for i in ids])
        start[mod] = np.array([row0[i] + P.starts(len(arr[i][mod]), mod, hop)[k] for i, k in smp], np.int64)
        last[mod] = np.array([row0[i] + len(arr[i][mod]) - 1 for i, _ in smp], np.int64)
    return arena, start, last
