"""Shared inputs and float64 numpy statements for the train-sampler tests (test_sampling_cpu.py,
test_gpu_sampling.py): pats_data_ref's four intervals with poses that differ in motion, the clip
velocity and the three classifications written out from their definitions.

Each interval's pose is a cumulative sum of Gaussian steps around 300 whose per-row amplitude is
exp(U(-2.5, 2.5)) (0.25 + |sin(row / 9 + phi)|): one amplitude and one phase per interval, drawn
with the steps and then the audio (as pats_data_ref draws it) from one generator, seed 23.  At hop 5
(N = 13: 4 clips of A, 1 of C, 8 of D) the velocities are 13 distinct values between 0.37 and 7.6;
three equal-width bins hold 1, 4 and 8 clips; Q(0.9) and Q(0.4) fall strictly between elements with
no clip within 1e-3 relative; Q(0.5) is the element of rank 6 itself.  test_sampling_cpu.py checks
all of that."""
import numpy as np

import pats_data_ref as P


def arrays(seed=23):
    g = np.random.default_rng(seed)
    out = {}
    for i, (lp, la) in P.LENGTHS.items():
        amp = np.exp(g.uniform(-2.5, 2.5))
        phi = g.uniform(0, 2 * np.pi)
        per_row = amp * (0.25 + np.abs(np.sin(np.arange(lp) / 9 + phi)))
        steps = g.standard_normal((lp, 104)) * per_row[:, None]
        out[i] = {P.POSE: (300 + np.cumsum(steps, axis=0)).astype(np.float32),
                  P.AUDIO: (g.standard_normal((la, 128)) * 2 - 4).astype(np.float32)}
    return out


def velocity(rows):
    """The mean over frames t = 1 .. T-1 and joints j = 1 .. K-1 of the 2-D speed of joint j, for
    the T rows [T, C] of one clip (x in channels 0 .. K-1, y in K .. 2K-1), in float64."""
    x = np.asarray(rows, np.float64)
    K = x.shape[1] // 2
    d = x[1:] - x[:-1]
    return np.sqrt(d[:, 1:K] ** 2 + d[:, K + 1:] ** 2).mean()


def table_velocity(arena, start, window, interval):
    """velocity of every clip arena[s : s + window : interval] of a start table."""
    return np.array([velocity(arena[s:s + window:interval]) for s in start])


def clip_velocities(arr, ids, hop):
    """velocity of every sample of the concatenation of the intervals `ids`, global-index order."""
    smp = P.samples(ids, hop)
    return np.array([velocity(P.window(arr, iid, k, P.POSE, hop)) for iid, k in smp])


def quantile(v, q):
    """numpy's default quantile from the two order statistics around q (n - 1)."""
    s = np.sort(np.asarray(v, np.float64))
    pos = q * (len(s) - 1)
    lo = int(np.floor(pos))
    hi = int(np.ceil(pos))
    return s[lo] + (pos - lo) * (s[hi] - s[lo])


def above(v, q):
    v = np.asarray(v, np.float64)
    return np.flatnonzero(v > quantile(v, q))


def tail(v, q0, q1):
    v = np.asarray(v, np.float64)
    return np.flatnonzero((v > quantile(v, q1)) | (v < quantile(v, q0)))


def edges(v, q):
    v = np.asarray(v, np.float64)
    e = [v.min() + j * (v.max() - v.min()) / q for j in range(q + 1)]
    e[-1] = v.max()
    return e


def bins_of(v, e):
    """Class of every value against the ascending edges e: the first j with e[j] <= v <= e[j+1],
    -1 if none."""
    out = []
    for x in np.asarray(v, np.float64):
        hit = [j for j in range(len(e) - 1) if e[j] <= x <= e[j + 1]]
        out.append(hit[0] if hit else -1)
    return np.array(out, np.int32)


def rebalance(v, q):
    """The non-empty bins' index lists, in bin order."""
    cls = bins_of(v, edges(v, q))
    assert (cls >= 0).all()
    return [np.flatnonzero(cls == j) for j in range(q) if (cls == j).any()]
