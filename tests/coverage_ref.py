"""The sample-level set metrics of a2m.evaluation.CoverageEvaluator in float64 numpy:
improved precision and recall (Kynkaanniemi et al. 2019), density and coverage (Naeem et al. 2020) and
diversity, as a2m defines them, on the float32 feature rows the device kernels see.

  features   of a clip: 'pose' the generated clip as it is and the real one (x - mean) / where(std < 1e-7,
             1, std), each step one float32 rounding; 'motion' the float32 frame differences of those
  dist2      |a - b|^2 by direct differences in float64: the exact value up to float64 rounding
  radii      r_k2(x in S): the k-th smallest dist2(x, y) over the y of S at another position than x
  metrics    with G [nG, D] the generated and R [nR, D] the real clips (the evaluator always has nG = nR):
             precision  #{g : some r has d2(g,r) <= r_k2(r)} / nG
             recall     #{r : some g has d2(r,g) <= r_k2(g)} / nR
             density    sum_g #{r : d2(g,r) <= r_k2(r)} / (k nG)
             coverage   #{r : min_g d2(r,g) <= r_k2(r)} / nR
             diversity  the mean of sqrt(d2) over the pairs of different positions of one set
             NaN where a set has no more than k members
  tol        4 D 2^-24 (|a|^2 + |b|^2): the bound of the device's fp32 Gram form (DESIGN.md 7.9's derivation)
"""
import numpy as np

METRICS = ('precision', 'recall', 'density', 'coverage', 'diversity_fake', 'diversity_real', 'n_coverage')


def standardise(x, mean, std):
    x, mean, std = (np.asarray(a, np.float32) for a in (x, mean, std))
    out = (x - mean) / np.where(std < np.float32(1e-7), np.float32(1), std)
    assert out.dtype == np.float32
    return out


def features(fake_norm, real_px, mean, std, feature='pose'):
    """(G, R) float32 [n, D] of fake_norm, real_px [n, T, F]."""
    g = np.asarray(fake_norm, np.float32)
    r = standardise(real_px, mean, std)
    if feature == 'motion':
        g, r = g[:, 1:] - g[:, :-1], r[:, 1:] - r[:, :-1]
        assert g.dtype == np.float32 and r.dtype == np.float32
    else:
        assert feature == 'pose'
    return g.reshape(len(g), -1), r.reshape(len(r), -1)


def sq_norms(x):
    x = np.asarray(x, np.float64)
    return (x * x).sum(-1)


def dist2(a, b):
    """[nA, nB] float64: sum_k (a[i,k] - b[j,k])^2, row by row to keep the temporaries small."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = np.empty((len(a), len(b)))
    for i in range(len(a)):
        d = b - a[i]
        out[i] = (d * d).sum(-1)
    return out


def tol(a, b):
    """[nA, nB]: 4 D 2^-24 (|a_i|^2 + |b_j|^2)."""
    D = np.asarray(a).shape[-1]
    return 4.0 * D * 2.0 ** -24 * (sq_norms(a)[:, None] + sq_norms(b)[None, :])


def kth_smallest(rows, k):
    """The k-th smallest value of every row of [n, m] (1-based k)."""
    return np.sort(np.asarray(rows), axis=1)[:, k - 1]


def radii(d_self, k):
    """r_k2 of every member of a set from its [n, n] distances: self is left out by position."""
    d = np.array(d_self, np.float64)
    assert d.shape[0] == d.shape[1] > k
    np.fill_diagonal(d, np.inf)
    return kth_smallest(d, k)


def diversity(d_self):
    n = len(d_self)
    off = ~np.eye(n, dtype=bool)
    return float(np.sqrt(np.asarray(d_self, np.float64)[off]).sum() / (n * (n - 1)))


def counts(G, R, k):
    """The integers and flags under the metrics: d_gr [nG, nR], r2_real [nR], r2_fake [nG], cnt_prec [nG]
    (#r with d2(g,r) <= r_k2(r)), cnt_rec [nR] (#g with d2(r,g) <= r_k2(g)), covered [nR]."""
    d_gr = dist2(G, R)
    r2_real, r2_fake = radii(dist2(R, R), k), radii(dist2(G, G), k)
    return {'d_gr': d_gr, 'r2_real': r2_real, 'r2_fake': r2_fake,
            'cnt_prec': (d_gr <= r2_real[None, :]).sum(1), 'cnt_rec': (d_gr.T <= r2_fake[None, :]).sum(1),
            'covered': d_gr.min(0) <= r2_real}


def metrics(G, R, k):
    G, R = np.asarray(G), np.asarray(R)
    nG, nR = len(G), len(R)
    if min(nG, nR) <= k:
        out = dict.fromkeys(METRICS, float('nan'))
        out['n_coverage'] = nR
        return out
    c = counts(G, R, k)
    return {'precision': float((c['cnt_prec'] > 0).sum()) / nG, 'recall': float((c['cnt_rec'] > 0).sum()) / nR,
            'density': float(c['cnt_prec'].sum()) / (k * nG), 'coverage': float(c['covered'].sum()) / nR,
            'diversity_fake': diversity(dist2(G, G)), 'diversity_real': diversity(dist2(R, R)), 'n_coverage': nR}


def by_style(G, R, style, n_styles, k):
    """{style id: metrics, 'all': metrics of the pooled clips whose style is in range}."""
    style = np.asarray(style)
    out = {s: metrics(G[style == s], R[style == s], k) for s in range(n_styles)}
    ok = (style >= 0) & (style < n_styles)
    out['all'] = metrics(G[ok], R[ok], k)
    return out
