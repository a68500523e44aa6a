"""The metrics of a2m.evaluation.PoseEvaluator restated in float64 numpy.

Poses are [B, T, 2K] float32, a frame being its x row then its y row.  fake_px comes in as
float32, already de-normalised, so that both sides round the de-normalisation identically
(denormalize() gives the two float32 roundings of fake_norm * std + mean).  Every function
returns, next to a sum, what its tolerance needs: the number of terms and the sum of their
magnitudes (the any-order summation bound |got - ref| <= 8 n 2^-53 sum |terms| of sum_tol)."""
import numpy as np

U = 2.0 ** -53


def sum_tol(n_terms, abs_sum):
    """8 n 2^-53 sum |terms|: n u sum |terms| bounds a float64 sum of n terms taken in any order, and
    the factor 8 leaves room for the few roundings inside each term."""
    return 8.0 * np.asarray(n_terms, np.float64) * U * np.asarray(abs_sum, np.float64)


def denormalise(fake_norm, mean, std):
    f = np.asarray(fake_norm, np.float32) * np.asarray(std, np.float32)
    out = f + np.asarray(mean, np.float32)
    assert out.dtype == np.float32
    return out


def _xy(px):
    p = np.asarray(px)
    assert p.dtype == np.float32 and p.shape[-1] % 2 == 0
    K = p.shape[-1] // 2
    p = p.astype(np.float64)
    return p[..., :K], p[..., K:]


def pck_hits(fake_px, real_px, alpha=0.2):
    """hits [..., K] (bool) and the smallest relative gap between a keypoint distance and its radius."""
    fx, fy = _xy(fake_px)
    rx, ry = _xy(real_px)
    ext = np.maximum(np.abs(rx.max(-1) - rx.min(-1)), np.abs(ry.max(-1) - ry.min(-1)))
    radius = (ext * alpha)[..., None]
    dist = np.sqrt((rx - fx) ** 2 + (ry - fy) ** 2)
    gap = np.abs(dist - radius) / np.maximum(radius, 1e-300)
    return dist <= radius, float(gap.min()) if gap.size else np.inf


def pck(pred, gt, alpha=0.2):
    """compute_pck's [N, 2, K] interface on the same arithmetic."""
    N = len(gt)
    hits, _ = pck_hits(np.asarray(pred, np.float32).reshape(N, -1), np.asarray(gt, np.float32).reshape(N, -1), alpha)
    return hits.sum(-1) / hits.shape[-1]


def speed_accel(px):
    """speed [B, T-1] (frames 1..T-1) and accel [B, T-2] (frames 2..T-1): the mean over joints 1..K-1 of
    |p[t] - p[t-1]| and of |p[t] - 2 p[t-1] + p[t-2]|.  Differences stay inside a clip (axis 1)."""
    x, y = _xy(px)
    x, y = x[..., 1:], y[..., 1:]
    B, T = x.shape[:2]
    speed = np.sqrt((x[:, 1:] - x[:, :-1]) ** 2 + (y[:, 1:] - y[:, :-1]) ** 2).mean(-1) if T > 1 else np.zeros((B, 0))
    if T > 2:
        ax = x[:, 2:] - 2.0 * x[:, 1:-1] + x[:, :-2]
        ay = y[:, 2:] - 2.0 * y[:, 1:-1] + y[:, :-2]
        accel = np.sqrt(ax ** 2 + ay ** 2).mean(-1)
    else:
        accel = np.zeros((B, 0))
    return speed, accel


def histogram(v, width, n_bins):
    """Counts of bin min(floor(v / width), n_bins - 1), int64 [n_bins], and the smallest relative gap
    between a value and a bin edge (inf where there are no values)."""
    v = np.asarray(v, np.float64).reshape(-1)
    idx = np.minimum(np.floor(v / width), n_bins - 1).astype(np.int64)
    edge = np.rint(v / width) * width                    # the nearest edge
    gap = np.abs(v - edge) / np.maximum(np.abs(v), 1e-300)
    return np.bincount(idx, minlength=n_bins).astype(np.int64), float(gap.min()) if v.size else np.inf


def clip_metrics(fake_px, real_px, style, n_styles, alpha, n_bins, speed_width, accel_width):
    """Everything a2m_eval_clip_f32 and a2m_eval_finish_f64 accumulate, per style:
    counts [S, 3] (clips, frames, hits), hits [B] per clip, sums [S, 3] (L1, real speed, generated speed)
    with their n_terms [S, 3] and abs_sums [S, 3], part [B, 3] the same sums per clip with part_n, part_abs,
    hist [S, 4, n_bins], dropped, and margin = the smallest relative gap of a distance to its radius or of
    a speed / acceleration to a bin edge."""
    fake_px, real_px = np.asarray(fake_px), np.asarray(real_px)
    style = np.asarray(style)
    B, T, Fd = real_px.shape
    S = n_styles
    hit, margin = pck_hits(fake_px, real_px, alpha)
    hits = hit.sum((1, 2)).astype(np.int64)
    l1 = np.abs(fake_px.astype(np.float64) - real_px.astype(np.float64)).sum((1, 2))
    sr, ar = speed_accel(real_px)
    sf, af = speed_accel(fake_px)
    part = np.stack([l1, sr.sum(1), sf.sum(1)], 1)
    part_n = np.broadcast_to(np.array([T * Fd, max(T - 1, 0), max(T - 1, 0)], np.float64), (B, 3))
    out = dict(hits=hits, part=part, part_n=part_n, part_abs=part.copy(), counts=np.zeros((S, 3), np.int64),
               sums=np.zeros((S, 3)), n_terms=np.zeros((S, 3)), hist=np.zeros((S, 4, n_bins), np.int64),
               dropped=int(((style < 0) | (style >= S)).sum()))
    for s in range(S):
        m = style == s
        out['counts'][s] = [m.sum(), m.sum() * T, hits[m].sum()]
        out['sums'][s] = part[m].sum(0)
        out['n_terms'][s] = part_n[m].sum(0)
        for j, (v, w) in enumerate(((sr, speed_width), (sf, speed_width), (ar, accel_width), (af, accel_width))):
            out['hist'][s, j], gap = histogram(v[m], w, n_bins)
            margin = min(margin, gap)
    out['abs_sums'] = out['sums'].copy()                  # every term is a magnitude
    out['margin'] = margin
    out['speed'], out['accel'] = (sr, sf), (ar, af)
    return out


def gram_sums(fake_px, real_px, style, n_styles):
    """Per style, for the real (index 0) and the generated (index 1) frames: n [S] frames, sx [S, 2, F],
    gram [S, 2, F, F], and abs_sx, abs_gram, the sums of the terms' magnitudes."""
    fake_px, real_px = np.asarray(fake_px), np.asarray(real_px)
    style = np.asarray(style)
    B, T, Fd = real_px.shape
    S = n_styles
    n = np.zeros(S, np.int64)
    sx, gram = np.zeros((S, 2, Fd)), np.zeros((S, 2, Fd, Fd))
    abs_sx, abs_gram = np.zeros_like(sx), np.zeros_like(gram)
    for s in range(S):
        m = style == s
        n[s] = m.sum() * T
        for w, px in enumerate((real_px, fake_px)):
            x = px[m].astype(np.float64).reshape(-1, Fd)
            sx[s, w], abs_sx[s, w] = x.sum(0), np.abs(x).sum(0)
            gram[s, w], abs_gram[s, w] = x.T @ x, np.abs(x).T @ np.abs(x)
    return dict(n=n, sx=sx, gram=gram, abs_sx=abs_sx, abs_gram=abs_gram)


def w1_samples(a, b):
    """The exact Wasserstein-1 distance of two samples: the integral of |F_a - F_b| between the sorted
    values of both."""
    a, b = np.sort(np.asarray(a, np.float64)), np.sort(np.asarray(b, np.float64))
    z = np.sort(np.concatenate([a, b]))
    fa = np.searchsorted(a, z[:-1], side='right') / a.size
    fb = np.searchsorted(b, z[:-1], side='right') / b.size
    return float((np.abs(fa - fb) * np.diff(z)).sum())
