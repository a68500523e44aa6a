"""Evaluation on the device.

compute_pck(pred, gt, alpha=0.2): PCK, motion_evaluation.py:4-22 (52
keypoints) and pose_video/evaluation.py:4-21 (48 keypoints; the keypoint count is taken from the
input).  pred, gt [N, 2, K] (x row, y row) -> [N], the fraction of keypoints whose distance to gt
is <= alpha * max(x extent, y extent) of that sample's gt.  numpy in -> numpy out (like the
reference); device tensors in -> device tensor out.

PoseEvaluator / evaluate: one pass over a split with every sum kept on the device (DESIGN.md
7.7): per speaker and pooled, PCK and L1 in pixels, the Frechet distance between the real and the
generated frames, and the Wasserstein-1 distance between their speed and acceleration
distributions.  The reference has PCK only; the other metrics are a2m's own definitions:

  fake_px   fake_norm * std + mean, two float32 roundings (a2m.normalization.denormalize)
  pck       hits / (frames K): the keypoints (the root included) within alpha * max(x extent,
            y extent) of the real frame, float64 on the float32 coordinates, as compute_pck
  l1        sum |fake_px - real_px| / (frames 2K)
  speed     of frame t >= 1: the mean over joints 1..K-1 of |pose[t] - pose[t-1]| (Euclidean)
  accel     of frame t >= 2: the same mean of |pose[t] - 2 pose[t-1] + pose[t-2]|
            both in float64, of the real and of the generated pose, never across a clip boundary,
            each counted in bin min(floor(v / width), n_bins - 1), width = max / n_bins
  fd        frechet_distance of the per-style frame counts, sum x [2K] and sum x x^T [2K, 2K]
  w1_*      w1_from_histograms of the real and the generated histogram

The histogram range (speed_max = accel_max = 64 px / frame in 512 bins) is a guess, nobody has
looked at PATS speeds at 15 fps: the last bin catches everything beyond it, and its share of the
samples is reported as speed_overflow / accel_overflow.  Widen the range when that share is large.

AudioSyncEvaluator / evaluate(..., sync=True): none of the metrics above reads the audio, so a
generator whose gestures ignore the speech scores like one whose strokes land on the syllables.
The opt-in synchrony metrics (SYNC_METRICS) do, again a2m's own definitions, float64
on the float32 inputs, per clip of frames 0..T-1:

  onset     o[t] = (1/C) sum_c max(0, (a[t,c] - a[t-1,c]) sigma_c), t = 1..T-1; a the audio feature
            the generator got, sigma_c = audio_std[c] when it was standardised (else 1), so that the
            onsets are those of the raw log-mel whatever the generator was trained with
  speed     s[t] as above, of the real and of the generated pose
  beats     audio at t in [2, T-2]: o[t] > o[t-1], o[t] >= o[t+1] and o[t] > onset_delta mean(o[1..T-1]);
            motion (kinematic) at t in [2, T-2]: s[t] < s[t-1] and s[t] <= s[t+1].  A constant signal
            has none, nor has a clip of T < 4
  beat_dist every motion beat's distance in frames to the clip's nearest audio beat, counted in bin
            min(d, n_dist - 1), the last bin also when the clip has no audio beat; and the reverse
            direction, every audio beat to the nearest motion beat, the same way
  beat_align_*   sum_d h[d] exp(-d^2 / (2 beat_sigma^2)) / sum_d h[d] over motion->audio (AIST++'s
                 direction); beat_recall_* the same over audio->motion
  sync_corr_*    Pearson's r of the pairs (o[t], s[t+l]), t and t + l in [1, T-1], for l = -n_lags ..
                 n_lags, from float64 sums; NaN with fewer than 2 pairs or no variance
  sync_lag_*     the l of the largest r; l > 0: the motion follows the audio

each for the real pose (the ceiling a generator can be held to) and the generated one.
onset_delta = 1.0 and beat_sigma = 1.0 frame (67 ms at 15 fps; AIST++ uses 50 ms) are guesses like
the histogram range: nobody has looked at PATS onsets at 15 fps.  beat_far_share is the share of
the motion beats in the last distance bin.

CoverageEvaluator / evaluate(..., coverage=True): all of the above pool frames, so a generator that
emits one plausible clip for every audio window scores well.  The opt-in set metrics over whole clips
(COVERAGE_METRICS) single it out: improved precision and recall, density and coverage,
and the mean pairwise distance among the generated and among the real clips; the class docstring has
the definitions.
"""
import numpy as np
import torch

from . import functional as F
from ._native import check, lib

METRICS = ('pck', 'l1', 'fd', 'w1_speed', 'w1_accel', 'mean_speed_real', 'mean_speed_fake', 'n_clips',
           'n_frames', 'speed_overflow', 'accel_overflow')
SYNC_METRICS = ('beat_align_real', 'beat_align_fake', 'beat_recall_real', 'beat_recall_fake', 'sync_corr_real',
                'sync_corr_fake', 'sync_lag_real', 'sync_lag_fake', 'n_audio_beats', 'n_motion_beats_real',
                'n_motion_beats_fake', 'beat_far_share')
COVERAGE_METRICS = ('precision', 'recall', 'density', 'coverage', 'diversity_fake', 'diversity_real', 'n_coverage')


def compute_pck(pred, gt, alpha=0.2):
    as_numpy = not torch.is_tensor(gt)
    g = torch.as_tensor(np.asarray(gt, np.float32)).cuda() if as_numpy else gt
    p = torch.as_tensor(np.asarray(pred, np.float32)).cuda() if as_numpy else pred
    F._check_dev(p.float(), g.float())
    g, p = g.float().contiguous(), p.float().contiguous()
    if g.dim() != 3 or g.shape[1] != 2 or tuple(p.shape) != tuple(g.shape):
        raise ValueError(f'pred and gt must both be [N, 2, K]; got {tuple(p.shape)}, {tuple(g.shape)}')
    N, _, K = g.shape
    out = torch.empty(N, dtype=torch.float64, device=g.device)
    check(lib.a2m_pck_f32(F._p(p), F._p(g), N, K, float(alpha), F._p(out), F._stream()))
    return out.cpu().numpy() if as_numpy else out


# ---------------------------------------------------------------------------------- host formulas
def _mean_cov(n, s, G):
    mu = np.asarray(s, np.float64) / n
    cov = np.asarray(G, np.float64) / n - np.outer(mu, mu)
    return mu, 0.5 * (cov + cov.T)


def frechet_distance(n1, s1, G1, n2, s2, G2):
    """The squared Frechet distance (the FID form) between the Gaussians fitted to two sets of
    frames given as counts, sums [F] and Gram sums [F, F]: mu = s / n, Sigma = G / n - mu mu^T,
        d^2 = |mu1 - mu2|^2 + tr Sigma1 + tr Sigma2 - 2 sum_i sqrt(lambda_i(Sigma1^1/2 Sigma2 Sigma1^1/2)).
    float64 numpy, two symmetric eigen-decompositions with the eigenvalues clipped at 0 (no scipy),
    so a rank-deficient covariance (fewer frames than features) is no error.  Rounding can leave
    the result of near-equal inputs a little below zero; it is not clipped."""
    mu1, c1 = _mean_cov(n1, s1, G1)
    mu2, c2 = _mean_cov(n2, s2, G2)
    w, v = np.linalg.eigh(c1)
    root = (v * np.sqrt(np.clip(w, 0.0, None))) @ v.T
    m = root @ c2 @ root
    lam = np.clip(np.linalg.eigvalsh(0.5 * (m + m.T)), 0.0, None)
    d = mu1 - mu2
    return float(d @ d + np.trace(c1) + np.trace(c2) - 2.0 * np.sqrt(lam).sum())


def w1_from_histograms(h1, h2, width):
    """Wasserstein-1 distance of two histograms over the same bins: width * sum |cdf1 - cdf2|, each
    cdf that of its histogram's share per bin.  Within one bin width of the samples' exact W1."""
    h1, h2 = np.asarray(h1, np.float64), np.asarray(h2, np.float64)
    if h1.sum() <= 0 or h2.sum() <= 0:
        return float('nan')
    return float(width * np.abs(np.cumsum(h1) / h1.sum() - np.cumsum(h2) / h2.sum()).sum())


def mirror_gram(gram):
    """The full symmetric [..., F, F] matrices of gram accumulators whose tiles below the diagonal are
    not kept up: the upper triangle and its mirror image."""
    gram = np.asarray(gram)
    return np.triu(gram) + np.swapaxes(np.triu(gram, 1), -1, -2)


def _metrics(counts, sums, hist, sx, gram, K, speed_width, accel_width):
    """One entry of result() from one style's (or the pooled) accumulators on the host."""
    n_clips, n_frames, hits = (int(c) for c in counts)
    nan = float('nan')
    out = {'n_clips': n_clips, 'n_frames': n_frames}
    out['pck'] = hits / (n_frames * K) if n_frames else nan
    out['l1'] = float(sums[0]) / (n_frames * 2 * K) if n_frames else nan
    n_speed = (int(hist[0].sum()), int(hist[1].sum()))
    out['mean_speed_real'] = float(sums[1]) / n_speed[0] if n_speed[0] else nan
    out['mean_speed_fake'] = float(sums[2]) / n_speed[1] if n_speed[1] else nan
    out['w1_speed'] = w1_from_histograms(hist[0], hist[1], speed_width)
    out['w1_accel'] = w1_from_histograms(hist[2], hist[3], accel_width)
    for name, h in (('speed_overflow', hist[:2]), ('accel_overflow', hist[2:])):
        out[name] = float(h[:, -1].sum()) / float(h.sum()) if h.sum() else nan
    out['fd'] = frechet_distance(n_frames, sx[0], gram[0], n_frames, sx[1], gram[1]) if n_frames else nan
    return out


def beat_alignment(hist, beat_sigma=1.0):
    """sum_d h[d] exp(-d^2 / (2 beat_sigma^2)) / sum_d h[d] of a histogram of beat distances in frames
    (bin d holds distance d; the last bin everything farther, and the beats with no partner);
    NaN for an empty histogram."""
    h = np.asarray(hist, np.float64)
    if h.sum() <= 0:
        return float('nan')
    d = np.arange(h.shape[-1], dtype=np.float64)
    return float((h * np.exp(-d * d / (2.0 * float(beat_sigma) ** 2))).sum() / h.sum())


def pearson_from_sums(n, sx, sxx, sy, syy, sxy):
    """Pearson's r per element from counts and float64 sums: (n sxy - sx sy) / sqrt((n sxx - sx^2)
    (n syy - sy^2)); NaN where n < 2 or a variance is <= 0."""
    n, sx, sxx, sy, syy, sxy = (np.asarray(a, np.float64) for a in (n, sx, sxx, sy, syy, sxy))
    vx, vy = n * sxx - sx * sx, n * syy - sy * sy
    ok = (n >= 2) & (vx > 0) & (vy > 0)
    r = np.full(np.broadcast(n, vx).shape, np.nan)
    r[ok] = ((n * sxy - sx * sy)[ok]) / np.sqrt(vx[ok] * vy[ok])
    return r


def _sync_metrics(beat_dist, beat_counts, lag_sums, lag_n, beat_sigma):
    """One entry of AudioSyncEvaluator.result() from one style's (or the pooled) accumulators."""
    nan = float('nan')
    n_lags = (len(lag_n) - 1) // 2
    out = {'n_audio_beats': int(beat_counts[0]), 'n_motion_beats_real': int(beat_counts[1]),
           'n_motion_beats_fake': int(beat_counts[2])}
    for w, name in enumerate(('real', 'fake')):
        out['beat_align_' + name] = beat_alignment(beat_dist[w, 0], beat_sigma)
        out['beat_recall_' + name] = beat_alignment(beat_dist[w, 1], beat_sigma)
        r = pearson_from_sums(lag_n, lag_sums[:, 0], lag_sums[:, 1], *(lag_sums[:, 2 + 3 * w + j] for j in range(3)))
        out['sync_corr_' + name] = [float(v) for v in r]
        out['sync_lag_' + name] = nan if np.isnan(r).all() else int(np.nanargmax(r)) - n_lags
    m2a = beat_dist[:, 0]
    out['beat_far_share'] = float(m2a[:, -1].sum()) / float(m2a.sum()) if m2a.sum() else nan
    return out


class PoseEvaluator:
    """The device accumulators of one evaluation pass.  pose_mean, pose_std [2K]: the statistics
    the generator's output is de-normalised with; n_styles: the number of speakers."""

    def __init__(self, pose_mean, pose_std, n_styles, alpha=0.2, n_bins=512, speed_max=64.0, accel_max=64.0,
                 device='cuda'):
        self.device = torch.device(device)
        self.mean = torch.as_tensor(pose_mean).to(self.device, torch.float32).contiguous().reshape(-1)
        self.std = torch.as_tensor(pose_std).to(self.device, torch.float32).contiguous().reshape(-1)
        Fd = self.mean.numel()
        if self.std.numel() != Fd or Fd % 2 or Fd < 4:
            raise ValueError(f'pose_mean and pose_std must both be [2K], K >= 2; got {Fd} and {self.std.numel()}')
        if n_styles <= 0 or n_bins <= 0 or not speed_max > 0 or not accel_max > 0:
            raise ValueError('n_styles, n_bins, speed_max and accel_max must be positive')
        self.n_styles, self.alpha, self.n_bins, self.Fd, self.K = int(n_styles), float(alpha), int(n_bins), Fd, Fd // 2
        self.speed_width, self.accel_width = float(speed_max) / n_bins, float(accel_max) / n_bins
        S = self.n_styles
        # one float64 arena, so that result() is one read; the integer counters are views of it
        sizes = [('counts', (3 * S + 1,), torch.int64), ('sums', (S, 3), torch.float64),
                 ('hist', (S, 4, self.n_bins), torch.int64), ('sx', (S, 2, Fd), torch.float64),
                 ('gram', (S, 2, Fd, Fd), torch.float64)]
        self._layout, n = [], 0
        for name, shape, dtype in sizes:
            self._layout.append((name, n, shape, dtype))
            n += int(np.prod(shape))
        self._arena = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._state = self._views(self._arena)
        self._buffers = {}

    def _views(self, arena):
        return {name: arena[a:a + int(np.prod(shape))].view(dtype).view(shape)
                for name, a, shape, dtype in self._layout}

    def reset(self):
        self._arena.zero_()

    def state(self):
        """The raw accumulators as device tensors (views, not copies): counts [3 n_styles + 1] (per
        style clips, frames, hits; then the dropped clips), sums [n_styles, 3] (L1, real speed,
        generated speed), hist [n_styles, 4, n_bins] (real speed, generated speed, real
        acceleration, generated acceleration), sx [n_styles, 2, 2K] and gram [n_styles, 2, 2K, 2K]
        (real, generated; only the 16 x 16 tiles on and above the diagonal are kept up)."""
        return dict(self._state)

    def update(self, fake_norm, real_px, style):
        """Adds one batch: fake_norm [n, T, 2K] the generator's normalised output, real_px
        [n, T, 2K] the neck-subtracted pose in pixels, style int32 [n] on the device.  Three
        launches, no host synchronisation, and no allocation after the first batch of a size."""
        n, T, Fd = fake_norm.shape
        if Fd != self.Fd:
            raise ValueError(f'poses of {Fd} features; the statistics have {self.Fd}')
        key = (n, T)
        if key not in self._buffers:
            self._buffers[key] = (torch.empty(n, T, Fd, device=self.device),
                                  torch.empty(n, 3, dtype=torch.float64, device=self.device),
                                  torch.empty(n, dtype=torch.int32, device=self.device))
        fake_px, part, hits = self._buffers[key]
        st = self._state
        F.eval_clip(fake_norm, real_px, style, self.mean, self.std, self.n_styles, self.alpha, self.speed_width,
                    self.accel_width, st['hist'], fake_px, part, hits)
        F.eval_gram(fake_px, real_px, style, st['sx'], st['gram'])
        F.eval_finish(part, hits, style, T, st['counts'], st['sums'])

    def fake_px(self, n, T):
        """The de-normalised generated pose [n, T, 2K] that the last update() of a batch of this size
        left on the device (read-only: the next such update() overwrites it)."""
        return self._buffers[(n, T)][0]

    def result(self):
        """The pass's one host read.  {style id: metrics, ..., 'all': metrics, 'dropped': clips whose
        style was out of range}; metrics holds METRICS.  'all' comes from the summed accumulators
        (the pooled distribution), it is no mean of the per-style values.  A style without
        frames has NaN metrics."""
        host = self._views(self._arena.cpu())
        counts, sums, hist = host['counts'].numpy(), host['sums'].numpy(), host['hist'].numpy()
        sx, gram = host['sx'].numpy(), host['gram'].numpy()
        gram = mirror_gram(gram)
        per = counts[:-1].reshape(self.n_styles, 3)
        args = (self.K, self.speed_width, self.accel_width)
        out = {s: _metrics(per[s], sums[s], hist[s], sx[s], gram[s], *args) for s in range(self.n_styles)}
        out['all'] = _metrics(per.sum(0), sums.sum(0), hist.sum(0), sx.sum(0), gram.sum(0), *args)
        out['dropped'] = int(counts[-1])
        return out


class AudioSyncEvaluator:
    """The device accumulators of the audio-motion synchrony metrics of one evaluation pass (the
    module docstring has the definitions).  n_styles: the number of speakers; n_lags: the lagged
    correlation runs over -n_lags .. n_lags frames (0 <= n_lags <= 16); n_dist: the bins of the beat
    distance histograms; audio_std [C]: the std the audio fed to update() was standardised with, or
    None when it is raw."""

    def __init__(self, n_styles, n_lags=4, n_dist=32, onset_delta=1.0, audio_std=None, device='cuda'):
        if n_styles <= 0 or n_dist < 2 or not 0 <= n_lags <= 16:
            raise ValueError('n_styles must be positive, n_dist >= 2 and 0 <= n_lags <= 16')
        if not (np.isfinite(onset_delta) and onset_delta >= 0):
            raise ValueError('onset_delta must be finite and >= 0')
        self.device = torch.device(device)
        self.n_styles, self.n_lags, self.n_dist = int(n_styles), int(n_lags), int(n_dist)
        self.onset_delta = float(onset_delta)
        self.audio_std = None if audio_std is None else \
            torch.as_tensor(audio_std).to(self.device, torch.float32).contiguous().reshape(-1)
        S, L = self.n_styles, 2 * self.n_lags + 1
        # one float64 arena, as PoseEvaluator's: result() is one read
        sizes = [('beat_dist', (S, 2, 2, self.n_dist), torch.int64), ('beat_counts', (S, 3), torch.int64),
                 ('lag_sums', (S, L, 8), torch.float64), ('lag_n', (S, L), torch.int64)]
        self._layout, n = [], 0
        for name, shape, dtype in sizes:
            self._layout.append((name, n, shape, dtype))
            n += int(np.prod(shape))
        self._arena = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._state = self._views(self._arena)
        self._buffers = {}

    _views = PoseEvaluator._views

    def reset(self):
        self._arena.zero_()

    def state(self):
        """The raw accumulators as device tensors (views, not copies): beat_dist [n_styles, 2, 2,
        n_dist] (real | generated pose; motion->audio | audio->motion), beat_counts [n_styles, 3]
        (audio, real motion, generated motion beats), lag_sums [n_styles, 2 n_lags + 1, 8] (per lag
        the sums of o, o^2, then s, s^2, o s of the real and of the generated pose) and lag_n
        [n_styles, 2 n_lags + 1] (the pairs)."""
        return dict(self._state)

    def update(self, audio, fake_px, real_px, style):
        """Adds one batch: audio [n, T, C] as the generator got it, fake_px and real_px [n, T, 2K]
        in pixels, style int32 [n] on the device.  Two launches, no host synchronisation, and no
        allocation after the first batch of a size."""
        n, T = audio.shape[:2]
        if self.audio_std is not None and self.audio_std.numel() != audio.shape[2]:
            raise ValueError(f'audio of {audio.shape[2]} columns; audio_std has {self.audio_std.numel()}')
        if n not in self._buffers:
            self._buffers[n] = torch.empty(n, 2 * self.n_lags + 1, 8, dtype=torch.float64, device=self.device)
        part, st = self._buffers[n], self._state
        F.eval_sync(audio, fake_px, real_px, style, st['beat_dist'], st['beat_counts'], self.n_lags,
                    self.onset_delta, self.audio_std, part)
        F.eval_sync_finish(part, style, T, st['lag_sums'], st['lag_n'])

    def result(self, beat_sigma=1.0):
        """The one host read.  {style id: metrics, ..., 'all': metrics}; metrics holds SYNC_METRICS.
        beat_sigma: the Gaussian width in frames of beat_align / beat_recall, a host-side choice.
        'all' comes from the summed accumulators.  A style without beats or pairs has NaN metrics."""
        host = {k: v.numpy() for k, v in self._views(self._arena.cpu()).items()}
        keys = ('beat_dist', 'beat_counts', 'lag_sums', 'lag_n')
        out = {s: _sync_metrics(*(host[k][s] for k in keys), beat_sigma) for s in range(self.n_styles)}
        out['all'] = _sync_metrics(*(host[k].sum(0) for k in keys), beat_sigma)
        return out


def _coverage_metrics(k, kth_real, cnt_prec, cnt_rec, min_rg, sum_real, sum_fake):
    """One entry of CoverageEvaluator.result() from one set's per-row vectors on the host."""
    m = len(kth_real)
    if m <= k:
        out = dict.fromkeys(COVERAGE_METRICS, float('nan'))
    else:
        pairs = float(m) * (m - 1)
        out = {'precision': float(np.count_nonzero(cnt_prec > 0)) / m,
               'recall': float(np.count_nonzero(cnt_rec > 0)) / m,
               'density': float(cnt_prec.astype(np.int64).sum()) / (float(k) * m),
               'coverage': float(np.count_nonzero(min_rg <= kth_real)) / m,
               'diversity_fake': float(np.sum(sum_fake)) / pairs,
               'diversity_real': float(np.sum(sum_real)) / pairs}
    out['n_coverage'] = m
    return out


class CoverageEvaluator:
    """Precision / recall (Kynkaanniemi et al. 2019), density / coverage (Naeem et al. 2020) and
    diversity over whole clips, per speaker and pooled (COVERAGE_METRICS): the
    numbers that single out a generator which emits one plausible clip for every audio window.
    a2m's own restatement, pinned in float64 by tests/coverage_ref.py:

      feature   of a clip, float32 [D], in the generator's normalised space: 'pose' (D = T 2K) the
                generated clip as it is and the real one (x - mean) / std as the loader's gather
                normalises; 'motion' (D = (T - 1) 2K) their frame differences x[t] - x[t-1], in
                which a static clip is the zero vector
      d2(a,b)   max((|a|^2 + |b|^2) - 2 a.b, 0) in fp32 on the exact MFMA, within tol(a,b) =
                4 D 2^-24 (|a|^2 + |b|^2) of the exact value; two identical clips are within tol
                of 0, not necessarily at 0
      R, G      the real and the generated clips of one speaker, or of every speaker ('all': the
                pooled sets, no mean of the speakers' values); n = |R| = |G|
      r_k2(x)   of x in a set S: the k-th smallest d2(x, y) over the y of S at another position
                than x (a duplicate of x is a neighbour at distance about 0)
      precision       #{g : some r has d2(g,r) <= r_k2(r)} / n
      recall          #{r : some g has d2(r,g) <= r_k2(g)} / n
      density         sum_g #{r : d2(g,r) <= r_k2(r)} / (k n)
      coverage        #{r : min_g d2(r,g) <= r_k2(r)} / n
      diversity_fake  the mean of sqrt(d2(g_j, g_j')) over the pairs j != j', each root and the sums
                      in float64; diversity_real the same over R, the ceiling
      n_coverage      n; a set with n <= k has NaN metrics

    capacity: the most clips one pass holds (two [capacity, D] float32 buffers are allocated
    here); T: frames a clip; 1 <= k <= 32.  block_rows: the rows of a distance slab (the
    workspace is min(block_rows, n) x n floats, whatever n)."""

    def __init__(self, pose_mean, pose_std, n_styles, capacity, T, k=5, feature='pose', device='cuda',
                 block_rows=4096):
        self.device = torch.device(device)
        self.mean = torch.as_tensor(pose_mean).to(self.device, torch.float32).contiguous().reshape(-1)
        self.std = torch.as_tensor(pose_std).to(self.device, torch.float32).contiguous().reshape(-1)
        Fd = self.mean.numel()
        if self.std.numel() != Fd or Fd % 4 or Fd < 4:
            raise ValueError(f'pose_mean and pose_std must both hold a multiple of 4 values; got {Fd} and '
                             f'{self.std.numel()}')
        if feature not in F.COVERAGE_FEATURES:
            raise ValueError(f'unknown feature {feature!r}: one of {tuple(F.COVERAGE_FEATURES)}')
        if n_styles <= 0 or capacity <= 0 or block_rows <= 0 or not 1 <= k <= 32:
            raise ValueError('n_styles, capacity and block_rows must be positive and 1 <= k <= 32')
        if T <= F.COVERAGE_FEATURES[feature]:
            raise ValueError(f"feature {feature!r} needs T > {F.COVERAGE_FEATURES[feature]}, got {T}")
        self.n_styles, self.capacity, self.T, self.k = int(n_styles), int(capacity), int(T), int(k)
        self.feature, self.Fd, self.block_rows = feature, Fd, int(block_rows)
        self.D = (self.T - F.COVERAGE_FEATURES[feature]) * Fd
        self.feat_fake = torch.zeros(self.capacity, self.D, device=self.device)
        self.feat_real = torch.zeros(self.capacity, self.D, device=self.device)
        self.styles = torch.full((self.capacity,), -1, dtype=torch.int32, device=self.device)
        self.n = 0
        # the per-row results of every set (the speakers partition the clips, 'all' holds them
        # again) in one float64 arena, as PoseEvaluator's: result() reads them once
        R = 2 * self.capacity
        half = (R + 1) // 2
        sizes = [('kth_real', half, torch.float32), ('kth_fake', half, torch.float32), ('min_rg', half, torch.float32),
                 ('min_gr', half, torch.float32), ('cnt_prec', half, torch.int32), ('cnt_rec', half, torch.int32),
                 ('sum_real', R, torch.float64), ('sum_fake', R, torch.float64)]
        self._layout, n = [], 0
        for name, words, dtype in sizes:
            self._layout.append((name, n, words, dtype))
            n += words
        self._arena = torch.zeros(n, dtype=torch.float64, device=self.device)
        self._rows = self._views(self._arena)
        self._slab = None

    def _views(self, arena):
        return {name: arena[a:a + words].view(dtype) for name, a, words, dtype in self._layout}

    def reset(self):
        self.n = 0

    def state(self):
        """The pass so far as device tensors (views, not copies): feat_fake and feat_real [n, D], the
        feature rows in the order of the update() calls, styles int32 [n], and n, the row count."""
        n = self.n
        return {'feat_fake': self.feat_fake[:n], 'feat_real': self.feat_real[:n], 'styles': self.styles[:n], 'n': n}

    def update(self, fake_norm, real_px, style):
        """Adds one batch: fake_norm [n, T, 2K] the generator's normalised output, real_px [n, T, 2K]
        the neck-subtracted pose in pixels, style int32 [n] on the device (what
        PoseEvaluator.update gets).  One launch, no host synchronisation, no allocation.  The row the
        batch starts at is a host value (batch sizes are known on the host), so successive updates
        are not one node of a HIP graph that could be replayed across batches.  ValueError, before
        any launch, for a batch that does not fit into capacity."""
        n, T, Fd = fake_norm.shape
        if (T, Fd) != (self.T, self.Fd):
            raise ValueError(f'clips of [{T}, {Fd}]; the evaluator was built for [{self.T}, {self.Fd}]')
        if self.n + n > self.capacity:
            raise ValueError(f'{self.n} + {n} clips exceed the capacity {self.capacity}')
        if n == 0:
            return
        F.coverage_store(fake_norm, real_px, style, self.mean, self.std, self.n, self.feat_fake, self.feat_real,
                         self.styles, self.feature)
        self.n += n

    def _slab_for(self, na, m):
        if self._slab is None or self._slab.numel() < na * m:
            self._slab = torch.empty(na * m, device=self.device)
        return self._slab[:na * m].view(na, m)

    def result(self, per_row=False):
        """{style id: metrics, ..., 'all': metrics}; metrics holds COVERAGE_METRICS.  Reads the
        styles, builds the row list of every speaker and of 'all' (the clips whose style is in
        range) on the host, and per set runs R|R and G|G (the radii and the diversity sums), then
        G|R (precision, density) and R|G (recall, coverage), a slab of at most block_rows rows at
        a time; the per-row vectors are read back once.  per_row=True returns (that dict, {key:
        per-row vectors}) for the sets with more than k clips: rows (positions in state()'s
        buffers), kth_real and kth_fake (the radii r_k2), cnt_prec (per generated clip, the real
        balls it lies in), cnt_rec (per real clip, the generated balls it lies in), min_rg (per
        real clip, the distance to the nearest generated one), sum_real and sum_fake (the row
        sums of sqrt d2): which clips are off the manifold, and which are not covered."""
        S, k, n = self.n_styles, self.k, self.n
        styles = self.styles[:n].cpu().numpy()
        sets = [(s, np.flatnonzero(styles == s)) for s in range(S)]
        sets.append(('all', np.flatnonzero((styles >= 0) & (styles < S))))
        live = [(key, rows) for key, rows in sets if len(rows) > k]
        spans, o = {}, 0
        for key, rows in live:
            spans[key] = (o, len(rows))
            o += len(rows)
        if live:
            rows_dev = torch.from_numpy(np.concatenate([rows for _, rows in live]).astype(np.int32)).to(self.device)
        v = self._rows
        for key, _ in live:
            o, m = spans[key]
            rows = rows_dev[o:o + m]
            blocks = [(a0, min(self.block_rows, m - a0)) for a0 in range(0, m, self.block_rows)]
            for feat, kth, sums in ((self.feat_real, v['kth_real'], v['sum_real']),
                                    (self.feat_fake, v['kth_fake'], v['sum_fake'])):
                for a0, na in blocks:
                    slab = F.pair_dist2(feat, rows[a0:a0 + na], feat, rows, True, a0, self._slab_for(na, m))
                    F.row_kth(slab, k, True, kth[o + a0:o + a0 + na], sums[o + a0:o + a0 + na])
            for fa, fb, r2, cnt, low in ((self.feat_fake, self.feat_real, v['kth_real'], v['cnt_prec'], v['min_gr']),
                                         (self.feat_real, self.feat_fake, v['kth_fake'], v['cnt_rec'], v['min_rg'])):
                for a0, na in blocks:
                    slab = F.pair_dist2(fa, rows[a0:a0 + na], fb, rows, out=self._slab_for(na, m))
                    F.row_cover(slab, r2[o:o + m], cnt[o + a0:o + a0 + na], low[o + a0:o + a0 + na])
        host = {name: t.numpy() for name, t in self._views(self._arena.cpu()).items()} if live else {}
        names = ('kth_real', 'cnt_prec', 'cnt_rec', 'min_rg', 'sum_real', 'sum_fake')
        out = {}
        for key, rows in sets:
            if key in spans:
                o, m = spans[key]
                out[key] = _coverage_metrics(k, *(host[name][o:o + m] for name in names))
            else:
                out[key] = _coverage_metrics(k, *(np.zeros(len(rows)) for _ in names))
        if not per_row:
            return out
        vectors = {}
        for key, rows in live:
            o, m = spans[key]
            vectors[key] = dict({name: host[name][o:o + m].copy() for name in names + ('kth_fake',)}, rows=rows)
        return out, vectors


def evaluate(generator, loader, split='test', pose_mean=None, pose_std=None, audio_mean=None, audio_std=None,
             sync=False, sync_kwargs=None, beat_sigma=1.0, coverage=False, coverage_kwargs=None,
             **evaluator_kwargs):
    """One evaluation pass of `generator` over a split of a PatsLoader: result() of a PoseEvaluator,
    keyed by speaker name (loader.speaker_dict), 'all' and 'dropped'.  pose_mean, pose_std: the
    statistics the generator was trained with (its output is de-normalised with them);
    audio_mean, audio_std: the audio is standardised with them when given.  The real poses come
    neck-subtracted and not normalised, as generate_motion_video.py:247-251 compares them.  The
    generator runs in eval mode under no_grad and gets its training flags back.
    sync=True adds the SYNC_METRICS of an AudioSyncEvaluator(**sync_kwargs) to every speaker's entry
    and to 'all' (two more launches a batch and a second host read after the last batch); it gets
    the audio the generator got and the audio_std it was standardised with.  beat_sigma: see
    AudioSyncEvaluator.result.
    coverage=True adds the COVERAGE_METRICS of a CoverageEvaluator(**coverage_kwargs: k, feature,
    block_rows), sized from the split's clip count in the loader's tables, to every speaker's entry
    and to 'all': one more launch a batch, from the tensors PoseEvaluator.update gets, and the
    distance passes of CoverageEvaluator.result() after the last batch.  Without it nothing of the
    kind is constructed or launched."""
    if pose_mean is None or pose_std is None:
        raise ValueError('evaluate needs pose_mean and pose_std')
    ev = PoseEvaluator(pose_mean, pose_std, len(loader.speaker_dict), device=loader.device, **evaluator_kwargs)
    sev = AudioSyncEvaluator(len(loader.speaker_dict), audio_std=audio_std, device=loader.device,
                             **(sync_kwargs or {})) if sync else None
    cev = None
    if coverage:
        pose = next(m for m in loader.modalities if m.startswith('pose'))
        cev = CoverageEvaluator(pose_mean, pose_std, len(loader.speaker_dict), max(loader.index.size(split), 1),
                                loader.index.geometry(pose)[2], device=loader.device, **(coverage_kwargs or {}))
    zero, one = torch.zeros_like(ev.mean), torch.ones_like(ev.std)
    flags = [(m, m.training) for m in generator.modules()]
    generator.eval()
    try:
        with torch.no_grad():
            for audio, real_px, style in loader.pairs(split, zero, one, audio_mean, audio_std, with_style=True):
                fake = generator(audio)
                fake = fake[0] if isinstance(fake, (tuple, list)) else fake
                ev.update(fake, real_px, style)
                if sev is not None:
                    sev.update(audio, ev.fake_px(*real_px.shape[:2]), real_px, style)
                if cev is not None:
                    cev.update(fake, real_px, style)
    finally:
        for m, flag in flags:
            m.training = flag
    res = ev.result()
    if sev is not None:
        for key, extra in sev.result(beat_sigma).items():
            res[key].update(extra)
    if cev is not None:
        for key, extra in cev.result().items():
            res[key].update(extra)
    out = {name: res[i] for name, i in loader.speaker_dict.items()}
    out['all'], out['dropped'] = res['all'], res['dropped']
    return out
