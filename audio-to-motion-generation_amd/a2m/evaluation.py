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
"""
import numpy as np
import torch

from . import functional as F
from ._native import check, lib

METRICS = ('pck', 'l1', 'fd', 'w1_speed', 'w1_accel', 'mean_speed_real', 'mean_speed_fake', 'n_clips',
           'n_frames', 'speed_overflow', 'accel_overflow')


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


def evaluate(generator, loader, split='test', pose_mean=None, pose_std=None, audio_mean=None, audio_std=None,
             **evaluator_kwargs):
    """One evaluation pass of `generator` over a split of a PatsLoader: result() of a PoseEvaluator,
    keyed by speaker name (loader.speaker_dict), 'all' and 'dropped'.  pose_mean, pose_std: the
    statistics the generator was trained with (its output is de-normalised with them);
    audio_mean, audio_std: the audio is standardised with them when given.  The real poses come
    neck-subtracted and not normalised, as generate_motion_video.py:247-251 compares them.  The
    generator runs in eval mode under no_grad and gets its training flags back."""
    if pose_mean is None or pose_std is None:
        raise ValueError('evaluate needs pose_mean and pose_std')
    ev = PoseEvaluator(pose_mean, pose_std, len(loader.speaker_dict), device=loader.device, **evaluator_kwargs)
    zero, one = torch.zeros_like(ev.mean), torch.ones_like(ev.std)
    flags = [(m, m.training) for m in generator.modules()]
    generator.eval()
    try:
        with torch.no_grad():
            for audio, real_px, style in loader.pairs(split, zero, one, audio_mean, audio_std, with_style=True):
                fake = generator(audio)
                ev.update(fake[0] if isinstance(fake, (tuple, list)) else fake, real_px, style)
    finally:
        for m, flag in flags:
            m.training = flag
    res = ev.result()
    out = {name: res[i] for name, i in loader.speaker_dict.items()}
    out['all'], out['dropped'] = res['all'], res['dropped']
    return out
