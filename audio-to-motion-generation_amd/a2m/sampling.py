"""Train samplers for the HBM loader: which clips a training pass sees, and in which order
(dataUtils.py's Data_Loader.get_train_sampler, AlternateClassSampler and BalanceClassSampler for the
pose and audio modalities).

  make_sampler   PatsLoader.train_sampler's body: picks the sampler from the reference's arguments,
                 in the reference's precedence
  TrainSampler   what it returns: .draw() is one pass's order, int64 [M] global indices of the
                 split on the host, new at every call; len(), .kind, .classes

The velocity samplers (quantile_sample) bin the clips by their mean joint speed.  That statistic is
computed where the clips are: PatsLoader.clip_velocity reads the arena in place
(a2m_clip_velocity_f32), a2m_select_f32 finds the exact order statistics a quantile needs, and
a2m_classify_f32 bins the clips; a handful of scalars and one int32 class table come back to the
host, once, at construction.  With velocity= (a host array) the same definitions run in numpy.  A
pass is then what it is without a sampler: one order uploaded, one gather launch a batch.

Definitions (n clips in the split, B the loader's global batch size):
  alternate   style_iters > 0: classes = the speakers' clips, ascending speaker id; m = style_iters *
              B // n_classes draws of torch.randint(0, len(class), (m,)) per class, class by class;
              position p of the order belongs to class p mod n_classes
  few_shot    num_training_sample = k: torch.randperm(n)[:k] at construction, each pass in
              torch.utils.data.SubsetRandomSampler's order
  above       quantile_sample = q in [0, 1): the clips with velocity > Q(q)
  tail        quantile_sample = [q0, q1]: the clips with velocity > Q(q1) or < Q(q0)
  rebalance   quantile_sample = q > 1 with quantile_num_training_sample = s: int(q) equal-width bins
              from the smallest to the largest velocity (edges min + j (max - min) / q in float64,
              the last one max itself; both ends of a bin closed, a value on an inner edge in the
              lower bin), empty bins dropped; m = s * B // n_classes draws per class as alternate
  weighted    weighted = w: torch.utils.data.WeightedRandomSampler([1] * n, w * B)
  iters       num_training_iters = it: RandomSampler(range(n), replacement=True, num_samples=it * B)
Q is numpy's default (linear) quantile, computed in float64 from the two order statistics at
floor and ceil of q (n - 1).
"""
import math
import numbers

import numpy as np
import torch
from torch.utils.data import RandomSampler, SubsetRandomSampler, WeightedRandomSampler

KINDS = ('alternate', 'few_shot', 'above', 'tail', 'rebalance', 'weighted', 'iters')


def quantile_ranks(q, n):
    """(floor, ceil) of q (n - 1): the two ranks Q(q) interpolates between."""
    pos = q * (n - 1)
    return int(math.floor(pos)), int(math.ceil(pos))


def quantile_lerp(q, n, a, b):
    """Q(q) from the order statistics a, b at quantile_ranks(q, n), in float64."""
    pos = q * (n - 1)
    a, b = float(a), float(b)
    return a + (pos - math.floor(pos)) * (b - a)


def bin_edges(vmin, vmax, q):
    """The q + 1 edges of q equal-width bins over [vmin, vmax], float64, the last one vmax exactly."""
    vmin, vmax = float(vmin), float(vmax)
    edges = [vmin + j * (vmax - vmin) / q for j in range(q + 1)]
    edges[-1] = vmax
    return edges


def classify_host(v, kind, thr):
    """a2m_classify_f32's definitions in numpy, float64: int32 [n] classes, -1 for none."""
    v = np.asarray(v, np.float64)
    if kind == 'above':
        return np.where(v > thr[0], 0, -1).astype(np.int32)
    if kind == 'tail':
        return np.where((v > thr[1]) | (v < thr[0]), 0, -1).astype(np.int32)
    cls = np.full(v.shape, -1, np.int32)
    for j in range(len(thr) - 2, -1, -1):           # descending: the first matching bin is written last
        cls[(thr[j] <= v) & (v <= thr[j + 1])] = j
    return cls


def _parse_quantile(q, s):
    """(kind, q) of a quantile_sample argument; every refusal is a ValueError."""
    if isinstance(q, (list, tuple)):
        if len(q) != 2 or not all(isinstance(x, numbers.Real) and 0 <= x <= 1 for x in q):
            raise ValueError(f'quantile_sample: a list must hold two quantiles in [0, 1], got {q!r}')
        return 'tail', [float(q[0]), float(q[1])]
    if not isinstance(q, numbers.Real) or q != q:
        raise ValueError(f'quantile_sample: a number or a list of two, got {q!r}')
    if q < 0 or q == 1:
        raise ValueError(f'quantile_sample: {q!r} is neither a quantile in [0, 1) nor a number of bins > 1')
    if q < 1:
        return 'above', float(q)
    if s is None:
        raise ValueError(f'quantile_sample={q!r} rebalances {int(q)} velocity bins and needs '
                         'quantile_num_training_sample')
    return 'rebalance', int(q)


class TrainSampler:
    """One of KINDS over the n clips of a split.  classes: the int64 index lists the draws go into
    (one list for few_shot, above and tail; none for weighted and iters, which draw from range(n))."""

    def __init__(self, kind, split, n, classes=(), per_class=0, num_samples=0, generator=None, thresholds=None):
        assert kind in KINDS
        self.kind, self.split, self.n, self.generator = kind, split, n, generator
        self.classes = [np.ascontiguousarray(c, dtype=np.int64) for c in classes]
        self.per_class, self.num_samples = per_class, num_samples
        self.thresholds = thresholds            # above / tail: the quantile values; rebalance: the edges
        if kind in ('few_shot', 'above', 'tail'):
            self._torch = SubsetRandomSampler(self.classes[0].tolist(), generator=generator)
        elif kind == 'weighted':
            self._torch = WeightedRandomSampler([1] * n, num_samples, generator=generator)
        elif kind == 'iters':
            self._torch = RandomSampler(range(n), replacement=True, num_samples=num_samples, generator=generator)

    def __len__(self):
        if self.kind in ('alternate', 'rebalance'):
            return self.per_class * len(self.classes)
        if self.kind in ('few_shot', 'above', 'tail'):
            return len(self.classes[0])
        return self.num_samples

    def draw(self):
        """One pass's order: int64 [len(self)] global indices of the split, on the host."""
        if self.kind in ('alternate', 'rebalance'):
            if not len(self):
                return np.zeros(0, np.int64)
            cols = [c[torch.randint(0, len(c), (self.per_class,), generator=self.generator).numpy()]
                    for c in self.classes]
            return np.stack(cols, axis=1).reshape(-1)
        return np.asarray(list(self._torch), np.int64).reshape(-1)


def _count(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError(f'{name} must be an integer >= 0, got {v!r}')
    return int(v)


def _velocity_classes(loader, split, n, kind, q, velocity):
    """(thresholds, int32 [n] classes, -1 for none) of a quantile sampler: in numpy from a host
    velocity array, else on the device from loader.clip_velocity(split)."""
    if kind == 'rebalance':
        ranks = [0]
    elif kind == 'above':
        ranks = list(quantile_ranks(q, n))
    else:
        ranks = [r for x in q for r in quantile_ranks(x, n)]
    if velocity is not None:
        v = np.asarray(torch.as_tensor(velocity).cpu().numpy(), np.float64).reshape(-1)
        if v.size != n:
            raise ValueError(f'velocity holds {v.size} values for the {n} clips of {split}')
        bad = int((~np.isfinite(v)).sum())
        if bad:
            raise ValueError(f'{bad} of the {n} clips of {split} have a non-finite velocity')
        ordered = np.sort(v)
        stats, vmin, vmax = ordered[ranks], ordered[0], ordered[-1]
    else:
        from . import functional as F
        vel = loader.clip_velocity(split)
        bad = int(loader._velocity_bad[split].item())
        if bad:
            raise ValueError(f'{bad} of the {n} clips of {split} have a non-finite velocity')
        stats, minmax = F.select(vel, ranks)
        stats, (vmin, vmax) = stats.cpu().numpy().astype(np.float64), minmax.cpu().numpy().astype(np.float64)
    if kind == 'rebalance':
        thr, ckind = bin_edges(vmin, vmax, q), 'bins'
    elif kind == 'above':
        thr, ckind = [quantile_lerp(q, n, stats[0], stats[1])], 'above'
    else:
        thr, ckind = [quantile_lerp(x, n, stats[2 * i], stats[2 * i + 1]) for i, x in enumerate(q)], 'tail'
    if velocity is not None:
        return thr, classify_host(v, ckind, thr)
    cls, _ = F.classify(vel, ckind, thr)
    return thr, cls.cpu().numpy()


def make_sampler(loader, split='train', *, style_iters=0, num_training_sample=None, quantile_sample=None,
                 quantile_num_training_sample=None, weighted=0, num_training_iters=None, sample_all_styles=0,
                 velocity=None, generator=None):
    """PatsLoader.train_sampler: a TrainSampler, or None where nothing is set (the ordinary shuffle)."""
    if sample_all_styles:
        raise NotImplementedError(f'sample_all_styles={sample_all_styles!r} is not supported (only 0)')
    ix = loader.index
    n, B = ix.size(split), loader.batch_size
    if generator is None:
        generator = loader.generator
    style_iters = _count('style_iters', style_iters)
    weighted = _count('weighted', weighted)
    chosen = (style_iters > 0 or num_training_sample is not None or quantile_sample is not None or weighted > 0
              or num_training_iters is not None)
    if not chosen:
        return None
    if n == 0:
        raise ValueError(f'{split} holds no clips to sample from')
    if style_iters > 0:
        styles = np.concatenate([np.full(k, ix.style[iid], np.int64)
                                 for iid, k in zip(ix.intervals[split], ix.sizes[split])])
        classes = [np.flatnonzero(styles == s) for s in np.unique(styles)]
        return TrainSampler('alternate', split, n, classes, style_iters * B // len(classes), generator=generator)
    if num_training_sample is not None:
        k = _count('num_training_sample', num_training_sample)
        subset = torch.randperm(n, generator=generator)[:k].numpy()
        return TrainSampler('few_shot', split, n, [subset], generator=generator)
    if quantile_sample is not None:
        kind, q = _parse_quantile(quantile_sample, quantile_num_training_sample)
        thr, cls = _velocity_classes(loader, split, n, kind, q, velocity)
        if kind != 'rebalance':
            return TrainSampler(kind, split, n, [np.flatnonzero(cls == 0)], generator=generator, thresholds=thr)
        s = _count('quantile_num_training_sample', int(quantile_num_training_sample))
        classes = [c for c in (np.flatnonzero(cls == j) for j in range(q)) if len(c)]
        return TrainSampler('rebalance', split, n, classes, s * B // len(classes), generator=generator,
                            thresholds=thr)
    if weighted > 0:
        return TrainSampler('weighted', split, n, num_samples=weighted * B, generator=generator)
    it = _count('num_training_iters', num_training_iters)
    return TrainSampler('iters', split, n, num_samples=it * B, generator=generator)
