"""The three trivial predictors a gesture metric is published beside (Speech2Gesture, PATS), over
the clips a PatsLoader already keeps in HBM, so that a2m.evaluation.evaluate can say what a
checkpoint's PCK / L1 / Frechet / W1 are worth:

  MedianPose    always the median training pose (neck-subtracted pixels, per channel, exact)
  RandomClip    the poses of a randomly drawn training clip
  NearestAudio  the poses of the training clip whose audio window is nearest to the query's

Each is a parameter-free torch.nn.Module with the generator's call surface: forward(audio
[n, T, 128], real_pose=None) -> (pose [n, T, 104], None), the poses normalised exactly as
loader.pairs(split, pose_mean, pose_std) normalises them, so evaluate's de-normalisation gives the
pixels back.  The median and the search are kernels of their own (csrc/baselines.hip) that read the
loader's arena through its start table in place; the clips come from the loader's one-launch gather.

Out of scope: restricting the neighbours to the query's speaker, excluding the query's own interval
(evaluate on another split than the one searched), k > 1 neighbours, bf16, a data-parallel search.
"""
import torch

from . import functional as F
from .data import MODE_NECKSUB


def _stat(t, loader, C, name):
    t = torch.as_tensor(t).to(loader.device, torch.float32).contiguous()
    if t.numel() != C:
        raise ValueError(f'{name} must hold {C} values, got {t.numel()}')
    return t


class _Baseline(torch.nn.Module):
    """What the three share: the loader's pose and audio modality, their geometry, the table range of
    the split and the pose statistics."""

    def __init__(self, loader, pose_mean, pose_std, split='train'):
        super().__init__()
        pose = [m for m in loader.modalities if m.startswith('pose')]
        audio = [m for m in loader.modalities if m.startswith('audio')]
        if len(pose) != 1 or len(audio) != 1:
            raise ValueError(f'the baselines need a loader with one pose and one audio modality, got '
                             f'{tuple(loader.modalities)}')
        self.loader, self.split = loader, split
        self.pose, self.audio = pose[0], audio[0]
        self.pose_geo, self.audio_geo = loader.index.geometry(self.pose), loader.index.geometry(self.audio)
        if self.pose_geo[2] != self.audio_geo[2]:
            raise ValueError(f'pose windows hold {self.pose_geo[2]} rows, audio windows {self.audio_geo[2]}')
        self.T = self.pose_geo[2]
        if loader.channels[self.pose] != 104:
            raise ValueError(f'{self.pose}: the poses must be planar [2][52], got {loader.channels[self.pose]} channels')
        self.base, self.n = loader.base[split], loader.index.size(split)
        if self.n == 0:
            raise ValueError(f'the {split} split of the loader holds no clip')
        if pose_mean is None or pose_std is None:
            raise ValueError('the baselines need pose_mean and pose_std')
        self.pose_mean = _stat(pose_mean, loader, 104, 'pose_mean')
        self.pose_std = _stat(pose_std, loader, 104, 'pose_std')

    def _check_audio(self, audio):
        C = self.loader.channels[self.audio]
        if audio.dim() != 3 or tuple(audio.shape[1:]) != (self.T, C):
            raise ValueError(f'audio must be [n, {self.T}, {C}], got {tuple(audio.shape)}')

    def _clips(self, positions):
        """The normalised poses of the clips at start-table positions `positions` (device int64)."""
        spec = (self.pose, MODE_NECKSUB, self.pose_mean, self.pose_std)
        return self.loader.gather(positions, 0, positions.numel(), [spec])[0]


class MedianPose(_Baseline):
    """Always the per-channel median of the split's neck-subtracted poses (every row of every
    window: a frame that overlapping windows share counts once per window, the population
    get_mean_std_necksub averages).  median_px [104] is computed once, here."""

    def __init__(self, loader, pose_mean, pose_std, split='train'):
        super().__init__(loader, pose_mean, pose_std, split)
        window, interval, _ = self.pose_geo
        self.median_px = F.window_median(loader.arena[self.pose], loader.start[self.pose], self.base, self.n,
                                         window, interval, necksub=True)
        self.median_norm = (self.median_px - self.pose_mean) / self.pose_std

    def forward(self, audio, real_pose=None):
        self._check_audio(audio)
        return self.median_norm.expand(audio.shape[0], self.T, 104).contiguous(), None


class RandomClip(_Baseline):
    """The poses of clips drawn uniformly from the split, on the device (torch.randint with
    `generator`, a generator of the loader's device); last_index [n]: the drawn clips, as indices
    within the split."""

    def __init__(self, loader, pose_mean, pose_std, split='train', generator=None):
        super().__init__(loader, pose_mean, pose_std, split)
        self.generator = generator
        self.last_index = None

    def forward(self, audio, real_pose=None):
        self._check_audio(audio)
        self.last_index = torch.randint(0, self.n, (audio.shape[0],), device=self.loader.device,
                                        generator=self.generator)
        return self._clips(self.last_index + self.base), None


class NearestAudio(_Baseline):
    """The poses of the split's clip whose audio window is nearest (squared L2 over the window) to
    each query's.  With audio_mean / audio_std the candidates are standardised as the queries then
    are (loader.pairs, evaluate).  One search (two launches) and one gather; no host read and no
    synchronisation.  last_index [n] (within the split) and last_distance [n]: the last forward's."""

    def __init__(self, loader, pose_mean, pose_std, audio_mean=None, audio_std=None, split='train'):
        super().__init__(loader, pose_mean, pose_std, split)
        if (audio_mean is None) != (audio_std is None):
            raise ValueError('mean and std come together')
        C = loader.channels[self.audio]
        self.audio_mean = None if audio_mean is None else _stat(audio_mean, loader, C, 'audio_mean')
        self.audio_std = None if audio_std is None else _stat(audio_std, loader, C, 'audio_std')
        self.last_index = self.last_distance = None

    def forward(self, audio, real_pose=None):
        self._check_audio(audio)
        window, interval, _ = self.audio_geo
        best, self.last_distance = F.nn_search(audio, self.loader.arena[self.audio], self.loader.start[self.audio],
                                               self.base, self.n, window, interval, self.audio_mean, self.audio_std)
        self.last_index = best - self.base
        return self._clips(best), None


def evaluate_baselines(loader, split='test', pose_mean=None, pose_std=None, audio_mean=None, audio_std=None,
                       generator=None, **evaluate_kwargs):
    """evaluate() of the three baselines, built from the loader's training split, over `split`:
    {'median': ..., 'random': ..., 'nearest': ...}, each value evaluate's result.  generator: the
    device generator RandomClip draws with."""
    from .evaluation import evaluate
    models = {'median': MedianPose(loader, pose_mean, pose_std),
              'random': RandomClip(loader, pose_mean, pose_std, generator=generator),
              'nearest': NearestAudio(loader, pose_mean, pose_std, audio_mean, audio_std)}
    return {name: evaluate(model, loader, split, pose_mean=pose_mean, pose_std=pose_std, audio_mean=audio_mean,
                           audio_std=audio_std, **evaluate_kwargs) for name, model in models.items()}
