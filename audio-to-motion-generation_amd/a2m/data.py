"""The PATS loader, resident in HBM: pats/data_loading/dataUtils.py's
Data_Loader for the pose and audio modalities, without pandas, h5py or a host collate.

  PatsIndex   the host-side index arithmetic, no native call: the interval table, the speaker
              filter and speaker_dict (dataUtils.py:111-132), tdt_split (:177-237, 259-272), the
              per-interval windows (a2m.windowing.window_index, :585-628), the ConcatDataset
              mapping of a global sample index (:741-758) and the epoch order a
              DataLoader(shuffle=True) would draw
  PatsLoader  every interval of every split in one device arena per modality; .train / .dev /
              .test yield the reference's batch dict, .pairs(split, ...) yields the paired and
              already normalised (audio, real_pose) that GANTrainer.fit and validate consume.
              A pass uploads one permutation; a batch is one launch of a2m_batch_gather_f32
              (csrc/data.hip), which reads the permutation on the device.
  Augment     settings of the train-time augmentation that .pairs(..., augment=) applies inside
              the gather (csrc/augment.hip): tempo, mirror, scale, gain, masks, drawn per clip on
              the device from a counter-based generator; off by default
  dp_plan     which rows of which global batch a data-parallel rank takes

PatsLoader.train_sampler gives the reference's train samplers (a2m/sampling.py: alternating
speakers, few-shot, the velocity quantiles and bins, weighted, fixed iterations);
.pairs(..., sampler=) and .sampled(split, sampler) draw each pass's order from one.

Audio and pose of a clip come from the same sample of the same pass, and the poses are
normalised in the gather: the reference's two separately shuffled passes
(version5_model_train.py:296-319) have no counterpart here.

HDF5 reading stays out of scope (h5py is absent): the arrays come from the caller, as a dict or
as the .npz that PatsLoader.save_arrays writes.
"""
import bisect
import csv
import ctypes
import os
from collections.abc import Mapping

import numpy as np
import torch
from torch.utils.data import DataLoader

from .windowing import PatsClip, window_index

COLUMNS = ('dataset', 'delta_time', 'end_time', 'interval_id', 'speaker', 'start_time', 'video_fn',
           'video_link')
SPLITS = ('train', 'dev', 'test')
MODE_RAW, MODE_STANDARDISE, MODE_NECKSUB = 0, 1, 2
ROLE_NONE, ROLE_POSE, ROLE_AUDIO = 0, 1, 2      # what gather_augmented applies to a modality
MAX_MOD = 4

# Data_Loader arguments the constructor refuses, with the only value accepted for each, the
# reference's default: the text options are not built, and the train samplers are asked for
# through PatsLoader.train_sampler (a2m/sampling.py), not here
UNSUPPORTED = {'style_iters': 0, 'num_training_sample': None, 'sample_all_styles': 0, 'repeat_text': 1,
               'quantile_sample': None, 'quantile_num_training_sample': None, 'weighted': 0,
               'filler': False, 'num_training_iters': None}


def _refuse_unsupported(modalities, kwargs):
    for name, value in kwargs.items():
        if name not in UNSUPPORTED:
            raise TypeError(f'unexpected argument {name!r}')
        default = UNSUPPORTED[name]
        if not (value is default or (default is not None and value is not None and value == default)):
            raise NotImplementedError(f'{name}={value!r} is not supported (only {default!r})')
    for mod in modalities:
        if 'text' in mod:
            raise NotImplementedError(f'modalities: the text modality {mod!r} is not supported')


def _read_table(table):
    """One table (a CSV path or a list of rows) or a list of tables -> rows as
    {'dataset', 'interval_id', 'speaker'} dicts of strings, appended in order."""
    def rows_of(t):
        if isinstance(t, (str, os.PathLike)):
            with open(t, newline='') as f:
                return list(csv.DictReader(f))
        return [r if isinstance(r, Mapping) else dict(zip(COLUMNS, r)) for r in t]

    def is_table(t):
        return isinstance(t, (str, os.PathLike)) or (
            isinstance(t, (list, tuple)) and (not t or isinstance(t[0], (Mapping, list, tuple))))

    if isinstance(table, (str, os.PathLike)):
        tables = [table]
    elif len(table) and all(is_table(t) for t in table):
        tables = list(table)
    else:
        tables = [table]
    return [{'dataset': str(r['dataset']), 'interval_id': str(r['interval_id']), 'speaker': str(r['speaker'])}
            for t in tables for r in rows_of(t)]


def dp_plan(n_samples, batch_size, rank=0, world=1):
    """The rows of an epoch's order that `rank` of `world` takes: from each global batch of n
    clips, rows [rank*m, (rank+1)*m) with m = n // world.  Returns ([(b0, m), ...] as positions
    into the order, dropped): a global batch with m == 0 is skipped on every rank, and dropped
    counts the n % world leftover clips nobody takes."""
    assert 0 <= rank < world and batch_size > 0
    plan, dropped = [], 0
    for g0 in range(0, n_samples, batch_size):
        n = min(batch_size, n_samples - g0)
        m = n // world
        dropped += n - m * world
        if m:
            plan.append((g0 + rank * m, m))
    return plan, dropped


class PatsIndex:
    """lengths: {interval_id: {modality: number of rows}}; table, speaker, split, missing,
    load_data, time, window_hop as Data_Loader's."""

    def __init__(self, lengths, table, speaker, modalities=('pose/data', 'audio/log_mel_512'),
                 fs_new=(15, 15), time=4.3, split=None, window_hop=0, load_data=True, missing=(),
                 **unsupported):
        _refuse_unsupported(modalities, unsupported)
        assert len(modalities) == len(fs_new), 'one fs_new per modality'
        self.modalities = tuple(modalities)
        self.fs_new = tuple(fs_new)
        self.split = split
        self.load_data = load_data
        self.lengths = lengths
        names = [speaker] if isinstance(speaker, str) else list(speaker)
        rows = _read_table(table)
        if names[0] == 'all':
            names = list(dict.fromkeys(r['speaker'] for r in rows))
        self.speaker = names
        self.rows = [r for r in rows if r['speaker'] in names]
        self.speaker_dict = {sp: i for i, sp in enumerate(names)}
        assert len(self.rows), 'speaker `{}` not found'.format(speaker)
        self.missing = self._with_transforms(set(str(i) for i in missing))
        self.intervals = self.tdt_split()
        absent = [iid for ids in self.intervals.values() for iid in ids if iid not in lengths]
        if absent:
            raise KeyError(f'{len(absent)} intervals of the table have no arrays (name them in missing= to '
                           f'leave them out): {absent[:5]}')
        by_id = {}
        for r in self.rows:
            by_id.setdefault(r['interval_id'], r['speaker'])
        self.style = {iid: self.speaker_dict[by_id[iid]] for ids in self.intervals.values() for iid in ids}
        self.update_dataloaders(time, window_hop)

    def _with_transforms(self, missing):
        """get_transforms_missing_intervals: for speakers named x|t, '<id>|t' of every missing id."""
        transforms = sorted({sp.split('|')[-1] for sp in self.speaker if '|' in sp})
        return missing | {'{}|{}'.format(i, t) for t in transforms for i in missing}

    def tdt_split(self):
        rows = self.rows
        if not self.split:
            parts = [[r for r in rows if r['dataset'] == s] for s in SPLITS]
        else:
            n = len(rows)
            end_train = int(n * self.split[0])
            end_dev = int(end_train + n * self.split[1])
            parts = [rows[:end_train], rows[end_train:end_dev], rows[end_dev:]]
        out = {}
        for s, part in zip(SPLITS, parts):
            ids = sorted(set(r['interval_id'] for r in part) - self.missing)
            out[s] = ids if self.load_data else ids[:5]
        return out

    def update_dataloaders(self, time, window_hop):
        """MiniData.update_idx_list for every interval of every split, and the cumulative sizes."""
        self.time, self.window_hop = time, window_hop
        self.windows, self.sizes, self.cumulative_sizes = {}, {}, {}
        for s in SPLITS:
            self.windows[s] = [
                {mod: window_index(int(self.lengths[iid][mod]), mod, fn, time, window_hop)
                 for mod, fn in zip(self.modalities, self.fs_new)} for iid in self.intervals[s]]
            self.sizes[s] = [min(len(ix[0]) for ix in w.values()) for w in self.windows[s]]
            self.cumulative_sizes[s] = np.cumsum(self.sizes[s], dtype=np.int64).tolist()

    def geometry(self, modality):
        """(window, interval, T) of a modality's windows."""
        fs_new = self.fs_new[self.modalities.index(modality)]
        _, window, interval = window_index(0, modality, fs_new, self.time, self.window_hop)
        return window, interval, (window + interval - 1) // interval

    def size(self, split):
        return self.cumulative_sizes[split][-1] if self.cumulative_sizes[split] else 0

    def locate(self, split, idx):
        """ConcatDatasetIndex.__getitem__'s mapping: global index -> (interval position, local index)."""
        n, cum = self.size(split), self.cumulative_sizes[split]
        if idx < 0:
            if -idx > n:
                raise ValueError('absolute value of index should not exceed dataset length')
            idx = n + idx
        if idx >= n:
            raise IndexError('index {} out of range for {} samples'.format(idx, n))
        k = bisect.bisect_right(cum, idx)
        return k, int(idx - (cum[k - 1] if k else 0))

    def order(self, split, shuffle=True, generator=None):
        """One epoch's sample order, int64 [N]: arange, or with shuffle=True what
        DataLoader(ConcatDataset(...), shuffle=True) draws -- a DataLoader over the indices draws
        it here, so the global (or the given) generator is consumed exactly as a full pass of the
        reference's loader consumes it, whatever the batch size."""
        n = self.size(split)
        if n == 0:
            return np.zeros(0, np.int64)
        if not shuffle:
            return np.arange(n, dtype=np.int64)
        loader = DataLoader(range(n), batch_size=n, shuffle=True, generator=generator,
                            collate_fn=lambda b: np.asarray(b, np.int64))
        return np.concatenate(list(loader))

    def batches(self, split, batch_size, shuffle=True, generator=None):
        """The global sample indices of each batch of one epoch; the last may be partial."""
        order = self.order(split, shuffle, generator)
        for b0 in range(0, len(order), batch_size):
            yield order[b0:b0 + batch_size]

    def meta_times(self, split):
        """(start, end) seconds of every sample of a split, float64 [N, 2] (PatsClip.window_times)."""
        first, last = self.modalities[0], self.modalities[-1]
        out = [PatsClip.window_times(w[first], w[last], self.fs_new, np.arange(n))
               for w, n in zip(self.windows[split], self.sizes[split])]
        return np.concatenate(out) if out else np.zeros((0, 2))


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _i32s(vs):
    return (ctypes.c_int32 * len(vs))(*vs)


class Augment:
    """Settings of the train-time augmentation that PatsLoader.pairs(..., augment=) applies inside
    its gather (csrc/augment.hip); every parameter is drawn per clip on the device, and everything
    is off by default: Augment() is the identity.

      seed        the Philox key; a clip's parameters depend on (seed, pass, start-table position) only
      p_mirror    probability of a left-right mirrored pose (needs pose statistics), in [0, 1]
      speed       tempo: both modalities are read at speed s, uniform in [1 - speed, 1 + speed]; in [0, 0.5]
      scale       the neck-subtracted pose times g, uniform in [1 - scale, 1 + scale]; in [0, 1)
      gain        added to the log-mel values, uniform in [-gain, gain]
      freq_mask   one band of 0 .. freq_mask audio channels is written as mask_fill
      time_mask   one run of 0 .. time_mask audio frames is written as mask_fill
      first_pass  the pass number of the first iter() of a view; iter() k uses first_pass + k

    The magnitudes are the caller's choice: which of these help on PATS has not been measured."""
    NPARAM = 8      # mirror, s, g, gain, f0, fw, t0, tw

    def __init__(self, seed=0, p_mirror=0., speed=0., scale=0., gain=0., freq_mask=0, time_mask=0,
                 mask_fill=0., first_pass=0):
        def real(name, v):
            v = float(v)
            if v != v or v in (float('inf'), float('-inf')):
                raise ValueError(f'Augment: {name} must be finite, got {v}')
            return v
        self.seed, self.first_pass = int(seed), int(first_pass)
        self.p_mirror, self.speed, self.scale = real('p_mirror', p_mirror), real('speed', speed), real('scale', scale)
        self.gain, self.mask_fill = real('gain', gain), real('mask_fill', mask_fill)
        self.freq_mask, self.time_mask = int(freq_mask), int(time_mask)
        if not 0 <= self.seed < 2 ** 64:
            raise ValueError(f'Augment: seed {seed} outside [0, 2^64)')
        if not 0 <= self.first_pass < 2 ** 32:
            raise ValueError(f'Augment: first_pass {first_pass} outside [0, 2^32)')
        if not 0. <= self.p_mirror <= 1.:
            raise ValueError(f'Augment: p_mirror {p_mirror} outside [0, 1]')
        if not 0. <= self.speed <= 0.5:
            raise ValueError(f'Augment: speed {speed} outside [0, 0.5]')
        if not 0. <= self.scale < 1.:
            raise ValueError(f'Augment: scale {scale} outside [0, 1)')
        if self.gain < 0.:
            raise ValueError(f'Augment: gain {gain} is negative')
        if self.freq_mask != freq_mask or self.time_mask != time_mask or self.freq_mask < 0 or self.time_mask < 0:
            raise ValueError(f'Augment: freq_mask {freq_mask} and time_mask {time_mask} must be integers >= 0')

    def check_geometry(self, channels, frames):
        if self.freq_mask > channels or self.time_mask > frames:
            raise ValueError(f'Augment: freq_mask {self.freq_mask} / time_mask {self.time_mask} exceed the audio '
                             f"window's {channels} channels / {frames} frames")

    def draw(self, order_dev, b0, n, pass_dev, channels, frames, out=None):
        """One launch: the float32 [n, 8] parameter table (columns mirror, s, g, gain, f0, fw, t0,
        tw) of the clips order_dev[b0 : b0+n] for the pass number in pass_dev (device int64 [1]);
        channels, frames: the audio window's C and T, which bound the masks."""
        from . import functional as F
        from ._native import check, lib
        self.check_geometry(channels, frames)
        if out is None:
            out = torch.empty(n, self.NPARAM, device=order_dev.device)
        F._check_dev(out)
        if tuple(out.shape) != (n, self.NPARAM) or not out.is_contiguous():
            raise ValueError(f'params must be a contiguous [{n}, {self.NPARAM}] tensor')
        assert b0 >= 0 and order_dev.dtype == torch.int64 and order_dev.is_cuda and b0 + n <= order_dev.numel()
        assert pass_dev.dtype == torch.int64 and pass_dev.is_cuda and pass_dev.numel() == 1
        check(lib.a2m_augment_params_f32(F._p(order_dev), b0, n, F._p(pass_dev), self.seed, self.p_mirror,
                                         self.speed, self.scale, self.gain, self.freq_mask, channels,
                                         self.time_mask, frames, F._p(out), F._stream()))
        return out


class PatsLoader:
    """arrays: {interval_id: {modality: float32 [L, C] ndarray or tensor}} or the path of a
    save_arrays file.  The other arguments are Data_Loader's; rank / world shard every global
    batch for data-parallel training.

    Every pass draws one permutation on the host (PatsIndex.order) and uploads it; nothing else
    crosses the bus during the pass.  All ranks must draw the same permutation: seed them alike
    (torch.manual_seed, or generators in the same state) before every pass."""

    def __init__(self, arrays, table, speaker, modalities=('pose/data', 'audio/log_mel_512'),
                 fs_new=(15, 15), time=4.3, split=None, batch_size=100, shuffle=True, window_hop=0,
                 load_data=True, missing=(), device='cuda', rank=0, world=1, generator=None,
                 **unsupported):
        assert 1 <= len(modalities) <= MAX_MOD and 0 <= rank < world and batch_size > 0
        if isinstance(arrays, (str, os.PathLike)):
            arrays = self.load_arrays(arrays)
        self.device = torch.device(device)
        self.batch_size, self.shuffle, self.generator = batch_size, shuffle, generator
        self.rank, self.world = rank, world
        lengths = {str(iid): {mod: a.shape[0] for mod, a in mods.items()} for iid, mods in arrays.items()}
        self.index = PatsIndex(lengths, table, speaker, modalities, fs_new, time, split, window_hop,
                               load_data, missing, **unsupported)
        self.modalities = self.index.modalities
        self.speaker_dict = self.index.speaker_dict
        arrays = {str(iid): mods for iid, mods in arrays.items()}
        needed = list(dict.fromkeys(iid for s in SPLITS for iid in self.index.intervals[s]))
        self.arena, self._row0, self.channels = {}, {}, {}
        for mod in self.modalities:
            parts = [np.ascontiguousarray(torch.as_tensor(arrays[iid][mod]).cpu().numpy(), dtype=np.float32)
                     for iid in needed]
            C = parts[0].shape[1] if parts else 4
            if any(p.ndim != 2 or p.shape[1] != C for p in parts) or C % 4:
                raise ValueError(f'{mod}: arrays must be [L, C] with one C, a multiple of 4')
            ends = np.cumsum([p.shape[0] for p in parts], dtype=np.int64)
            self._row0[mod] = dict(zip(needed, (ends - [p.shape[0] for p in parts]).tolist()))
            host = np.concatenate(parts) if parts else np.zeros((0, C), np.float32)
            self.arena[mod] = torch.from_numpy(host).to(self.device)
            self.channels[mod] = C
        self._buffers, self._style_buffers = {}, {}
        self._param_buffers, self._perm = {}, None
        self._velocity, self._velocity_bad = {}, {}
        self._upload_tables()
        for s in SPLITS:
            setattr(self, s, _DictView(self, s))

    # ------------------------------------------------------------------ arrays on disk
    @staticmethod
    def save_arrays(path, arrays):
        """One .npz with the keys '<interval_id>::<modality>'."""
        np.savez(path, **{f'{iid}::{mod}': np.asarray(torch.as_tensor(a).cpu().numpy(), np.float32)
                          for iid, mods in arrays.items() for mod, a in mods.items()})

    @staticmethod
    def load_arrays(path):
        out = {}
        with np.load(path) as z:
            for key in z.files:
                iid, mod = key.split('::', 1)
                out.setdefault(iid, {})[mod] = z[key]
        return out

    # ------------------------------------------------------------------ tables
    def _upload_tables(self):
        """The start tables over the samples of train, dev and test in that order (a sample's
        table position is its split's base + its global index), uploaded once."""
        ix = self.index
        self.base, base = {}, 0
        for s in SPLITS:
            self.base[s] = base
            base += ix.size(s)
        self.start, self.last, style = {}, {}, []
        for mod in self.modalities:
            rows = [self._row0[mod][iid] + w[mod][0][:n]
                    for s in SPLITS for iid, w, n in zip(ix.intervals[s], ix.windows[s], ix.sizes[s])]
            host = np.concatenate(rows).astype(np.int64) if rows else np.zeros(0, np.int64)
            self.start[mod] = torch.from_numpy(host).to(self.device)
            # beside start: the arena row of the last row of each sample's interval, where the
            # augmenting gather clamps a stretched read
            ends = [np.full(n, self._row0[mod][iid] + int(ix.lengths[iid][mod]) - 1, np.int64)
                    for s in SPLITS for iid, n in zip(ix.intervals[s], ix.sizes[s])]
            self.last[mod] = torch.from_numpy(np.concatenate(ends) if ends else np.zeros(0, np.int64)).to(self.device)
        for s in SPLITS:
            style += [np.full(n, ix.style[iid], np.float32) for iid, n in zip(ix.intervals[s], ix.sizes[s])]
        self._style = torch.from_numpy(np.concatenate(style) if style else np.zeros(0, np.float32)).to(self.device)
        # the same ids as integers, for pairs(with_style=True); _style stays what .train / .dev / .test yield
        self._style_i32 = torch.from_numpy(np.concatenate(style).astype(np.int32) if style
                                           else np.zeros(0, np.int32)).to(self.device)
        self._meta = {}
        self._velocity.clear()
        self._velocity_bad.clear()
        self.dropped = {s: dp_plan(ix.size(s), self.batch_size, self.rank, self.world)[1] for s in SPLITS}
        self._buffers.clear()

    def update_dataloaders(self, time, window_hop):
        """Re-derives the windows (Data_Loader.update_dataloaders); the arenas stay."""
        self.index.update_dataloaders(time, window_hop)
        self._upload_tables()

    def plan(self, split):
        return dp_plan(self.index.size(split), self.batch_size, self.rank, self.world)[0]

    def meta(self, split, idx):
        """The reference's collated meta of the samples idx (host arithmetic on the tables)."""
        if split not in self._meta:
            ix = self.index
            ids = [iid for iid, n in zip(ix.intervals[split], ix.sizes[split]) for _ in range(n)]
            local = [k for n in ix.sizes[split] for k in range(n)]
            self._meta[split] = (ids, ix.meta_times(split), np.asarray(local, np.int64))
        ids, times, local = self._meta[split]
        return {'interval_id': [ids[i] for i in idx], 'start': torch.from_numpy(times[idx, 0]),
                'end': torch.from_numpy(times[idx, 1]), 'idx': torch.from_numpy(local[idx])}

    # ------------------------------------------------------------------ train samplers
    def clip_velocity(self, split):
        """The mean joint speed (pixels per frame, a2m.functional.clip_velocity) of every clip of
        the split in global-index order: float32 [N] on the device, read from the pose arena in
        place at the loader's geometry, computed once per split and kept until update_dataloaders."""
        if split not in self._velocity:
            from . import functional as F
            pose = next(m for m in self.modalities if m.startswith('pose'))
            window, interval, _ = self.index.geometry(pose)
            self._velocity[split], self._velocity_bad[split] = F.clip_velocity(
                self.arena[pose], self.start[pose], self.base[split], self.index.size(split), window, interval)
        return self._velocity[split]

    def train_sampler(self, split='train', *, style_iters=0, num_training_sample=None, quantile_sample=None,
                      quantile_num_training_sample=None, weighted=0, num_training_iters=None,
                      sample_all_styles=0, velocity=None, generator=None):
        """The reference's train sampler for its arguments style_iters, num_training_sample,
        quantile_sample, quantile_num_training_sample, weighted and num_training_iters, in its
        precedence (a2m.sampling.make_sampler, which documents each): a TrainSampler for
        pairs(..., sampler=) and sampled(), or None where nothing is set.  velocity=: a host array
        [N] to bin by instead of clip_velocity(split); generator=: feeds every draw (default: the
        loader's, else torch's global one).  Construction may synchronise; a pass does not."""
        from .sampling import make_sampler
        return make_sampler(self, split, style_iters=style_iters, num_training_sample=num_training_sample,
                            quantile_sample=quantile_sample,
                            quantile_num_training_sample=quantile_num_training_sample, weighted=weighted,
                            num_training_iters=num_training_iters, sample_all_styles=sample_all_styles,
                            velocity=velocity, generator=generator)

    def sampled(self, split, sampler):
        """The batch-dict view of .train / .dev / .test over the sampler's order: every iter() is a
        new draw."""
        self._check_sampler(split, sampler)
        return _DictView(self, split, sampler=sampler)

    def _check_sampler(self, split, sampler):
        # the gather checks no index: a sampler built for another split or other windows is refused here
        if sampler.split != split or sampler.n != self.index.size(split):
            raise ValueError(f'sampler: built for the {sampler.n} clips of {sampler.split}, not the '
                             f'{self.index.size(split)} of {split}')

    # ------------------------------------------------------------------ one pass
    def draw(self, split, order=None):
        """The pass's order on the host (int64 [N], global indices of the split): drawn as the
        reference's loader would, or the caller's, range-checked here because the kernel checks
        nothing."""
        n = self.index.size(split)
        if order is None:
            return self.index.order(split, self.shuffle, self.generator)
        order = np.ascontiguousarray(torch.as_tensor(order).cpu().numpy(), dtype=np.int64).reshape(-1)
        if order.size and (order.min() < 0 or order.max() >= n):
            raise ValueError(f'order holds an index outside [0, {n}) of {split}')
        return order

    def upload(self, split, order):
        """The order as positions of the start tables, on the device: the pass's one upload."""
        return torch.from_numpy(order + self.base[split]).to(self.device)

    def gather(self, order_dev, b0, n, specs, outs=None):
        """One launch: clips order_dev[b0 : b0+n] of every (modality, mode, mean, std) of specs
        -> [n, T, C] tensors (outs, or new ones).  order_dev holds start-table positions
        (upload()); the caller guarantees them in range."""
        from . import functional as F
        from ._native import check, lib
        mods = [s[0] for s in specs]
        geo = [self.index.geometry(m) for m in mods]
        if outs is None:
            outs = [torch.empty(n, g[2], self.channels[m], device=self.device) for m, g in zip(mods, geo)]
        means, stds = [s[2] for s in specs], [s[3] for s in specs]
        F._check_dev(*outs, *means, *stds)
        for m, g, out, mean, std in zip(mods, geo, outs, means, stds):
            if tuple(out.shape) != (n, g[2], self.channels[m]) or not out.is_contiguous():
                raise ValueError(f'{m}: out must be a contiguous [{n}, {g[2]}, {self.channels[m]}] tensor')
            if any(t is not None and (t.numel() != self.channels[m] or not t.is_contiguous()) for t in (mean, std)):
                raise ValueError(f'{m}: mean and std must be contiguous [{self.channels[m]}] tensors')
        assert b0 >= 0 and order_dev.dtype == torch.int64 and order_dev.is_cuda and b0 + n <= order_dev.numel()
        check(lib.a2m_batch_gather_f32(
            len(specs), _ptrs([self.arena[m] for m in mods]), _ptrs([self.start[m] for m in mods]),
            _i32s([self.channels[m] for m in mods]), _i32s([g[0] for g in geo]), _i32s([g[1] for g in geo]),
            _i32s([s[1] for s in specs]), _ptrs(means), _ptrs(stds), _ptrs(outs), F._p(order_dev), b0, n,
            F._stream()))
        return outs

    def gather_augmented(self, order_dev, b0, n, specs, params, outs=None, mask_fill=0.):
        """gather() with row b of params (float32 [n, 8], Augment.draw's or the caller's: mirror, s,
        g, gain, f0, fw, t0, tw) applied to clip b, one launch.  A pose modality in the neck-sub
        mode is mirrored and scaled, an audio modality takes the gain and the masks, every
        modality the tempo.  A caller's table keeps s >= 0 and the masks inside the window."""
        from . import functional as F
        from ._native import check, lib
        from .skeleton import mirror_permutation
        mods = [s[0] for s in specs]
        geo = [self.index.geometry(m) for m in mods]
        if outs is None:
            outs = [torch.empty(n, g[2], self.channels[m], device=self.device) for m, g in zip(mods, geo)]
        means, stds = [s[2] for s in specs], [s[3] for s in specs]
        F._check_dev(*outs, *means, *stds, params)
        for m, g, out, mean, std in zip(mods, geo, outs, means, stds):
            if tuple(out.shape) != (n, g[2], self.channels[m]) or not out.is_contiguous():
                raise ValueError(f'{m}: out must be a contiguous [{n}, {g[2]}, {self.channels[m]}] tensor')
            if any(t is not None and (t.numel() != self.channels[m] or not t.is_contiguous()) for t in (mean, std)):
                raise ValueError(f'{m}: mean and std must be contiguous [{self.channels[m]}] tensors')
        if tuple(params.shape) != (n, Augment.NPARAM) or not params.is_contiguous():
            raise ValueError(f'params must be a contiguous [{n}, {Augment.NPARAM}] tensor')
        assert b0 >= 0 and order_dev.dtype == torch.int64 and order_dev.is_cuda and b0 + n <= order_dev.numel()
        roles = [ROLE_POSE if m.startswith('pose') and s[1] == MODE_NECKSUB else
                 ROLE_AUDIO if m.startswith('audio') else ROLE_NONE for m, s in zip(mods, specs)]
        if self._perm is None:
            self._perm = torch.tensor(mirror_permutation(), dtype=torch.int32).to(self.device)
        check(lib.a2m_batch_gather_aug_f32(
            len(specs), _ptrs([self.arena[m] for m in mods]), _ptrs([self.start[m] for m in mods]),
            _ptrs([self.last[m] for m in mods]), _i32s([self.channels[m] for m in mods]),
            _i32s([g[0] for g in geo]), _i32s([g[1] for g in geo]), _i32s([s[1] for s in specs]), _i32s(roles),
            _ptrs(means), _ptrs(stds), _ptrs(outs), F._p(order_dev), b0, n, F._p(params), F._p(self._perm),
            float(mask_fill), F._stream()))
        return outs

    def _stat(self, t):
        return None if t is None else torch.as_tensor(t).to(self.device, torch.float32).contiguous()

    def pairs(self, split, pose_mean=None, pose_std=None, audio_mean=None, audio_std=None, copy=False,
              order=None, with_style=False, augment=None, sampler=None):
        """A re-iterable of (audio [n, T, 128], real_pose [n, T, 104]) for GANTrainer.fit /
        validate, one launch a batch.  With pose statistics the poses are neck-subtracted and
        normalised as necksub_normalize, with audio statistics the audio is standardised as
        gather_windows; without, raw.  The output buffers are reused per batch size: a yielded
        batch is valid until the next one is asked for (the trainer consumes a batch before the
        next is formed, on one stream); copy=True yields fresh tensors for callers that keep
        batches.  order: the caller's order of the split's global indices instead of a drawn one.
        with_style=True yields (audio, real_pose, style), style the int32 [n] speaker ids of the
        batch's clips, looked up on the device (one more launch a batch, no synchronisation).
        augment: an Augment; each batch is then the parameter draw plus the augmenting gather (two
        launches, no synchronisation), iter() number k of the view draws for pass
        augment.first_pass + k, and the view's last_params is the device table of the batch just
        yielded.  Mirroring and scaling act on the neck-subtracted pose and need pose statistics
        (left-right symmetric ones, for a mirrored pose to be normalised like its original).
        sampler: a train_sampler(); every iter() then takes a new draw of it as the pass's order
        (not together with order=), and len() follows its length."""
        if sampler is not None:
            if order is not None:
                raise ValueError('sampler and order both name the pass\'s order: give one')
            self._check_sampler(split, sampler)
        if (pose_mean is None) != (pose_std is None) or (audio_mean is None) != (audio_std is None):
            raise ValueError('mean and std come together')
        if augment is not None:
            if not isinstance(augment, Augment):
                raise TypeError('augment must be an a2m.data.Augment')
            if pose_mean is None and (augment.p_mirror > 0 or augment.scale > 0):
                raise ValueError('augment: p_mirror and scale act on the neck-subtracted pose and need '
                                 'pose_mean / pose_std')
        if order is not None:
            order = self.draw(split, order)     # refused here, on the host, before any launch
        pose =next(m for m in self.modalities if m.startswith('pose'))
        audio = next(m for m in self.modalities if m.startswith('audio'))
        specs = [(audio, MODE_RAW if audio_mean is None else MODE_STANDARDISE, self._stat(audio_mean),
                  self._stat(audio_std)),
                 (pose, MODE_RAW if pose_mean is None else MODE_NECKSUB, self._stat(pose_mean),
                  self._stat(pose_std))]
        if augment is not None:
            augment.check_geometry(self.channels[audio], self.index.geometry(audio)[2])
        return _Pairs(self, split, specs, copy, order, with_style, augment, sampler)


class _View:
    def __init__(self, loader, split, order=None, sampler=None):
        self.loader, self.split, self.order, self.sampler = loader, split, order, sampler

    def __len__(self):
        fixed = self.sampler if self.sampler is not None else self.order
        if fixed is not None:
            return len(dp_plan(len(fixed), self.loader.batch_size, self.loader.rank, self.loader.world)[0])
        return len(self.loader.plan(self.split))

    def _draw(self):
        if self.sampler is None:
            return self.loader.draw(self.split, self.order)
        self.loader._check_sampler(self.split, self.sampler)
        return self.sampler.draw()

    def __iter__(self):
        # the draw and the upload happen here, not at the first next(): the loop that follows
        # crosses the bus no more
        ld = self.loader
        host = self._draw()
        plan = dp_plan(len(host), ld.batch_size, ld.rank, ld.world)[0]
        return self._run(host, ld.upload(self.split, host) if len(host) else None, plan)


class _Pairs(_View):
    def __init__(self, loader, split, specs, copy, order, with_style=False, augment=None, sampler=None):
        super().__init__(loader, split, order, sampler)
        self.specs, self.copy, self.with_style = specs, copy, with_style
        self.augment, self.passes, self.pass_dev, self.last_params = augment, 0, None, None

    def __iter__(self):
        if self.augment is None:
            return super().__iter__()
        # the pass number goes up next to the order, in a scalar of this pass's own: an iterator
        # of an earlier pass that is still being consumed keeps its number
        ld = self.loader
        host = self._draw()
        plan = dp_plan(len(host), ld.batch_size, ld.rank, ld.world)[0]
        self.pass_dev = torch.tensor([self.augment.first_pass + self.passes], dtype=torch.int64).to(ld.device)
        self.passes += 1
        return self._run(host, ld.upload(self.split, host) if len(host) else None, plan, self.pass_dev)

    def _gather_augmented(self, order_dev, b0, n, outs, pass_dev):
        ld, aug = self.loader, self.augment
        audio = self.specs[0][0]
        params = None if self.copy else ld._param_buffers.get(n)
        params = aug.draw(order_dev, b0, n, pass_dev, ld.channels[audio], ld.index.geometry(audio)[2], params)
        if not self.copy:
            ld._param_buffers[n] = params
        self.last_params = params
        return ld.gather_augmented(order_dev, b0, n, self.specs, params, outs, aug.mask_fill)

    def _run(self, host, order_dev, plan, pass_dev=None):
        ld = self.loader
        for b0, n in plan:
            outs = None if self.copy else ld._buffers.get(n)
            if pass_dev is None:
                outs = ld.gather(order_dev, b0, n, self.specs, outs)
            else:
                outs = self._gather_augmented(order_dev, b0, n, outs, pass_dev)
            if not self.copy:
                ld._buffers[n] = outs
            if not self.with_style:
                yield tuple(outs)
                continue
            style = None if self.copy else ld._style_buffers.get(n)
            if style is None:
                style = torch.empty(n, dtype=torch.int32, device=ld.device)
                if not self.copy:
                    ld._style_buffers[n] = style
            torch.index_select(ld._style_i32, 0, order_dev[b0:b0 + n], out=style)
            yield (*outs, style)


class _DictView(_View):
    """.train / .dev / .test: the reference's batch dict, the modalities raw."""

    def _run(self, host, order_dev, plan):
        ld = self.loader
        specs = [(m, MODE_RAW, None, None) for m in ld.modalities]
        T = ld.index.geometry(ld.modalities[0])[2]
        for b0, n in plan:
            batch = dict(zip(ld.modalities, ld.gather(order_dev, b0, n, specs)))
            pos = order_dev[b0:b0 + n]
            batch['idx'] = pos - ld.base[self.split]
            batch['style'] = ld._style[pos].unsqueeze(1).expand(n, T).contiguous()
            batch['meta'] = ld.meta(self.split, host[b0:b0 + n])
            yield batch
