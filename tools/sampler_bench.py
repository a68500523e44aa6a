"""Construction time of the velocity samplers on a synthetic train split of 40
recordings of 60 s at window_hop 5 (the split of tools/pose_eval_bench.py, as 'train'), batch size 64:

  above_device      host-clock milliseconds of loader.train_sampler(quantile_sample=0.9) with the
                    velocity cache dropped first: the velocity kernel, the select passes, the
                    classification, the reads of two order statistics and of the int32 class table,
                    np.flatnonzero
  rebalance_device  the same for quantile_sample=8, quantile_num_training_sample=4
  above_host, rebalance_host
                    the only way to the same sampler without the kernels: gather every clip with
                    loader.pairs('train', copy=True), move the poses to the host, compute the
                    statistic in numpy (vectorised, float32 differences, float64 mean) and hand it to
                    train_sampler(velocity=)
  velocity_kernel   device microseconds of a2m_clip_velocity_f32 over the split (events around a HIP
                    graph of 20 launches), and from it the achieved bytes per second over the
                    distinct arena bytes the clips touch, as a fraction of the 6.29 TB/s a float4 copy
                    reaches and of the 8 TB/s specification.  The pose arena is a few MB and stays in
                    the last-level cache between launches: this is the rate of a warm arena.

Every path is warmed once; the paths are then sampled in turn ROUNDS times and the median / min /
max printed as one JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'audio-to-motion-generation_amd'))
from a2m import functional as F  # noqa: E402
from a2m.data import PatsLoader  # noqa: E402

DEV = 'cuda'
B, INNER, ROUNDS = 64, 20, 15
POSE, AUDIO = 'pose/data', 'audio/log_mel_512'
HBM_MEASURED, HBM_SPEC = 6.29e12, 8.0e12

rng = np.random.default_rng(0)
ids = [str(100000 + k) for k in range(40)]
# random walks whose step size differs by recording and along it, so the velocities spread
arrays = {i: {POSE: (300 + np.cumsum(rng.standard_normal((900, 104)) * np.exp(rng.uniform(-2, 2))
                                     * (0.25 + np.abs(np.sin(np.arange(900) / 40 + rng.uniform(0, 6))))[:, None],
                                     axis=0)).astype(np.float32),
              AUDIO: (rng.standard_normal((5340, 128)) * 2 - 4).astype(np.float32)} for i in ids}
table = [{'dataset': 'train', 'interval_id': i, 'speaker': 'speaker0'} for i in ids]
loader = PatsLoader(arrays, table, 'speaker0', batch_size=B, window_hop=5, shuffle=False, device=DEV)
N = loader.index.size('train')
window, interval, T = loader.index.geometry(POSE)


def device_sampler(**kw):
    def run():
        loader._velocity.clear()
        loader._velocity_bad.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = loader.train_sampler(**kw)
        dt = time.perf_counter() - t0
        return dt * 1e3, s
    return run


def host_velocity():
    out = []
    for _, pose in loader.pairs('train', copy=True):
        x = pose.cpu().numpy()
        d = x[:, 1:] - x[:, :-1]
        out.append(np.sqrt(d[..., 1:52] ** 2 + d[..., 53:] ** 2).astype(np.float64).mean(axis=(1, 2)))
    return np.concatenate(out)


def host_sampler(**kw):
    def run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s = loader.train_sampler(velocity=host_velocity(), **kw)
        dt = time.perf_counter() - t0
        return dt * 1e3, s
    return run


ABOVE, REBALANCE = dict(quantile_sample=0.9), dict(quantile_sample=8, quantile_num_training_sample=4)
paths = {'above_device': device_sampler(**ABOVE), 'rebalance_device': device_sampler(**REBALANCE),
         'above_host': host_sampler(**ABOVE), 'rebalance_host': host_sampler(**REBALANCE)}
first = {k: fn()[1] for k, fn in paths.items()}                                     # the warm-up
# the two ways agree wherever no clip sits within float32 rounding of a threshold; report, do not assume
same = {k: bool(len(first[f'{k}_device'].classes) == len(first[f'{k}_host'].classes) and all(
    np.array_equal(a, b) for a, b in zip(first[f'{k}_device'].classes, first[f'{k}_host'].classes)))
    for k in ('above', 'rebalance')}

arena, start = loader.arena[POSE], loader.start[POSE]
F.clip_velocity(arena, start, loader.base['train'], N, window, interval)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    for _ in range(INNER):
        F.clip_velocity(arena, start, loader.base['train'], N, window, interval)


def kernel_us():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(5):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (5 * INNER)


kernel_us()
res = {k: [] for k in list(paths) + ['velocity_kernel']}
for _ in range(ROUNDS):
    for k, fn in paths.items():
        res[k].append(fn()[0])
    res['velocity_kernel'].append(kernel_us())
stat = {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}

rows = start[loader.base['train']:loader.base['train'] + N].cpu().numpy()[:, None] + np.arange(T)[None] * interval
distinct_bytes = int(np.unique(rows).size) * arena.shape[1] * 4
read_bytes = N * T * arena.shape[1] * 4
rate = distinct_bytes / (stat['velocity_kernel'][0] * 1e-6)
print(json.dumps({'clips': N, 'frames': T, 'batch_size': B, 'rounds': ROUNDS,
                  'ms_median_min_max': {k: v for k, v in stat.items() if k != 'velocity_kernel'},
                  'velocity_kernel_us_median_min_max': stat['velocity_kernel'],
                  'distinct_arena_bytes': distinct_bytes, 'clip_bytes_read': read_bytes,
                  'distinct_bytes_per_s': rate, 'fraction_of_measured_hbm_6.29TBs': rate / HBM_MEASURED,
                  'fraction_of_spec_hbm_8TBs': rate / HBM_SPEC,
                  'host_over_device': {k: stat[f'{k}_host'][0] / stat[f'{k}_device'][0] for k in ('above', 'rebalance')},
                  'device_and_host_select_the_same_clips': same,
                  'subset_sizes': {k: [len(c) for c in s.classes] for k, s in first.items()}}))
