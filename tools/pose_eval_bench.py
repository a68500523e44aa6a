"""Evaluation pass timings: over a synthetic test split of 8 speakers (40 recordings
of 60 s, window_hop 5) in batches of 64 clips,

  evaluate        host-clock microseconds per batch of a2m.evaluation.evaluate(): the loader's gather and
                  style lookup, the generator forward, the three metric launches, and at the end the one
                  host read and the host formulas of result() (two 104 x 104 eigh per speaker)
  parent_pck      the best the library offered before for "how good is this checkpoint": per batch
                  generator -> denormalize -> compute_pck on [n T, 2, 52] with its result read back to the
                  host (one synchronisation a batch), PCK only, no per-speaker split
  metric_launches device microseconds (events around a HIP graph of 20 updates) of eval_clip + eval_gram +
                  eval_finish on one batch; eval_clip, eval_gram, eval_finish: each alone, the same way
  forward         device microseconds of the generator forward on the same batch
  evaluate_sync   evaluate(sync=True): the same pass with the two launches of the synchrony metrics a batch
                  and AudioSyncEvaluator.result() at the end, by the host clock, against evaluate in the same run
  sync_launches   device microseconds of eval_sync + eval_sync_finish on one batch, graphed as metric_launches

Every path is warmed with one pass; the paths are then sampled in turn ROUNDS times and the median /
min / max printed as one JSON line."""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'audio-to-motion-generation_amd'))
sys.path.insert(0, REPO)
from a2m import functional as F  # noqa: E402
from a2m.data import PatsLoader  # noqa: E402
from a2m.evaluation import AudioSyncEvaluator, PoseEvaluator, compute_pck, evaluate  # noqa: E402
from a2m.normalization import denormalize  # noqa: E402
from a2m.real_motion_model import SelfAttention_G  # noqa: E402
from oracle import weights  # noqa: E402

DEV = 'cuda'
B, INNER, ROUNDS, SPEAKERS = 64, 20, 15, 8
POSE, AUDIO = 'pose/data', 'audio/log_mel_512'

rng = np.random.default_rng(0)
ids = [str(100000 + k) for k in range(40)]
arrays = {i: {POSE: (rng.standard_normal((900, 104)) * 40 + 300).astype(np.float32),
              AUDIO: (rng.standard_normal((5340, 128)) * 2 - 4).astype(np.float32)} for i in ids}
names = [f'speaker{k}' for k in range(SPEAKERS)]
table = [{'dataset': 'test', 'interval_id': i, 'speaker': names[k % SPEAKERS]} for k, i in enumerate(ids)]
loader = PatsLoader(arrays, table, names, batch_size=B, window_hop=5, shuffle=False, device=DEV)
N = loader.index.size('test')
n_batches = len(loader.plan('test'))
pm = torch.from_numpy((rng.standard_normal(104) * 30).astype(np.float32)).to(DEV)
ps = torch.from_numpy((rng.random(104) * 50 + 5).astype(np.float32)).to(DEV)
am = torch.from_numpy((rng.standard_normal(128) - 4).astype(np.float32)).to(DEV)
asd = torch.from_numpy((rng.random(128) * 2 + 0.5).astype(np.float32)).to(DEV)
zero, one = torch.zeros_like(pm), torch.ones_like(ps)

g = SelfAttention_G(p=0.0)
g.load_state_dict(weights.make_state_dict({k: tuple(v.shape) for k, v in g.state_dict().items()}, seed=99), strict=False)
g = g.to(DEV).eval()


def evaluate_pass(sync=False):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = evaluate(g, loader, 'test', pose_mean=pm, pose_std=ps, audio_mean=am, audio_std=asd, sync=sync)
    dt = time.perf_counter() - t0
    assert res['all']['n_clips'] == N and ('n_audio_beats' in res['all']) == sync
    return dt * 1e6 / n_batches


def parent_pass():
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    scores = []
    with torch.no_grad():
        for audio, real in loader.pairs('test', zero, one, am, asd):
            fake_px = denormalize(g(audio)[0], pm, ps)
            pck = compute_pck(fake_px.view(-1, 2, 52), real.view(-1, 2, 52))
            scores.append(pck.cpu().numpy())
    mean = float(np.concatenate(scores).mean())
    dt = time.perf_counter() - t0
    assert 0.0 <= mean <= 1.0
    return dt * 1e6 / n_batches


audio0, real0, style0 = [t.clone() for t in next(iter(loader.pairs('test', zero, one, am, asd, with_style=True)))]
ev = PoseEvaluator(pm, ps, SPEAKERS, device=DEV)
with torch.no_grad():
    fake0 = g(audio0)[0].clone()


def _events(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def _graphed(fn):
    """INNER calls of fn captured to one HIP graph: device time once the host is out of the way."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(INNER):
            fn()
    return lambda: _events(graph.replay, 5) / INNER


ev.update(fake0, real0, style0)
st = ev.state()
fake_px0, part0, hits0 = ev._buffers[(B, 64)]
metric_sample = _graphed(lambda: ev.update(fake0, real0, style0))
clip_sample = _graphed(lambda: F.eval_clip(fake0, real0, style0, ev.mean, ev.std, SPEAKERS, ev.alpha, ev.speed_width,
                                           ev.accel_width, st['hist'], fake_px0, part0, hits0))
gram_sample = _graphed(lambda: F.eval_gram(fake_px0, real0, style0, st['sx'], st['gram']))
finish_sample = _graphed(lambda: F.eval_finish(part0, hits0, style0, 64, st['counts'], st['sums']))
sev = AudioSyncEvaluator(SPEAKERS, audio_std=asd, device=DEV)
sync_sample = _graphed(lambda: sev.update(audio0, fake_px0, real0, style0))


def forward_sample():
    with torch.no_grad():
        return _events(lambda: g(audio0), INNER)


paths = {'evaluate': evaluate_pass, 'evaluate_sync': lambda: evaluate_pass(True), 'parent_pck': parent_pass,
         'metric_launches': metric_sample, 'sync_launches': sync_sample, 'eval_clip': clip_sample,
         'eval_gram': gram_sample, 'eval_finish': finish_sample, 'forward': forward_sample}
for fn in paths.values():
    fn()
res = {k: [] for k in paths}
for _ in range(ROUNDS):
    for k, fn in paths.items():
        res[k].append(fn())
us = {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}
# launches a batch on top of the forward: the style lookup and PoseEvaluator's three kernels; sync=True adds two
print(json.dumps({'clips': N, 'batches': n_batches, 'speakers': SPEAKERS, 'launches_added_per_batch': 4,
                  'sync_launches_added_per_batch': 2,
                  'us_per_batch_median_min_max': us,
                  'metric_launches_over_forward': us['metric_launches'][0] / us['forward'][0],
                  'evaluate_sync_over_evaluate': us['evaluate_sync'][0] / us['evaluate'][0]}))
