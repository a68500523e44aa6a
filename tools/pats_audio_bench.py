"""PATS audio front-end timings (PATS audio features): every call is captured
20x into a HIP graph, the graphs are replayed 5x per sample in turn, and the median / min / max of
15 interleaved samples is printed as one JSON line of microseconds per call.

  log_mel_batch             the VGGish front end at the same 64 x 135 frames
  log_mel_512[_sr44100]     64 clips x 4.3 s
  log_mel_400               the same waves
  windows_fused             64 windows of 382 / 6 over one long clip (log_mel_512_windows)
  windows_full_then_gather  log_mel_512 of the whole clip + a2m_window_gather_f32

usage: pats_audio_bench.py new|old   (old: only log_mel_batch, for a library selected with A2M_LIB
that predates a2m.pats_audio)"""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                'audio-to-motion-generation_amd'))
which = sys.argv[1]
DEV = 'cuda'
INNER = 20      # launches per graph
ROUNDS = 15


def graphed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(INNER):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_all(graphs):
    res = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                g.replay()
            b.record()
            torch.cuda.synchronize()
            res[k].append(a.elapsed_time(b) * 1e3 / (5 * INNER))   # us per call
    return {k: (statistics.median(v), min(v), max(v)) for k, v in res.items()}


rng = np.random.default_rng(0)
B = 64
S512 = int(4.3 * 16000)                      # 68800 -> 135 frames
NF = 1 + S512 // 512
SB = 2048 + (NF - 1) * 1067                  # log_mel_batch: the same 135 frames per clip
w512 = torch.from_numpy(rng.standard_normal((B, S512)).astype(np.float32) * 0.1).to(DEV)
wb = torch.from_numpy(rng.standard_normal((B, SB)).astype(np.float32) * 0.1).to(DEV)

from a2m.mel_features import log_mel_batch
graphs = {}
ob = log_mel_batch(wb)
assert ob.shape == (B, NF, 128), ob.shape
graphs['log_mel_batch'] = graphed(lambda: log_mel_batch(wb, out=ob))
out = {'which': which, 'frames': B * NF}
if which == 'new':
    from a2m.pats_audio import log_mel_512, log_mel_512_windows, log_mel_400
    from a2m.windowing import gather_windows
    o512 = log_mel_512(w512, 16000)
    assert o512.shape == (B, NF, 128)
    graphs['log_mel_512'] = graphed(lambda: log_mel_512(w512, 16000, out=o512))
    w441 = w512
    o441 = log_mel_512(w441, 44100)
    graphs['log_mel_512_sr44100'] = graphed(lambda: log_mel_512(w441, 44100, out=o441))
    o400 = log_mel_400(w512)
    out['frames_400'] = o400.shape[0] * o400.shape[1]
    graphs['log_mel_400'] = graphed(lambda: log_mel_400(w512, out=o400))
    # 64 windows of 382 / 6 on one long clip
    nwin = 64
    long = torch.from_numpy(rng.standard_normal(512 * 382 * nwin).astype(np.float32) * 0.1).to(DEV)
    starts = torch.arange(nwin, device=DEV) * 382
    full = log_mel_512(long, 16000)
    out['frames_long'] = full.shape[0]
    ow = log_mel_512_windows(long, 16000, starts)
    og = torch.empty_like(ow)
    assert torch.equal(ow, gather_windows(full, starts.cpu().numpy(), 382, 6))
    graphs['windows_fused'] = graphed(lambda: log_mel_512_windows(long, 16000, starts, out=ow))

    def full_then_gather():
        from a2m import functional as F
        from a2m._native import check, lib
        log_mel_512(long, 16000, out=full)
        check(lib.a2m_window_gather_f32(F._p(full), full.shape[0], 128, F._p(starts), nwin, 382, 6,
                                        None, None, F._p(og), F._stream()))
    graphs['windows_full_then_gather'] = graphed(full_then_gather)
    graphs['log_mel_512_long_only'] = graphed(lambda: log_mel_512(long, 16000, out=full))
out['us_median_min_max'] = time_all(graphs)
print(json.dumps(out))
