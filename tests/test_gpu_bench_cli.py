"""bench.py's command line: a plain run times its steps and prints the headline line only (no
entry that `--full` measures with runs of its own); `--dump-outputs` writes what the last timed
step returned.

One small plain run (B = 2 clips x 64 frames, 3 timed steps) in a child process, shared by the
tests; the dumped poses are compared with the same step built and run eagerly in this process
(same seeds, same kernels; a replayed graph and an eager step may differ by fp32 rounding in the
split-K reductions only, far inside north_star's 1e-4).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
B, T, STEPS, WARMUP = 2, 64, 3, 1
HEADLINE = {'metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup'}
FULL_ONLY = {'roofline', 'mel_roofline', 'mel_encoder_roofline', 'cpu_baseline'}


@pytest.fixture(scope='module')
def plain_run(tmp_path_factory):
    out = tmp_path_factory.mktemp('bench_dump')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(STEPS),
                        '--warmup', str(WARMUP), '--batch', str(B), '--frames', str(T),
                        '--dump-outputs', str(out)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, cwd=str(out))
    assert r.returncode == 0, r.stderr.decode(errors='replace')[-2000:]
    lines = [x for x in r.stdout.decode().splitlines() if x.startswith('{')]
    assert len(lines) == 1
    return json.loads(lines[0]), out


def test_plain_run_prints_the_headline_only(plain_run):
    line, _ = plain_run
    assert HEADLINE <= set(line)
    assert not FULL_ONLY & set(line)
    assert line['steps'] == STEPS and line['warmup'] == WARMUP
    assert line['unit'] == 'pose-frames/s' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['ms_per_step'] > 0
    # value is the throughput of that step time (both are rounded in the line)
    assert line['value'] == pytest.approx(B * T / (line['ms_per_step'] * 1e-3), rel=1e-3)


def test_dump_outputs_is_the_timed_steps_result(plain_run):
    import bench
    _, out = plain_run
    assert sorted(os.listdir(out)) == ['pose.npy']
    pose = np.load(os.path.join(out, 'pose.npy'), allow_pickle=False)
    assert pose.dtype == np.float32 and pose.shape == (B, T, 104)
    assert pose.nbytes <= bench.DUMP_MAX_BYTES
    dev = torch.device('cuda', 0)
    g, wave = bench.build_infer(B, T, 0, dev)
    with torch.no_grad():
        ref = bench.infer_step(g, wave)().cpu().numpy()
    assert np.isfinite(pose).all() and np.abs(ref).max() > 0
    assert rel_err(pose, ref) < TOL

