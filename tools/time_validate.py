"""Time GANTrainer.validate against the reference-shaped composition of the public ops.

Default: B = 64, T = 64, 8 dev batches, fp32, one process.  The two passes alternate in one process
(the box-to-box spread is about +-6 %, so only the interleaved ratio means anything); each is run
--reps times after --warmup untimed rounds, wall clock around a device synchronise, and the medians
are reported with the launches each pass issues per batch (the loss launches are counted from the
entry points called; D forwards are counted by a forward hook).

    python tools/time_validate.py [--batch 64] [--batches 8] [--reps 7] [--warmup 2]

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, 'audio-to-motion-generation_amd')):
    if p not in sys.path:
        sys.path.insert(0, p)


def composition(G, D, batches, lambda_gan, lambda_d):
    """version5_model_train.py:438-492 from the public ops, with the reference's `.item()` per term:
    per batch 2 D forwards (its third repeats the first), 2 diff_time, motion_losses (2 launches) and
    3 mse_loss (2 launches each)."""
    from a2m import functional as F
    G.eval()
    D.eval()
    tot = [0.0] * 6
    with torch.no_grad():
        for audio, real_pose in batches:
            fake_pose, internal = G(audio, real_pose=real_pose)
            tot[2] += internal[0].item()
            tot[3] += internal[1].item()
            fake_d, _ = D(F.diff_time(fake_pose))
            real_d, _ = D(F.diff_time(real_pose))
            terms, _ = F.motion_losses(fake_pose, real_pose)
            tot[4] += terms[1].item()
            tot[5] += terms[2].item()
            ones, zeros = torch.ones_like(fake_d), torch.zeros_like(fake_d)
            tot[0] += (terms[0] + lambda_gan * F.mse_loss(fake_d, ones)[0]).item()
            tot[1] += (F.mse_loss(real_d, ones)[0] + lambda_d * F.mse_loss(fake_d, zeros)[0]).item()
    G.train()
    D.train()
    return [v / len(batches) for v in tot]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    from a2m.real_motion_model import SelfAttention_D, SelfAttention_G
    from a2m.training import GANTrainer
    dev = torch.device('cuda', 0)
    torch.manual_seed(0)
    g = SelfAttention_G(time_steps=64, p=0.2).to(dev).train()
    d = SelfAttention_D(out_channels=64).to(dev).train()
    tr = GANTrainer(g, d, lr=1e-4, label_seed=7)
    gen = torch.Generator().manual_seed(1)
    batches = [((torch.randn(args.batch, 64, 128, generator=gen) * 2.0 - 3.0).to(dev),
                torch.randn(args.batch, 64, 104, generator=gen).to(dev)) for _ in range(args.batches)]
    d_calls = [0]
    hook = d.register_forward_hook(lambda *_: d_calls.__setitem__(0, d_calls[0] + 1))

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out

    passes = {'validate': lambda: tr.validate(batches),
              'composition': lambda: composition(g, d, batches, tr.lambda_gan, tr.lambda_d)}
    times = {k: [] for k in passes}
    d_forwards, last = {}, {}
    for rep in range(args.warmup + args.reps):
        for name, fn in passes.items():
            d_calls[0] = 0
            ms, last[name] = timed(fn)
            d_forwards[name] = d_calls[0] / args.batches
            if rep >= args.warmup:
                times[name].append(ms)
    hook.remove()
    med = {k: statistics.median(v) for k, v in times.items()}
    v = last['validate']
    agree = max(abs(a - b) / abs(b) for a, b in zip([v['g_loss'], v['d_loss'], v['bone_loss'], v['angle_loss'],
                                                     v['smoothness_loss'], v['jerk_loss']], last['composition']))
    print(json.dumps({
        'batch': args.batch, 'batches': args.batches, 'reps': args.reps,
        'validate_ms': round(med['validate'], 3), 'composition_ms': round(med['composition'], 3),
        'ratio': round(med['validate'] / med['composition'], 4),
        'validate_ms_all': [round(t, 3) for t in times['validate']],
        'composition_ms_all': [round(t, 3) for t in times['composition']],
        'per_batch': {'validate': {'d_forwards': d_forwards['validate'], 'loss_launches': 2, 'host_reads': 0},
                      'composition': {'d_forwards': d_forwards['composition'], 'loss_launches': 10,
                                      'host_reads': 6}},
        'max_rel_difference': agree}))


if __name__ == '__main__':
    main()
