"""The validation epoch on the device: csrc/validation.hip's two kernels against float64, and
GANTrainer.validate / fit on the real models against the composition of the public ops.

Kernel tolerances are this project's rule from tests/test_gpu_losses_fp64.py, imported, not restated:
a term passes within 8 x e32()[k] x |value| (e32: the largest relative error torch-CPU float32 makes
on that loss over that module's cases), a composite (g_loss, d_loss) within the lambda-weighted sum of
its parts' bounds, and bone / angle, passed-in float32 scalars, arrive exactly.  References are
tests/loss_ref.py (float64 numpy).  That module's self-check is kept: every reference recomputed with
one element left out must move by more than 4 x the tolerance (a bound that could hide a dropped row
fails on the CPU side, inside check_scalar).  The stacked motion is compared bit for bit.

val_motion's partials are per clip.  They are checked twice under the same rule: summed over the clips
against the whole batch's terms (with the self-check on the sentinel element), and clip by clip against
loss_ref on that clip alone (a one-clip batch), which pins the clip order of `part`.

Model tests hold validate() to the composition of the already pinned public ops at relative 1e-4, the
project's parity bar: eval G(audio, real_pose), D on diff_time of each pose separately, motion_losses,
mse_loss against ones and zeros, a host read per term as the reference does.
"""
import numpy as np
import pytest
import torch

import loss_ref as R
import test_gpu_losses_fp64 as L
from test_gpu_configs import _models

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda', 0)

VAL_MOTION_SHAPES = [(1, 2, 104), (2, 3, 104), (2, 4, 104), (3, 65, 104), (2, 33, 7), (130, 5, 104), (1, 512, 6)]
KEYS3 = ('l1', 'smooth', 'jerk')
CANARY = -7777.25


def _counts(B, T, Fd):
    """Divisors of the three motion terms (a term over no frames keeps 1: its sum is 0)."""
    return [B * (T - 1) * Fd, max(B * (T - 2), 1), max(B * (T - 3), 1)]


# ------------------------------------------------------------------------------ val_motion
@pytest.mark.parametrize('shape', VAL_MOTION_SHAPES, ids=L._mid)
def test_val_motion(shape, request):
    """T = 2, 3, 4: terms over no frames and over one; T = 65: the 64-step time loop's second trip,
    whose rows wrap the LDS ring; T = 512: eight trips; Fd = 6, 7: ragged feature quads; B = 130:
    more clips than the finish kernel has lanes.  The outputs sit in larger buffers whose
    tails must keep their canary."""
    from a2m import functional as F
    B, T, Fd = shape
    fake, real = L.motion_inputs(B, T, Fd)
    n = 2 * B * (T - 1) * Fd
    mbuf = torch.full((n + 256,), CANARY, device=DEV)
    pbuf = torch.full((3 * B + 16,), CANARY, dtype=torch.float64, device=DEV)
    motion, part = F.val_motion(torch.from_numpy(fake).to(DEV), torch.from_numpy(real).to(DEV),
                                mbuf[:n].view(2 * B, T - 1, Fd), pbuf[:3 * B].view(B, 3))
    torch.cuda.synchronize()
    assert motion.data_ptr() == mbuf.data_ptr() and part.data_ptr() == pbuf.data_ptr()
    assert (mbuf[n:] == CANARY).all() and (pbuf[3 * B:] == CANARY).all()
    got_m = L._np(motion)
    assert np.array_equal(got_m[:B], torch.diff(torch.from_numpy(fake), dim=1).numpy())
    assert np.array_equal(got_m[B:], torch.diff(torch.from_numpy(real), dim=1).numpy())
    got = L._np(part)
    assert got.dtype == np.float64 and got.shape == (B, 3)
    E = L.e32()
    fails, name = [], request.node.callspec.id
    live = [True, T > 2, T > 3]
    # the clips summed, against the whole batch (with the self-check on the last element)
    ref = R.motion_terms(fake, real)
    for i, k in enumerate(KEYS3):
        val = got[:, i].sum() / _counts(B, T, Fd)[i]
        if not live[i]:
            assert (got[:, i] == 0.0).all(), f'{k} over no frames is 0'
            continue
        shift = [abs(R.motion_terms(fake, real, {k: L.LAST})[i] - ref[i])]
        L.check_scalar('val-motion', name, k, val, ref[i], 8.0 * E[k] * ref[i], shift, fails)
    # clip by clip, each a one-clip batch under the same rule
    for b in range(B):
        one = R.motion_terms(fake[b:b + 1], real[b:b + 1])
        for i, k in enumerate(KEYS3):
            if live[i]:
                val = got[b, i] / _counts(1, T, Fd)[i]
                L.check_scalar('val-motion-clip', f'{name}-clip{b}', k, val, one[i], 8.0 * E[k] * one[i], None, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_val_motion_allocates_its_outputs():
    from a2m import functional as F
    fake, real = L.motion_inputs(2, 33, 7)
    f, r = torch.from_numpy(fake).to(DEV), torch.from_numpy(real).to(DEV)
    motion, part = F.val_motion(f, r)
    assert tuple(motion.shape) == (4, 32, 7) and motion.dtype == torch.float32
    assert tuple(part.shape) == (2, 3) and part.dtype == torch.float64
    m2, p2 = F.val_motion(f, r, motion.clone().fill_(1.0), part.clone().fill_(1.0))
    assert torch.equal(m2, motion) and torch.equal(p2, part)         # overwritten, and reproducible
    with pytest.raises(TypeError):
        F.val_motion(f, r, None, torch.empty(2, 3, device=DEV))


# ------------------------------------------------------------------------------ val_finish
def _finish_inputs(B, T, Fd, Lg, seed):
    """part: float64 sums of the size real clips give; logits float32 with a sentinel in the last fake and
    the last real element (the terms the self-check leaves out); bone, angle float32 scalars."""
    rng = np.random.default_rng(seed)
    part = np.stack([rng.uniform(0.5, 1.5, B) * (T - 1) * Fd, rng.uniform(0.5, 1.5, B) * 14.0 * max(T - 2, 0),
                     rng.uniform(0.5, 1.5, B) * 25.0 * max(T - 3, 0)], axis=1)
    logits = rng.standard_normal((2 * B, Lg)).astype(np.float32)
    logits[B - 1, -1] = np.float32(4.0)
    logits[-1, -1] = np.float32(-2.0)
    bone, angle = np.float32(rng.uniform(0.1, 0.9)), np.float32(rng.uniform(0.1, 0.9))
    return part, logits, bone, angle


def _finish_reference(part, T, Fd, logits, bone, angle, lg, ld):
    """(values [8], tolerances [8], shifts [8]) of one call by loss_ref and the module's rule."""
    E = L.e32()
    B = part.shape[0]
    fake, real = logits[:B], logits[B:]
    ones, zeros = np.ones_like(fake), np.zeros_like(fake)
    cnt = _counts(B, T, Fd)
    terms = [float(part[:, i].sum() / cnt[i]) for i in range(3)]
    lost = [float(part[:-1, i].sum() / cnt[i]) for i in range(3)]           # the last clip's partial left out
    t_tol = [8.0 * E[k] * v for k, v in zip(KEYS3, terms)]
    mse = {k: R.mse_loss(p, t) for k, p, t in (('f1', fake, ones), ('f0', fake, zeros), ('r1', real, ones))}
    mse_lost = {k: R.mse_loss(p, t, -1) for k, p, t in (('f1', fake, ones), ('f0', fake, zeros), ('r1', real, ones))}
    m_tol = {k: 8.0 * E['mse'] * v for k, v in mse.items()}
    lg, ld = L._f32(lg), L._f32(ld)
    vals = [terms[0] + lg * mse['f1'], mse['r1'] + ld * mse['f0'], float(bone), float(angle), terms[1], terms[2],
            terms[0], 1.0]
    tols = [t_tol[0] + lg * m_tol['f1'], m_tol['r1'] + ld * m_tol['f0'], 0.0, 0.0, t_tol[1], t_tol[2], t_tol[0], 0.0]
    shifts = [[abs(lost[0] - terms[0]), lg * abs(mse_lost['f1'] - mse['f1'])],
              [abs(mse_lost['r1'] - mse['r1']), ld * abs(mse_lost['f0'] - mse['f0'])], [], [],
              [abs(lost[1] - terms[1])] if T > 2 else [], [abs(lost[2] - terms[2])] if T > 3 else [],
              [abs(lost[0] - terms[0])], []]
    return np.array(vals), np.array(tols), shifts


def _run_finish(part, T, Fd, logits, bone, angle, lg, ld, acc):
    from a2m import functional as F
    return F.val_finish(torch.from_numpy(part).to(DEV), T, Fd, torch.from_numpy(logits).to(DEV),
                        torch.tensor(bone, device=DEV), torch.tensor(angle, device=DEV), lg, ld, acc)


FINISH_NAMES = ('g_loss', 'd_loss', 'bone', 'angle', 'smooth', 'jerk', 'motion_l1', 'count')


def _check_acc(name, got, start, vals, tols, shifts, fails):
    for i, q in enumerate(FINISH_NAMES):
        want = start[i] + vals[i]
        if tols[i] == 0.0:                      # bone, angle, the call count: exact
            if got[i] != want:
                fails.append(f'{q}: {got[i]!r} != {want!r}')
            continue
        # the tolerance and the shifts are the term's own; the accumulator's start is exact
        L.check_scalar('val-finish', name, q, got[i] - start[i], vals[i], tols[i], shifts[i], fails)


@pytest.mark.parametrize('lam', [(1.0, 1.0), (0.5, 2.0)], ids=['lam1-1', 'lam0.5-2'])
@pytest.mark.parametrize('B', [1, 3, 130], ids=lambda b: f'B{b}')
@pytest.mark.parametrize('Lg', [1, 4, 5], ids=lambda v: f'L{v}')
def test_val_finish(Lg, B, lam, request):
    """Two calls with different inputs (T = 9, then T = 3: no jerk frames) into an accumulator that
    starts at zero and into one that starts at non-zero values: each call adds its eight terms,
    acc[7] counts the calls, and the first call into a second fresh accumulator gives the same bytes.
    The non-zero start is dyadic and small, so that start + bone is exact in float64."""
    Fd = 104
    name = request.node.callspec.id
    calls = [(9, _finish_inputs(B, 9, Fd, Lg, 100 * B + Lg)), (3, _finish_inputs(B, 3, Fd, Lg, 100 * B + Lg + 50))]
    starts = [np.zeros(8), np.array([2.0, 4.0, 2.0, 1.0, 8.0, 16.0, 0.5, 3.0])]
    fails = []
    for start in starts:
        acc = torch.from_numpy(start.copy()).to(DEV)
        tot, tol_tot = np.zeros(8), np.zeros(8)
        for k, (T, (part, logits, bone, angle)) in enumerate(calls):
            before = L._np(acc).copy()
            out = _run_finish(part, T, Fd, logits, bone, angle, lam[0], lam[1], acc)
            assert out.data_ptr() == acc.data_ptr()
            got = L._np(acc)
            vals, tols, shifts = _finish_reference(part, T, Fd, logits, bone, angle, *lam)
            _check_acc(f'{name}-start{start[0]:g}-call{k + 1}', got, before, vals, tols, shifts, fails)
            tot, tol_tot = tot + vals, tol_tot + tols
            assert got[7] == start[7] + k + 1
            if T == 3:
                assert got[5] == before[5]                                  # jerk over no frames adds 0
        assert np.all(np.abs(L._np(acc) - start - tot) <= tol_tot + 1e-15 * np.abs(start))
    T, (part, logits, bone, angle) = calls[0]
    a, b = torch.zeros(8, dtype=torch.float64, device=DEV), torch.zeros(8, dtype=torch.float64, device=DEV)
    _run_finish(part, T, Fd, logits, bone, angle, lam[0], lam[1], a)
    _run_finish(part, T, Fd, logits, bone, angle, lam[0], lam[1], b)
    assert L._np(a).tobytes() == L._np(b).tobytes() and L._np(a)[7] == 1.0
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_val_finish_terms_over_no_frames():
    """T = 2: smoothness and jerk add exactly 0 whatever `part` holds there."""
    part, logits, bone, angle = _finish_inputs(3, 2, 104, 4, 7)
    part[:, 1:] = 5.0
    acc = torch.zeros(8, dtype=torch.float64, device=DEV)
    _run_finish(part, 2, 104, logits, bone, angle, 1.0, 1.0, acc)
    got = L._np(acc)
    assert got[4] == 0.0 and got[5] == 0.0 and got[6] > 0 and got[7] == 1.0


def test_val_finish_refuses_wrong_dtypes():
    from a2m import functional as F
    part, logits, bone, angle = _finish_inputs(2, 9, 104, 4, 3)
    args = dict(part=torch.from_numpy(part).to(DEV), logits=torch.from_numpy(logits).to(DEV),
                bone=torch.tensor(bone, device=DEV), angle=torch.tensor(angle, device=DEV),
                acc=torch.zeros(8, dtype=torch.float64, device=DEV))

    def call(**kw):
        a = {**args, **kw}
        return F.val_finish(a['part'], 9, 104, a['logits'], a['bone'], a['angle'], 1.0, 1.0, a['acc'])

    with pytest.raises(TypeError):
        call(acc=torch.zeros(8, device=DEV))
    with pytest.raises(TypeError):
        call(part=args['part'].float())
    with pytest.raises(TypeError):
        call(logits=args['logits'].double())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        call(acc=torch.zeros(8, dtype=torch.float64))
    assert not args['acc'].any()


# ------------------------------------------------------------------------------ the models
T_MODEL = 64
LAMBDAS = (0.5, 2.0)


def _batches(sizes, seed, dev=DEV):
    from oracle import synth
    out = []
    for k, B in enumerate(sizes):
        gen = torch.Generator().manual_seed(seed + 10 * k)
        audio = torch.randn(B, T_MODEL, 128, generator=gen) * 2.0 - 3.0
        pose = torch.from_numpy(synth.pose_targets(B, T_MODEL, seed=seed + 10 * k + 1))
        out.append((audio.to(dev), pose.to(dev)))
    return out


def _trainer(graphs=False, lr=1e-3, models=None):
    from a2m.training import GANTrainer
    g, d = models if models is not None else _models(DEV)
    return GANTrainer(g, d, lr=lr, lambda_gan=LAMBDAS[0], lambda_d=LAMBDAS[1], fixed_labels=(0.93, 0.07),
                      graphs=graphs)


def composition(G, D, batches, lambda_gan, lambda_d):
    """The reference-shaped pass from the public ops: two D forwards, the motion losses and three MSE
    launches per batch, a host read per term, the batches averaged equally."""
    from a2m import functional as F
    flags = [(m, m.training) for net in (G, D) for m in net.modules()]
    G.eval()
    D.eval()
    tot = dict.fromkeys(('g_loss', 'd_loss', 'bone_loss', 'angle_loss', 'smoothness_loss', 'jerk_loss', 'motion_l1'), 0.0)
    with torch.no_grad():
        for audio, real_pose in batches:
            fake_pose, internal = G(audio, real_pose=real_pose)
            tot['bone_loss'] += internal[0].item()
            tot['angle_loss'] += internal[1].item()
            fake_d, _ = D(F.diff_time(fake_pose))
            real_d, _ = D(F.diff_time(real_pose))
            terms, _ = F.motion_losses(fake_pose, real_pose)
            ones, zeros = torch.ones_like(fake_d), torch.zeros_like(fake_d)
            tot['motion_l1'] += terms[0].item()
            tot['smoothness_loss'] += terms[1].item()
            tot['jerk_loss'] += terms[2].item()
            tot['g_loss'] += terms[0].item() + lambda_gan * F.mse_loss(fake_d, ones)[0].item()
            tot['d_loss'] += F.mse_loss(real_d, ones)[0].item() + lambda_d * F.mse_loss(fake_d, zeros)[0].item()
    for m, f in flags:
        m.training = f
    out = {k: v / len(batches) for k, v in tot.items()}
    out['steps'] = len(batches)
    return out


def _parity(got, want, rel=1e-4):
    assert sorted(got) == sorted(want) and got['steps'] == want['steps']
    for k, v in want.items():
        print(f'VAL {k}: validate {got[k]!r} composition {v!r}')
        assert got[k] == pytest.approx(v, rel=rel), k


def _moved(a, b):
    """The largest relative change of a term from a to b."""
    return max(abs(a[k] - b[k]) / abs(a[k]) for k in ('g_loss', 'd_loss', 'smoothness_loss'))


def test_validate_matches_the_public_ops():
    """Two dev batches of 2 and 3 clips at T = 64 on the default models (train mode before, so the
    pass must switch to eval itself): every term at 1e-4, host batches give the same result as device
    batches bit for bit, and the flags are back."""
    tr = _trainer()
    dev = _batches([2, 3], seed=41)
    got = tr.validate(dev)
    assert tr.G.training and tr.D.training and all(isinstance(got[k], float) for k in tr.VAL_KEYS)
    _parity(got, composition(tr.G, tr.D, dev, *LAMBDAS))
    assert got['bone_loss'] > 0 and got['jerk_loss'] > 0 and got['steps'] == 2
    host = [(a.cpu(), p.cpu()) for a, p in dev]
    assert tr.validate(host) == got


@pytest.mark.parametrize('graphs', [False, True], ids=['eager', 'graphs'])
def test_validate_follows_the_weights(graphs):
    """validate, one training iteration, validate: the second result is the composition on the updated
    weights (no derived weight layout is served stale) and has moved by more than ten times the parity
    bar.  With graphs=True the trainer is past GRAPH_WARMUP for both step kinds first, so the iteration in
    between is a replay; validate itself stays eager and leaves the captured steps alone."""
    tr = _trainer(graphs=graphs)
    train, dev = _batches([4], seed=51)[0], _batches([2, 3], seed=41)
    if graphs:
        for it in range(3):
            tr.iteration(*train, epoch=it, g_freq=3, d_freq=1)
        assert tr._captured['g'] is not None and tr._captured['d'] is not None
    captured = dict(tr._captured)
    first = tr.validate(dev)
    _parity(first, composition(tr.G, tr.D, dev, *LAMBDAS))
    tr.iteration(*train, epoch=3, g_freq=3, d_freq=1)
    second = tr.validate(dev)
    _parity(second, composition(tr.G, tr.D, dev, *LAMBDAS))
    print(f'VAL moved by {_moved(first, second):.3e}')
    assert _moved(first, second) > 1e-3
    assert tr._captured == captured and tr.G.training and tr.D.training


def test_validate_loop_does_not_synchronise():
    """With device batches the accumulation loop runs under torch's sync debug mode 'error'; the pass's
    one read (8 doubles, GANTrainer._validate_read) is the only thing that synchronises."""
    tr = _trainer()
    dev = _batches([2, 3], seed=41)
    want = tr.validate(dev)                     # caches, workspaces and buffers exist from here on
    torch.cuda.synchronize()
    probe = torch.ones(1, device=DEV)
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        try:
            probe.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            acc, n = tr._validate_accumulate(dev)
            with pytest.raises(RuntimeError):
                tr._validate_read(acc)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    if not honoured:
        pytest.skip("the installed ROCm torch does not honour torch.cuda.set_sync_debug_mode('error')")
    sums = tr._validate_read(acc)
    assert n == 2 and sums[7] == 2.0
    assert {k: v / 2 for k, v in zip(tr.VAL_KEYS, sums)} == {k: want[k] for k in tr.VAL_KEYS}


def test_fit_checkpoints_reload(tmp_path):
    """Two epochs of one train batch (B = 2) and one dev batch: the files the reference writes exist,
    load_generator reads gen/Best_Gen, and fresh models loaded from gen/epoch_1 and dis/epoch_1 reproduce
    the second epoch's validation terms."""
    from a2m.inference import load_generator
    from a2m.real_motion_model import SelfAttention_D, SelfAttention_G
    tr = _trainer()
    train, dev = _batches([2], seed=61), _batches([3], seed=41)
    rec = tr.fit(train, dev, 2, save_dir=str(tmp_path), log=lambda s: None)
    assert len(rec['val_terms']) == 2 and rec['train_g'] == []
    assert sorted(p.name for p in (tmp_path / 'gen').iterdir()) == ['Best_Gen', 'epoch_0', 'epoch_1']
    assert sorted(p.name for p in (tmp_path / 'dis').iterdir()) == ['epoch_0', 'epoch_1']
    assert torch.load(tmp_path / 'loss.npy', weights_only=True)['val_g'] == rec['val_g']
    best = load_generator(str(tmp_path / 'gen' / 'Best_Gen'), device=DEV, p=0.0)
    assert isinstance(best, SelfAttention_G) and not best.training
    k = 1 if rec['val_g'][1] < rec['val_g'][0] else 0
    kept = torch.load(tmp_path / 'gen' / f'epoch_{k}', map_location='cpu', weights_only=True)
    assert all(torch.equal(v.cpu(), kept[n]) for n, v in best.state_dict().items())
    g, d = SelfAttention_G(p=0.0), SelfAttention_D(out_channels=64, p=0.0)
    g.load_state_dict(torch.load(tmp_path / 'gen' / 'epoch_1', map_location='cpu', weights_only=True))
    d.load_state_dict(torch.load(tmp_path / 'dis' / 'epoch_1', map_location='cpu', weights_only=True))
    again = _trainer(models=(g.to(DEV).train(), d.to(DEV).train())).validate(dev)
    _parity(again, rec['val_terms'][1])
