"""GANTrainer.validate and GANTrainer.fit on the CPU: the host side of the validation epoch and of
the epoch loop (version5_model_train.py:325-532).

The HIP kernels cannot run here, so, as tests/test_dp_cpu.py does, the trainer's device ops are
swapped for torch stand-ins -- among them stand-ins for the two new calls, functional.val_motion
and functional.val_finish, written from their contract in include/a2m.h -- and small torch G / D
modules with the reference's call contract take the models' place.  Under test: the batch
averaging, the eval / no-grad discipline, the flag restoration, the all-reduce of the sums, the
checkpoint policy and the loss record.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

T, FD = 12, 104
LAMBDA_GAN, LAMBDA_D = 0.5, 2.0


class TinyG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.inp = torch.nn.Linear(128, 32)
        self.drop = torch.nn.Dropout(0.5)       # eval and train forwards differ
        self.lin = torch.nn.Linear(32, FD)
        self.fail_at = None                     # raise in this forward (0-based) of an eval pass
        self.calls = 0

    def forward(self, audio, real_pose=None):
        if not self.training:
            if self.fail_at is not None and self.calls == self.fail_at:
                raise RuntimeError('TinyG: planned failure')
            self.calls += 1
        pose = self.lin(self.drop(torch.tanh(self.inp(audio))))
        internal = [(pose ** 2).mean() * 1e-3]
        if real_pose is not None:
            internal.insert(0, (pose - real_pose).abs().mean() * 1e-2)
        return pose, internal


class TinyD(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = torch.nn.Linear(FD, 1)
        self.bn = torch.nn.BatchNorm1d(4)       # running statistics in eval: per-sample independent

    def forward(self, x, audio=None, aux_labels=None):
        y = self.lin(x)[:, :4, 0]
        return self.bn(y), []


def stand_ins():
    """[(module, attribute, torch stand-in)] for the device ops the trainer calls."""
    from a2m import autograd as AG
    from a2m import functional as F
    from oracle import model as OM

    def motion_terms(fake, real):
        return torch.stack(OM.motion_terms(real, fake))

    def adam_(p, g, m, v, lr, b1, b2, eps, wd, step):
        m.mul_(b1).add_(g, alpha=1 - b1)
        v.mul_(b2).addcmul_(g, g, value=1 - b2)
        p.addcdiv_(m, (v / (1 - b2 ** step)).sqrt_().add_(eps), value=-lr / (1 - b1 ** step))

    def gather_segments_(dst, segs):
        for o, t in segs:
            dst[o:o + t.numel()].copy_(t.reshape(-1))
        return dst

    def val_motion(fake_pose, real_pose, motion=None, part=None):
        B = fake_pose.shape[0]
        mf, mr = torch.diff(fake_pose, dim=1), torch.diff(real_pose, dim=1)
        acc = mf[:, 1:] - mf[:, :-1]
        jerk = acc[:, 1:] - acc[:, :-1]
        m = torch.cat([mf, mr])
        p = torch.stack([(mr - mf).abs().double().sum((1, 2)), acc.norm(dim=2).double().sum(1),
                         jerk.norm(dim=2).double().sum(1)], dim=1)
        motion = m.clone() if motion is None else motion.copy_(m)
        part = p if part is None else part.copy_(p)
        assert part.dtype == torch.float64 and tuple(part.shape) == (B, 3)
        return motion, part

    def val_finish(part, T_, Fd, logits, bone, angle, lambda_gan, lambda_d, acc):
        B = part.shape[0]
        assert acc.dtype == torch.float64 and tuple(logits.shape[:1]) == (2 * B,)
        f, r = logits[:B].double(), logits[B:].double()
        s = part.sum(0)
        l1 = s[0] / (B * (T_ - 1) * Fd)
        smooth = s[1] / (B * (T_ - 2)) if T_ > 2 else torch.zeros((), dtype=torch.float64)
        jerk = s[2] / (B * (T_ - 3)) if T_ > 3 else torch.zeros((), dtype=torch.float64)
        acc += torch.stack([l1 + lambda_gan * ((f - 1) ** 2).mean(), ((r - 1) ** 2).mean() + lambda_d * (f ** 2).mean(),
                            bone.double().reshape(()), angle.double().reshape(()), smooth, jerk, l1,
                            torch.ones((), dtype=torch.float64)])
        return acc

    return [(AG, 'pos_to_motion', lambda x: torch.diff(x, dim=1)), (AG, 'motion_terms', motion_terms),
            (AG, 'mse_loss', torch.nn.functional.mse_loss), (F, 'adam_', adam_),
            (F, 'gather_segments_', gather_segments_), (F, 'val_motion', val_motion), (F, 'val_finish', val_finish)]


@pytest.fixture
def patched(monkeypatch):
    for mod, name, fn in stand_ins():
        monkeypatch.setattr(mod, name, fn)


def _models():
    torch.manual_seed(11)
    g, d = TinyG(), TinyD()
    with torch.no_grad():                      # running statistics away from the (0, 1) defaults
        d.bn.running_mean.copy_(torch.tensor([0.1, -0.2, 0.3, 0.0]))
        d.bn.running_var.copy_(torch.tensor([0.5, 1.5, 1.0, 2.0]))
    return g.train(), d.train()


def _batches(sizes, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(B, T, 128, generator=g), torch.randn(B, T, FD, generator=g)) for B in sizes]


def _trainer(**kw):
    from a2m.training import GANTrainer
    g, d = _models()
    return GANTrainer(g, d, lr=1e-2, lambda_gan=LAMBDA_GAN, lambda_d=LAMBDA_D, fixed_labels=(0.93, 0.07), **kw)


def restated_validate(G, D, batches, lambda_gan, lambda_d):
    """The reference's validation pass (:427-499) in plain torch-CPU float32, with its three D
    forwards and its per-batch averaging; plus the motion L1 on its own."""
    mse, l1 = torch.nn.MSELoss(), torch.nn.L1Loss()
    was = G.training, D.training
    G.eval()
    D.eval()
    tot = dict(g_loss=0.0, d_loss=0.0, bone_loss=0.0, angle_loss=0.0, smoothness_loss=0.0, jerk_loss=0.0,
               motion_l1=0.0)
    steps = 0
    with torch.no_grad():
        for audio, real_pose in batches:
            fake_pose, internal = G(audio, real_pose=real_pose)
            tot['bone_loss'] += internal[0].item()
            tot['angle_loss'] += internal[1].item()
            real_m, fake_m = torch.diff(real_pose, dim=1), torch.diff(fake_pose, dim=1)
            accel = fake_m[:, 1:] - fake_m[:, :-1]
            tot['smoothness_loss'] += torch.norm(accel, dim=-1).mean().item()
            tot['jerk_loss'] += torch.norm(accel[:, 1:] - accel[:, :-1], dim=-1).mean().item()
            ones = torch.ones(real_pose.shape[0], 4)
            zeros = torch.zeros(real_pose.shape[0], 4)
            reg = l1(real_m, fake_m)
            tot['motion_l1'] += reg.item()
            tot['g_loss'] += (reg + lambda_gan * mse(D(fake_m)[0], ones)).item()
            real_d, fake_d = D(real_m)[0], D(fake_m.detach())[0]
            tot['d_loss'] += (mse(real_d, ones) + lambda_d * mse(fake_d, zeros)).item()
            steps += 1
    G.train(was[0])
    D.train(was[1])
    out = {k: v / steps for k, v in tot.items()}
    out['steps'] = steps
    return out


def _close(got, want, rel=1e-5):
    assert sorted(got) == sorted(want)
    assert got['steps'] == want['steps']
    for k, v in want.items():
        assert got[k] == pytest.approx(v, rel=rel), k


def test_validate_equals_the_restated_reference(patched):
    """Batches of 3 and 5 clips: every returned term equals the restatement to float32 rounding
    (both sides are torch-CPU float32 and differ only in summation order), and the batches weigh
    equally -- the mean of the two one-batch results, not the sample-weighted mean."""
    tr = _trainer()
    batches = _batches([3, 5])
    got = tr.validate(batches)
    want = restated_validate(tr.G, tr.D, batches, LAMBDA_GAN, LAMBDA_D)
    _close(got, want)
    assert all(isinstance(v, float) for k, v in got.items() if k != 'steps') and got['steps'] == 2
    one = [tr.validate([b]) for b in batches]
    for k in tr.VAL_KEYS:
        assert got[k] == pytest.approx((one[0][k] + one[1][k]) / 2, rel=1e-9), k
    by_sample = (3 * one[0]['g_loss'] + 5 * one[1]['g_loss']) / 8
    assert abs(got['g_loss'] - by_sample) > 1e-4 * abs(got['g_loss'])
    # a generator yields the same result as a list, and the buffers are kept per batch shape
    _close(tr.validate(b for b in batches), got, rel=1e-12)
    assert sorted(k[0] for k in tr._val_bufs) == [3, 5]


def test_validate_restores_training_flags(patched):
    """Every submodule gets its own previous flag back -- one was in eval before the call -- after
    a normal pass and after G raises in the second batch; the pass itself runs in eval mode."""
    tr = _trainer()
    tr.G.drop.eval()
    before = [(m, m.training) for net in (tr.G, tr.D) for m in net.modules()]
    assert [f for _, f in before].count(False) == 1
    seen = []
    hook = tr.D.register_forward_pre_hook(lambda m, a: seen.append((tr.G.training, m.training, m.bn.training,
                                                                   torch.is_grad_enabled())))
    tr.validate(_batches([3, 5]))
    hook.remove()
    assert seen == [(False, False, False, False)] * 2          # one D forward per batch, eval, no grad
    assert all(m.training == f for m, f in before)
    tr.G.calls, tr.G.fail_at = 0, 1
    with pytest.raises(RuntimeError, match='planned failure'):
        tr.validate(_batches([3, 5]))
    assert tr.G.calls == 1
    assert all(m.training == f for m, f in before)


def test_validate_leaves_gradients_and_trainer_state_alone(patched):
    tr = _trainer(graphs=False)
    params = list(tr.G.parameters()) + list(tr.D.parameters())
    params[1].requires_grad_(False)
    grads = []
    for i, p in enumerate(params):
        p.grad = None if i % 2 else torch.full_like(p, 0.25 * (i + 1))
        grads.append(p.grad)
    state = (tr.opt_G.step_count, tr.opt_D.step_count, tr.opt_G.flat.clone(), tr.opt_D.flat.clone(),
             list(tr.dyn.d_loss_history), tr._label_gen, tr._seed_ctr, dict(tr._captured), dict(tr._warm))
    bn = (tr.D.bn.running_mean.clone(), tr.D.bn.running_var.clone(), tr.D.bn.num_batches_tracked.clone())
    tr.validate(_batches([3, 5]))
    for i, (p, g) in enumerate(zip(params, grads)):
        assert p.grad is g and p.requires_grad == (i != 1)
        assert g is None or torch.equal(g, torch.full_like(p, 0.25 * (i + 1)))
    assert (tr.opt_G.step_count, tr.opt_D.step_count) == state[:2]
    assert torch.equal(tr.opt_G.flat, state[2]) and torch.equal(tr.opt_D.flat, state[3])
    assert tr.dyn.d_loss_history == state[4] and tr._label_gen is state[5] and tr._seed_ctr is state[6]
    assert tr._captured == state[7] and tr._warm == state[8]
    assert torch.equal(tr.D.bn.running_mean, bn[0]) and torch.equal(tr.D.bn.running_var, bn[1])
    assert torch.equal(tr.D.bn.num_batches_tracked, bn[2])


def test_validate_refuses_empty_input(patched):
    tr = _trainer()
    with pytest.raises(ValueError, match='no batches'):
        tr.validate([])
    with pytest.raises(ValueError, match='no batches'):
        tr.validate(iter(()))
    assert tr.G.training and tr.D.training


# ------------------------------------------------------------------------------ two gloo ranks
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, q):
    key = 'ref' if world == 1 else rank
    try:
        for mod, name, fn in stand_ins():
            setattr(mod, name, fn)
        batches = _batches([3, 5, 4])
        if world == 1:
            q.put((key, _trainer().validate(batches)))
            return
        os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        dist.init_process_group('gloo', rank=rank, world_size=world)
        try:
            q.put((key, _trainer().validate(batches[:2] if rank == 0 else batches[2:])))
        finally:
            dist.destroy_process_group()
    except Exception as e:          # the parent fails at once instead of waiting for the queue
        q.put((key, repr(e)))
        raise


@pytest.mark.timeout(300)
def test_validate_two_ranks_average_over_all_batches():
    """Rank 0 holds two batches, rank 1 one: both return the one-process result over the three."""
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(0, 1, port, q))]
    procs += [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=240) for _ in procs)
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert res['ref']['steps'] == 3
    for r in (0, 1):
        _close(res[r], res['ref'], rel=1e-12)


# ------------------------------------------------------------------------------ fit
def _tensors_equal(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_fit_checkpoints_and_loss_record(patched, tmp_path):
    """Three epochs of five train batches with log_every = 2: two logged batches per epoch (i = 1,
    3), one history entry per epoch, Best_Gen holding the tensors of the last epoch whose
    validation G loss was a strict new minimum, epoch files for G and D, loss.npy the returned
    record; the saved G reproduces its epoch's validation terms."""
    tr = _trainer()
    train, dev = _batches([4] * 5, seed=5), _batches([3, 5], seed=6)
    lines = []
    rec = tr.fit(train, dev, 3, save_dir=str(tmp_path), log_every=2, log=lines.append)
    assert sorted(rec) == ['dynamic_stats', 'train_d', 'train_g', 'val_d', 'val_g', 'val_terms']
    assert len(rec['train_g']) == len(rec['train_d']) == 3 * len([i for i in range(5) if i % 2 == 1])
    assert rec['train_g'] == [tr.dyn.g_loss_history[i] for i in (1, 3, 6, 8, 11, 13)]
    assert len(rec['val_g']) == len(rec['val_d']) == len(rec['val_terms']) == 3
    assert [v['g_loss'] for v in rec['val_terms']] == rec['val_g']
    assert sorted(rec['dynamic_stats']) == ['d_freq_history', 'd_lr_history', 'g_freq_history', 'g_lr_history']
    assert all(len(v) == 3 for v in rec['dynamic_stats'].values())
    assert rec['dynamic_stats']['g_freq_history'][-1] == tr.dyn.g_train_freq
    assert rec['dynamic_stats']['g_lr_history'][-1] == tr.dyn.g_lr_current
    assert any(s.startswith('[Validation] Epoch 2/3') for s in lines)
    assert sorted(os.listdir(tmp_path)) == ['dis', 'gen', 'loss.npy']
    assert sorted(os.listdir(tmp_path / 'gen')) == ['Best_Gen', 'epoch_0', 'epoch_1', 'epoch_2']
    assert sorted(os.listdir(tmp_path / 'dis')) == ['epoch_0', 'epoch_1', 'epoch_2']
    best_k, best = None, float('inf')
    for k, v in enumerate(rec['val_g']):
        if v < best:
            best_k, best = k, v
    load = lambda *p: torch.load(os.path.join(tmp_path, *p), map_location='cpu', weights_only=True)  # noqa: E731
    assert _tensors_equal(load('gen', 'Best_Gen'), load('gen', f'epoch_{best_k}'))
    for k in range(3):
        if k != best_k:
            assert not _tensors_equal(load('gen', 'Best_Gen'), load('gen', f'epoch_{k}'))
    assert _tensors_equal(load('gen', 'epoch_2'), tr.G.state_dict())
    assert _tensors_equal(load('dis', 'epoch_2'), tr.D.state_dict())
    saved = load('loss.npy')
    assert saved['val_g'] == rec['val_g'] and saved['train_d'] == rec['train_d']
    assert saved['dynamic_stats'] == rec['dynamic_stats']
    g1, d1 = _models()
    g1.load_state_dict(load('gen', 'epoch_1'))
    d1.load_state_dict(load('dis', 'epoch_1'))
    _close(restated_validate(g1, d1, dev, LAMBDA_GAN, LAMBDA_D), rec['val_terms'][1])


def test_fit_best_checkpoint_follows_the_strict_minimum(patched, tmp_path, monkeypatch):
    """The policy on a forced sequence of validation G losses: Best_Gen is rewritten at epochs 0
    and 2 (strict new minima), not at 1 (higher), 3 (a tie) or 4 (higher)."""
    tr = _trainer()
    seq = iter([0.5, 0.7, 0.3, 0.3, 0.4])
    real_validate = tr.validate

    def fake_validate(batches):
        out = real_validate(batches)
        out['g_loss'] = next(seq)
        return out

    monkeypatch.setattr(tr, 'validate', fake_validate)
    rec = tr.fit(_batches([4], seed=5), _batches([3], seed=6), 5, save_dir=str(tmp_path), log=lambda s: None)
    assert rec['val_g'] == [0.5, 0.7, 0.3, 0.3, 0.4]
    load = lambda name: torch.load(os.path.join(tmp_path, 'gen', name), map_location='cpu', weights_only=True)  # noqa: E731
    assert _tensors_equal(load('Best_Gen'), load('epoch_2'))
    assert not _tensors_equal(load('Best_Gen'), load('epoch_3'))


def test_fit_without_save_dir_writes_nothing(patched, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    tr = _trainer()
    rec = tr.fit(_batches([4] * 2, seed=5), _batches([3], seed=6), 2, log_every=1, log=lambda s: None, start_epoch=4)
    assert len(rec['val_g']) == 2 and len(rec['train_g']) == 4
    assert os.listdir(tmp_path) == []
