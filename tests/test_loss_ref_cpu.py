"""tests/loss_ref.py, the float64 numpy restatements that tests/test_gpu_losses_fp64.py bounds the
kernels with: every value and gradient against torch-CPU float64 autograd of oracle.model's
functions (torch.optim.Adam for the optimiser) at every shape the GPU module uses, the input
conditions of every GPU case, what `omit` leaves out, and the argument checks of the entry points
of csrc/losses.hip, csrc/train_loss.hip and csrc/evaluation.hip, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import loss_ref as R
import test_gpu_losses_fp64 as G
from conftest import rel_err
from oracle import model as OM

RTOL = 1e-11
CASES = G.cases()
POSES = [(f'B{c["B"]}-T{c["T"]}', c['gen'], c['real']) for c in CASES['pose']] + [('degenerate',) + CASES['pose_degenerate']]
MOTIONS = [('B%d-T%d-F%d' % f.shape, f, r) for f, r in CASES['motion']] + [('degenerate',) + CASES['motion_degenerate']]


def _close(a, b):
    return abs(a - b) <= RTOL * abs(b)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


# ------------------------------------------------------------------------------ the tables and chain_pose
def test_tables_are_the_oracles():
    assert R.PARENTS == OM.PARENTS
    assert R.HAND_TRIPLES == [tuple(t) for t in OM.HAND_TRIPLES]
    assert R.BODY_TRIPLES == [tuple(t) for t in OM.BODY_TRIPLES]
    assert all(0 <= p < j for j, p in enumerate(R.PARENTS) if j), 'every parent precedes its joint'


def test_chain_pose_keeps_bones_long_and_is_reproducible():
    p = R.chain_pose(3, 37, 100)
    assert p.dtype == np.float32 and p.shape == (3, 37, 104)
    assert np.array_equal(p, R.chain_pose(3, 37, 100)) and not np.array_equal(p, R.chain_pose(3, 37, 101))
    ln = R.bone_lengths(p)
    assert ln.min() >= 0.5 - 1e-5 and ln.max() < 1.5 + 1e-5
    # independent Gaussian joints are not such an input: bones far shorter than 0.05 occur
    g = np.random.default_rng(0).standard_normal((3, 37, 104)).astype(np.float32)
    assert R.bone_lengths(g).min() < 0.05
    joints = p.reshape(3, 37, 52, 2).astype(np.float64)
    assert abs(joints[:, :, 0].mean()) < 0.5 and 0.5 < joints[:, :, 0].std() < 1.5


# ------------------------------------------------------------------------------ references against torch float64
@pytest.mark.parametrize('name,gen,real', POSES, ids=[p[0] for p in POSES])
def test_pose_references_match_torch_float64(name, gen, real):
    g = _t64(gen).requires_grad_(True)
    for part, fn in (('hand', OM.hand_angle_loss), ('body', OM.body_angle_loss)):
        val = fn(g)
        grad, = torch.autograd.grad(val, g)
        assert _close(R.angle_loss(gen, part), val.item()), part
        assert rel_err(R.angle_grad(gen, part), grad.numpy()) <= RTOL, part
    val = OM.bone_length_loss(_t64(real), g)
    grad, = torch.autograd.grad(val, g)
    assert _close(R.bone_loss(gen, real), val.item())
    assert rel_err(R.bone_grad(gen, real), grad.numpy()) <= RTOL
    for w in CASES['weights']:
        for go in CASES['grad_outs']:
            for r in (real, None):
                ref = G.pose_torch(gen, r, w[0], w[1], go, torch.float64)['dgen']
                assert rel_err(G.pose_manual(gen, r, w[0], w[1], go), ref) <= RTOL


@pytest.mark.parametrize('name,fake,real', MOTIONS, ids=[m[0] for m in MOTIONS])
def test_motion_references_match_torch_float64(name, fake, real):
    T = fake.shape[1]
    onehots = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
    for r in (real, None):
        for gterms in [CASES['gterms']] + onehots:
            vals, grad = G.motion_torch(fake, r, gterms, torch.float64)
            mine = R.motion_terms(fake, r)
            assert all(_close(a, b) for a, b in zip(mine, vals))
            assert rel_err(R.motion_grad(fake, r, [G._f32(v) for v in gterms]), grad) <= RTOL
    # a term over no frames is 0 here where torch's empty mean is NaN
    raw = OM.motion_terms(_t64(real), _t64(fake))
    assert [bool(torch.isnan(t)) for t in raw] == [False, T <= 2, T <= 3]
    if T <= 3:
        assert mine[2] == 0.0
    if T <= 2:
        assert mine[1] == 0.0


@pytest.mark.parametrize('k', range(len(CASES['mse'])))
def test_mse_reference_matches_torch_float64(k):
    pred, target = CASES['mse'][k]
    p = _t64(pred).requires_grad_(True)
    loss = TF.mse_loss(p, _t64(target))
    (loss * 0.37).backward()
    assert _close(R.mse_loss(pred, target), loss.item())
    assert rel_err(R.mse_grad(pred, target, 0.37), p.grad.numpy()) <= RTOL


@pytest.mark.parametrize('n,wd', CASES['adam'], ids=[f'n{n}-wd{wd}' for n, wd in CASES['adam']])
def test_adam_reference_matches_torch_float64(n, wd):
    ref, t64 = G.adam_ref(n, wd), G.adam_torch(n, wd, torch.float64)
    for k in range(3):
        for q, a, b in zip('pmv', ref[k], t64[k]):
            assert rel_err(a, b) <= RTOL, (q, k + 1)
    # with plain double hyperparameters too, from a state that is not zero, at steps 4..5
    p0, grads = G.adam_inputs(min(n, 4099))
    p = p0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([p], lr=0.05, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd, foreach=False)
    seq = [g.double() for g in grads] + [grads[0].double() * 0.5, grads[1].double() * 3.0]
    for g in seq:
        p.grad = g.clone()
        opt.step()
    first = R.adam(p0.numpy(), [g.numpy() for g in seq[:3]], np.zeros(p0.numel()), np.zeros(p0.numel()), 0.05, 0.9,
                   0.999, 1e-8, wd)[-1]
    last = R.adam(first[0], [g.numpy() for g in seq[3:]], first[1], first[2], 0.05, 0.9, 0.999, 1e-8, wd,
                  first_step=4)[-1]
    st = opt.state[p]
    for a, b in zip(last, (p.detach(), st['exp_avg'], st['exp_avg_sq'])):
        assert rel_err(a, b.numpy()) <= RTOL


@pytest.mark.parametrize('shape,x,dy', CASES['interp'], ids=['H%d-W%d-T%d' % c[0] for c in CASES['interp']])
def test_interp_reference_matches_torch_float64(shape, x, dy):
    H, W, T = shape
    y, dx = G.interp_torch(x, dy, T, torch.float64)
    assert rel_err(R.interp_time(x.numpy(), T), y) <= RTOL
    assert rel_err(R.interp_time_bwd(dy.numpy(), H, W), dx) <= RTOL
    lost = R.interp_time_bwd(dy.numpy(), H, W) - R.interp_time_bwd(dy.numpy(), H, W, omit=-1)
    only = np.zeros_like(dy.numpy())
    only[:, :, -1] = dy.numpy()[:, :, -1]
    assert rel_err(lost, R.interp_time_bwd(only, H, W)) <= RTOL


def test_pose_moments_reference():
    pose = (np.random.default_rng(3).standard_normal((11, 104)) * 3 + 500).astype(np.float32)
    m1, m2, a1, a2 = R.pose_moments(pose, 0)
    assert rel_err(m1, pose.astype(np.float64).mean(0)) <= RTOL and rel_err(m2, (pose.astype(np.float64) ** 2).mean(0)) <= RTOL
    n1, n2, _, _ = R.pose_moments(pose, 1)
    sub = pose.copy()
    sub[:, :52] -= pose[:, :1]
    sub[:, 52:] -= pose[:, 52:53]
    assert sub.dtype == np.float32                       # the subtraction rounds to float32, as the kernel's
    assert rel_err(n1, sub.astype(np.float64).mean(0)) <= RTOL and rel_err(n2, (sub.astype(np.float64) ** 2).mean(0)) <= RTOL
    assert n1[0] == 0 and n1[52] == 0
    o1, _, _, _ = R.pose_moments(pose, 0, omit=-1)
    assert rel_err(m1 - o1, pose[-1].astype(np.float64) / 11) <= 1e-9


# ------------------------------------------------------------------------------ what omit leaves out
def test_omit_drops_one_term_and_keeps_the_divisor():
    _, gen, real = G.pose_inputs(2, 17)
    for part in ('hand', 'body'):
        t = R.angle_terms(gen, part)
        assert t[G.LAST] > 0
        assert _close(R.angle_loss(gen, part) - R.angle_loss(gen, part, G.LAST), t[G.LAST] / t.size)
        one = R.angle_grad(gen, part) - R.angle_grad(gen, part, G.LAST)
        assert np.abs(one[:-1]).max() == 0 and np.abs(one[-1, :-1]).max() == 0 and np.abs(one[-1, -1]).max() > 0
    lg, lr = R.bone_lengths(gen), R.bone_lengths(real)
    d = lg.mean(1) - lr.mean(1)
    d[-1, -1] -= lg[G.LAST] / 17
    assert _close(R.bone_loss(gen, real, G.LAST), (d * d).mean())
    fake, realm = G.motion_inputs(2, 33, 7)
    full, less = R.motion_terms(fake, realm), R.motion_terms(fake, realm, G.LAST)
    fm = np.diff(fake.astype(np.float64), axis=1)
    dm = fm - np.diff(realm.astype(np.float64), axis=1)
    assert _close(full[0] - less[0], abs(dm[G.LAST]) / dm.size)
    acc = np.diff(fm, axis=1)
    lost = np.linalg.norm(acc[-1, -1]) - np.linalg.norm(acc[-1, -1, :-1])
    assert abs((full[1] - less[1]) - lost / (2 * 31)) <= 1e-9 * full[1]
    assert less[2] < full[2]
    only_jerk = R.motion_terms(fake, realm, {'jerk': G.LAST})
    assert only_jerk[:2] == full[:2] and only_jerk[2] == less[2]
    pred, target = G.mse_inputs(257, 0)
    d2 = (pred.astype(np.float64) - target.astype(np.float64)) ** 2
    assert _close(R.mse_loss(pred, target) - R.mse_loss(pred, target, -1), d2[-1] / 257)


# ------------------------------------------------------------------------------ the GPU module's inputs
@pytest.mark.parametrize('case', CASES['pose'], ids=[f'B{c["B"]}-T{c["T"]}' for c in CASES['pose']])
def test_pose_cases_meet_the_input_condition(case):
    """At least 1e-5 rad from every kink (0 and +-pi for hand triples, -pi/2 and +-pi for body
    triples), the last hand and body terms active, and the first such seed from 100 within 64."""
    B, T, seed, gen = case['B'], case['T'], case['seed'], case['gen']
    assert G.SEED_BASE == 100 and 100 <= seed < 164
    assert np.array_equal(gen, R.chain_pose(B, T, seed)) and np.array_equal(case['real'], R.chain_pose(B, T, seed + 1000))
    for part, kinks in (('hand', (0.0, np.pi, -np.pi)), ('body', (-np.pi / 2, np.pi, -np.pi))):
        a = R.angles(gen, part)
        dist = min(np.abs(a - k).min() for k in kinks)
        assert dist >= 1e-5, (part, dist)
        assert abs(dist - R.kink_distance(gen, part)) <= 1e-15
        assert R.angle_terms(gen, part)[G.LAST] > 0
    assert R.bone_lengths(gen).min() >= 0.5 - 1e-5
    for s in range(100, seed):
        assert not G.pose_ok(R.chain_pose(B, T, s)), f'seed {s} already meets the condition'


def test_pose_shapes_cover_the_chunk_edges():
    shapes = [(c['B'], c['T']) for c in CASES['pose']]
    assert shapes == [(1, 1), (2, 15), (3, 16), (2, 17), (3, 37), (2, 64), (1, 100)]
    assert {T % 16 for _, T in shapes} >= {0, 1, 15, 5, 4} and max(T for _, T in shapes) > 64


def test_degenerate_pose_is_exact_in_float32():
    gen, real = CASES['pose_degenerate']
    for b, t in ((0, 3), (1, 16)):
        assert np.array_equal(gen[b, t], np.round(gen[b, t])) and np.abs(gen[b, t]).max() < 64
    assert R.bone_lengths(gen)[0, 3, 13] == 0.0 and R.angles(gen, 'hand')[0, 3, 2] == 0.0
    assert R.angles(gen, 'hand')[1, 16, 5] == 0.0
    for part in ('hand', 'body'):                        # nothing at the +-pi wrap
        assert (np.pi - np.abs(R.angles(gen, part))).min() >= 1e-5
    # torch gives zero gradient through atan2(0, 0), relu(0) and a zero norm: all finite
    ref = G.pose_torch(gen, real, 0.7, 0.3, (0.7, 1.3), torch.float64)
    assert np.isfinite(ref['dgen']).all() and np.isfinite([ref['bone'], ref['hand'], ref['body']]).all()


@pytest.mark.parametrize('name,fake,real', MOTIONS[:-1], ids=[m[0] for m in MOTIONS[:-1]])
def test_motion_cases_stay_off_the_l1_kink(name, fake, real):
    d = np.diff(fake.astype(np.float64), axis=1) - np.diff(real.astype(np.float64), axis=1)
    assert np.abs(d).min() >= 1e-5
    assert abs(d[G.LAST]) >= 3.0


def test_degenerate_motion_is_exact_in_float32():
    fake, real = CASES['motion_degenerate']
    f = fake.astype(np.float64)
    assert np.array_equal(f, np.round(f)) and np.abs(f).max() < 2 ** 12
    assert np.array_equal(fake[0], real[0])
    assert not np.diff(f, 2, axis=1)[1].any() and np.diff(f, 2, axis=1)[2].all() and not np.diff(f, 3, axis=1)[2].any()
    d = np.diff(f, axis=1) - np.diff(real.astype(np.float64), axis=1)
    assert not d[0].any() and d[1:].all()
    _, grad = G.motion_torch(fake, real, CASES['gterms'], torch.float64)
    assert np.isfinite(grad).all()


def test_scalar_pools_have_seven_cases_each():
    assert len(POSES) >= 7 and len(CASES['mse']) >= 7
    T = [f.shape[1] for f, _ in CASES['motion']]
    assert len(T) >= 7 and sum(t > 2 for t in T) >= 7 and sum(t > 3 for t in T) >= 7
    E = G.e32()
    assert sorted(E) == ['body', 'bone', 'hand', 'jerk', 'l1', 'mse', 'smooth']
    assert all(2.0 ** -30 < v < 2.0 ** -19 for v in E.values()), E


# ------------------------------------------------------------------------------ argument checks (no launch)
@pytest.fixture(scope='module')
def abi():
    from a2m import _native as N
    buf = (ctypes.c_float * 1024)()
    return N, ctypes.cast(buf, ctypes.c_void_p), buf


def test_entry_points_reject_bad_arguments(abi):
    N, p, _ = abi
    lib, EINVAL = N.lib, N.A2M_EINVAL
    big = 1 << 20
    for T in (1, 513):
        assert lib.a2m_motion_losses_f32(p, p, 2, T, 8, p, None, None, p, big, None) == EINVAL, T
    # grad_terms and dfake come together
    assert lib.a2m_motion_losses_f32(p, p, 2, 9, 8, p, p, None, p, big, None) == EINVAL
    assert lib.a2m_motion_losses_f32(p, p, 2, 9, 8, p, None, p, p, big, None) == EINVAL
    assert 'motion_losses' in N.last_error()
    assert lib.a2m_mse_loss_f32(p, p, 0, p, None, None, p, big, None) == EINVAL
    assert lib.a2m_diff_time_f32(p, 2, 1, 8, p, None) == EINVAL
    assert lib.a2m_diff_time_bwd_f32(p, 2, 1, 8, p, 0, None) == EINVAL
    assert lib.a2m_adam_f32(p, p, p, p, 16, 0.05, 0.9, 0.999, 1e-8, 0.0, 0, None) == EINVAL
    src = (ctypes.c_void_p * 1)(p.value)
    off = (ctypes.c_int64 * 1)(0)
    for n, o in ((-1, 0), (4, -4)):
        off[0] = o
        assert lib.a2m_gather_segments_f32(src, off, (ctypes.c_int64 * 1)(n), 1, p, None) == EINVAL
        assert 'segment 0' in N.last_error()
    off[0] = 0
    assert lib.a2m_gather_segments_f32((ctypes.c_void_p * 1)(None), off, (ctypes.c_int64 * 1)(4), 1, p, None) == EINVAL
    assert lib.a2m_window_gather_f32(p, 100, 4, p, 1, 8, 1, p, None, p, None) == EINVAL
    assert lib.a2m_window_gather_f32(p, 100, 4, p, 1, 8, 1, None, p, p, None) == EINVAL
    assert lib.a2m_pck_f32(p, p, 2, 0, 0.2, p, None) == EINVAL
    assert lib.a2m_pose_moments_f32(p, 0, 1, p, None) == EINVAL
    assert lib.a2m_pose_losses_w_f32(p, 104, 104, p, 104, 104, 0, 4, 0.7, 0.3, p, p, big, None) == EINVAL
    assert lib.a2m_pose_losses_w_bwd_f32(p, 104, 104, p, 104, 104, 2, 0, 0.7, 0.3, p, p, p, big, None) == EINVAL
    for fn in (lib.a2m_pose_normalize_f32, lib.a2m_pose_denormalize_f32):
        assert fn(None, 3, p, p, p, None) == EINVAL
        assert fn(p, -1, p, p, p, None) == EINVAL
    assert lib.a2m_pck_f32(None, p, 2, 52, 0.2, p, None) == EINVAL
    assert lib.a2m_window_gather_f32(p, 100, 4, None, 1, 8, 1, None, None, p, None) == EINVAL


def test_empty_inputs_are_no_ops_with_null_pointers(abi):
    """An empty tensor has a null data pointer: nothing to read, nothing launched, A2M_OK."""
    N, p, _ = abi
    lib = N.lib
    assert lib.a2m_pose_normalize_f32(None, 0, p, p, None, None) == 0
    assert lib.a2m_pose_denormalize_f32(None, 0, p, p, None, None) == 0
    assert lib.a2m_pck_f32(None, None, 0, 52, 0.2, None, None) == 0
    assert lib.a2m_window_gather_f32(p, 100, 4, None, 0, 8, 1, None, None, None, None) == 0
    assert lib.a2m_gather_segments_f32((ctypes.c_void_p * 2)(None, None), (ctypes.c_int64 * 2)(0, 7),
                                       (ctypes.c_int64 * 2)(0, 0), 2, p, None) == 0
    assert lib.a2m_gather_segments_f32(None, None, None, 0, None, None) == 0
    assert lib.a2m_adam_f32(p, p, p, p, 0, 0.05, 0.9, 0.999, 1e-8, 0.0, 1, None) == 0


@pytest.mark.parametrize('entry', ['pose_losses', 'motion_losses', 'mse'])
def test_entry_points_report_a_workspace_one_byte_short(abi, entry):
    N, p, _ = abi
    lib = N.lib
    B, T, n = 3, 37, 65537
    call, need = {
        'pose_losses': (lambda ws: lib.a2m_pose_losses_w_f32(p, 104 * T, 104, p, 104 * T, 104, B, T, 0.7, 0.3, p, p, ws,
                                                             None), 4 * B * 3 * 104),
        'motion_losses': (lambda ws: lib.a2m_motion_losses_f32(p, p, B, T, 104, p, None, None, p, ws, None), 12 * B),
        'mse': (lambda ws: lib.a2m_mse_loss_f32(p, p, n, p, None, None, p, ws, None), 4 * 256),
    }[entry]
    assert call(need - 1) == N.A2M_EWS
    assert f'< {need}' in N.last_error(), N.last_error()
    with pytest.raises(N.WorkspaceTooSmall):
        N.check(N.A2M_EWS)
