"""csrc/losses.hip, csrc/train_loss.hip and csrc/evaluation.hip against float64 at edge shapes: the
pose and motion losses and their gradients, MSE, pos_to_motion and its adjoint, the bilinear
resample and its adjoint, Adam in both forms, the gradient segment gather, pose moments,
normalise / denormalise, PCK and the window gather.

References: torch-CPU float64 autograd of oracle.model's losses, F.mse_loss and F.interpolate, and
tests/loss_ref.py (float64 numpy, proved against torch float64 by tests/test_loss_ref_cpu.py) for
Adam, the moments and every self-check.  Pose inputs come from loss_ref.chain_pose.

Tolerances (none is tuned to the kernels):
  gradient tensors, interp   rel_err <= 8 x the rel_err torch-CPU float32 makes on the same inputs
  y, Adam's p, m, v          against the same float64 reference (summation order, FMA contraction)
  scalar losses              |err| <= 8 x E32 x |value|, E32 the largest relative error torch-CPU
                             float32 makes on that loss over all of this module's cases of it (one
                             scalar's float32 error is a lottery, down to 1e-9 here), computed when
                             the module is collected.  A weighted angle loss h hand + b body is
                             bounded by the sum of its parts' bounds, 8 (h E32_hand hand + b E32_body
                             body); MSE pools its 20 cases.
  bitwise (np.array_equal)   diff_time, diff_time_bwd (also accumulating), pose_normalize,
                             pose_denormalize, window_gather, gather_segments, adam_dev against
                             adam, a prefilled dgen against base + grad, pck against a float64
                             restatement on the same float32 inputs: fixed sequences of correctly
                             rounded operations with no multiply-add to contract
  pose_moments               |err| <= 1e-12 (|value| + mean |terms|): float64 sums of float32 data
  adjoint identity           <interp(x), g> = <x, interp_bwd(g)> in float64 to 1e-5 relative
Input conditions (checked on the CPU by tests/test_loss_ref_cpu.py through cases()): every float64
angle of a pose case is at least 1e-5 rad from the kinks of its loss (0 for hand triples, -pi/2 for
body triples) and from the +-pi wrap, and the last hand and the last body triple of the last frame
of the last clip are active, so that the self-check has a term to lose; the first seed from 100
upwards that meets this is used.  Every |motion difference| of a motion case is at least 1e-5 (the
L1 gradient is a sign).  The degenerate cases put exact zeros there on purpose, in small integers
that float32 holds exactly; torch gives zero gradient through atan2(0, 0), relu at 0, a zero norm
and sign(0), and so do the kernels.

Sensitivity self-check (CPU, every case that sums): the float64 reference recomputed with the last
term left out -- the last frame of the last clip and the last bone, triple, feature, element or time
step -- must move the bounded quantity by more than 4 x its tolerance.  In the degenerate cases,
whose last terms are zero by construction, the last non-zero term is left out instead.  Terms over
no frames (motion at T <= 3) have nothing to lose.

Adam's hyperparameters are taken as the C entry points hold them, in float32, by the reference and
by torch alike: float32(0.999) leaves 1 - beta2 1.3e-5 from 0.001, which is the caller's choice of
beta2 and no error of the kernel.

Seen on an MI355X (every comparison prints an ERR line; run with -s): the largest kernel error /
torch-float32 error (bound 8; for a scalar loss the torch error is its E32) and the smallest
self-check margin, reference shift / tolerance (must exceed 4).  E32: bone 2.5e-7, hand 8.3e-8,
body 1.9e-7, L1 7.2e-8, smoothness 6.4e-8, jerk 1.2e-7, mse 8.8e-8.

  part                                  kernel / torch32              smallest margin
  1  pose forward, 7 shapes x 3 weights 1.49 (bone, T 100)            14 (angle, B 3 T 16)
  1  pose backward, 49 cases            1.84 (bone alone, B 1 T 1)    1389
  1  real = NULL                        0.33 scalar, 1.00 dgen        314
  1  strided operands                   0.33 scalar, 1.00 dgen        584
  1  degenerate inputs                  1.89 (bone), 0.96 dgen        697
  2  motion terms, 10 shapes            0.91 (smoothness, T 64)       24 (jerk, T 65)
  2  motion gradient                    1.57 (B 1 T 5 Fd 3)           1279
  2  one gradient at a time             0.90 scalar, 1.00 dfake       24
  2  real = NULL                        0.44 scalar, 1.14 dfake       24
  2  degenerate clips                   0.64 scalar, 0.89 dfake       12394
  3  mse, 20 cases                      1.00 loss, 1.00 dpred         97 (n 65537)
  4  interp forward and adjoint         1.33 (y, H 1), 1.00 dx        46836
  4  <interp(x), g> - <x, interp_bwd(g)>  1.6e-8 relative (bound 1e-5)  -
  5  adam, three steps                  7.48 (v3 at n = 1: torch's    -
                                        own error there is 8.5e-9, a
                                        seventh of an ulp); 2.03 at n > 1
  6  pose moments                       0.002 of the 1e-12 bound      105880
Every bitwise comparison holds.  The module found two bugs, both fixed with it:
  pose_denormalize fused x * std + mean into one multiply-add: the build's -ffp-contract=fast
    contracts in the back end, through __fmul_rn / __fadd_rn too, so the result was one rounding
    where the header promises torch's two (an ulp off in places, and a normalised neck,
    (0 - mean) / std, did not come back to 0).  An empty asm between product and sum keeps them apart.
  empty inputs: an empty tensor's data pointer is NULL, which pose_normalize, pose_denormalize,
    pck, window_gather (n = 0) and a zero-length gather segment refused as A2M_EINVAL before their
    own n = 0 early return.  They now accept NULL data where there is nothing to read.
"""
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import loss_ref as R
from conftest import rel_err
from oracle import model as OM

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32

SEED_BASE = 100
POSE_SHAPES = [(1, 1), (2, 15), (3, 16), (2, 17), (3, 37), (2, 64), (1, 100)]
POSE_WEIGHTS = [(0.7, 0.3), (1.0, 0.0), (0.0, 1.0)]
GRAD_OUTS = [(1.0, 0.0), (0.0, 1.0), (0.7, 1.3)]
DEGEN_SHAPE = (2, 17)
STRIDED_SHAPE = (3, 37)
MOTION_SHAPES = [(2, 2, 104), (2, 3, 104), (2, 4, 104), (3, 9, 104), (2, 64, 104), (2, 65, 104), (1, 512, 6),
                 (2, 33, 7), (1, 5, 1), (1, 5, 3)]
MOTION_GTERMS = (0.8, 1.1, 1.3)
MOTION_DEGEN = (3, 9, 8)
MSE_N = [1, 255, 256, 257, 65537]
MSE_GL = 0.37
DIFF_SHAPES = [(1, 2, 1), (3, 9, 104), (2, 64, 7), (41, 250, 104)]
INTERP_SHAPES = [(8, 15, 64), (8, 16, 64), (8, 1, 64), (8, 2, 5), (64, 3, 8), (1, 4, 7), (5, 7, 5), (3, 5, 100)]
ADAM_N = [1, 255, 4099, 2097152 + 77]
ADAM_HP = dict(lr=0.05, b1=0.9, b2=0.999, eps=1e-8)
GATHER_COUNTS = [1, 48, 49, 97]
GATHER_LENGTHS = [0, 1, 3, 4, 5, 1023, 1025, 65541]
MOMENT_FRAMES = [1, 7, 8, 9, 1003]
NORM_FRAMES = [0, 1, 3, 10083]
PCK_SHAPES = [(0, 52), (1, 1), (3, 52), (4, 63), (5, 64), (9, 65), (2, 130)]
WINDOWS = [(64, 1), (64, 4), (10, 3), (1, 1)]
WINDOW_C = [1, 104, 128]
WINDOW_N = [0, 1, 7, 130]
LAST = (-1, -1, -1)


def _f32(v):
    """A Python float as the kernels hold it."""
    return float(F32(v))


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _record(part, name, q, kernel, torch32, margin=None):
    """One line per comparison (shown with -s): the figures the module docstring tabulates."""
    ratio = kernel / torch32 if torch32 > 0 else (0.0 if kernel == 0 else float('inf'))
    print(f'ERR part={part} case={name} q={q} kernel={kernel:.3e} torch32={torch32:.3e} ratio={ratio:.3f}'
          + ('' if margin is None else f' margin={margin:.1f}'))


def check_scalar(part, name, q, got, ref, tol, shifts, fails):
    """|got - ref| <= tol, and every shift of the reference that loses a term exceeds 4 tol."""
    err = abs(float(got) - ref)
    margin = min(s / max(tol, 1e-300) for s in shifts) if shifts else None
    scale = max(abs(ref), 1e-300)
    _record(part, name, q, err / scale, tol / 8.0 / scale, margin)
    if margin is not None and not margin > 4.0:
        fails.append(f'{q}: self-check margin {margin:.2f} <= 4')
    if not (np.isfinite(got) and err <= tol):
        fails.append(f'{q}: |{float(got)!r} - {ref!r}| = {err:.3e} > {tol:.3e}')


def check_tensor(part, name, q, got, ref, r32, sens, fails):
    """rel_err(got) <= 8 rel_err(torch float32); `sens`: references that lost a term."""
    got = np.asarray(got, dtype=np.float64)
    e_k, e_t = rel_err(got, ref), rel_err(r32, ref)
    tol = 8.0 * e_t
    margin = min(rel_err(s, ref) / max(tol, 1e-300) for s in sens) if sens else None
    _record(part, name, q, e_k, e_t, margin)
    if margin is not None and not margin > 4.0:
        fails.append(f'{q}: self-check margin {margin:.2f} <= 4')
    if not (np.isfinite(got).all() and e_k <= tol):
        fails.append(f'{q}: rel_err {e_k:.3e} > 8 x torch float32 {e_t:.3e}')


def last_nonzero(terms):
    """The index of the last non-zero term (the degenerate cases' self-check)."""
    nz = np.argwhere(np.asarray(terms) != 0)
    assert len(nz), 'no non-zero term'
    return tuple(int(i) for i in nz[-1])


# ------------------------------------------------------------------------------ pose: inputs, references
def pose_ok(gen):
    return (min(R.kink_distance(gen, 'hand'), R.kink_distance(gen, 'body')) >= 1e-5
            and R.angle_terms(gen, 'hand')[LAST] > 0 and R.angle_terms(gen, 'body')[LAST] > 0)


@functools.lru_cache(maxsize=None)
def pose_inputs(B, T):
    """(seed, gen, real): the first seed from SEED_BASE upwards that meets the input condition."""
    for seed in range(SEED_BASE, SEED_BASE + 64):
        gen = R.chain_pose(B, T, seed)
        if pose_ok(gen):
            return seed, gen, R.chain_pose(B, T, seed + 1000)
    raise AssertionError('no seed meets the input condition')


@functools.lru_cache(maxsize=None)
def degenerate_pose():
    """(gen, real) at DEGEN_SHAPE.  Frames (0, 3) and (1, 16) of gen hold small integers: a chain
    of (+-1, +-2) / (+-2, +-1) steps whose every triple turns by atan2(4, -3); in the first, hand
    joint 14 sits on its parent 13 (a bone of length 0, v = 0); in the second, joints 16, 17, 18
    lie on a line with u = (1, 0), v = (2, 0), an angle of exactly 0."""
    B, T = DEGEN_SHAPE
    _, gen, real = pose_inputs(B, T)
    gen = gen.copy().reshape(B, T, 52, 2)
    cyc = [(2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)]
    frame = np.zeros((52, 2), dtype=F32)
    for j in range(1, 52):
        frame[j] = frame[R.PARENTS[j]] + F32(cyc[(3 * j) % 8])
    a, b = frame.copy(), frame.copy()
    a[14] = a[13]
    b[17] = b[16] + F32((1, 0))
    b[18] = b[17] + F32((2, 0))
    gen[0, 3], gen[1, 16] = a, b
    return gen.reshape(B, T, 104), real


def pose_torch(gen, real, hw, bw, go, dtype):
    """torch-CPU autograd of oracle.model's losses: the three values and d (go . (bone, angle)) / d gen."""
    g = _t(gen, dtype).requires_grad_(True)
    hand, body = OM.hand_angle_loss(g), OM.body_angle_loss(g)
    bone = OM.bone_length_loss(_t(real, dtype), g) if real is not None else torch.zeros((), dtype=dtype)
    (_f32(go[0]) * bone + _f32(go[1]) * (_f32(hw) * hand + _f32(bw) * body)).backward()
    return dict(bone=bone.item(), hand=hand.item(), body=body.item(), dgen=g.grad.numpy())


def pose_manual(gen, real, hw, bw, go, omit_part=None, omit=LAST):
    """The same gradient by loss_ref's formulas, optionally with one term of one part left out."""
    def om(part):
        return omit if omit_part == part else None
    out = _f32(go[1]) * (_f32(hw) * R.angle_grad(gen, 'hand', om('hand')) + _f32(bw) * R.angle_grad(gen, 'body', om('body')))
    if real is not None:
        out = out + _f32(go[0]) * R.bone_grad(gen, real, om('bone'))
    return out


def _pose_scalar_cases():
    return [pose_inputs(B, T)[1:] for B, T in POSE_SHAPES] + [degenerate_pose()]


def _rel(a, b):
    return abs(a - b) / abs(b)


@functools.lru_cache(maxsize=None)
def e32():
    """loss -> the largest relative error of torch-CPU float32 over this module's cases of it."""
    out = {}
    one = (1.0, 1.0)
    for gen, real in _pose_scalar_cases():
        r64, r32 = pose_torch(gen, real, 1, 1, one, torch.float64), pose_torch(gen, real, 1, 1, one, torch.float32)
        for k in ('bone', 'hand', 'body'):
            out[k] = max(out.get(k, 0.0), _rel(r32[k], r64[k]))
    for shape in MOTION_SHAPES:
        fake, real = motion_inputs(*shape)
        t64, t32 = motion_torch(fake, real, None, torch.float64)[0], motion_torch(fake, real, None, torch.float32)[0]
        for k, a, b in zip(('l1', 'smooth', 'jerk'), t32, t64):
            if b != 0:
                out[k] = max(out.get(k, 0.0), _rel(a, b))
    for n in MSE_N:
        for variant in range(4):
            pred, target = mse_inputs(n, variant)
            v64 = TF.mse_loss(_t(pred, torch.float64), _t(target, torch.float64)).item()
            v32 = TF.mse_loss(_t(pred, torch.float32), _t(target, torch.float32)).item()
            out['mse'] = max(out.get('mse', 0.0), _rel(v32, v64))
    return out


def angle_tol(hw, bw, hand, body):
    E = e32()
    return 8.0 * (_f32(hw) * E['hand'] * hand + _f32(bw) * E['body'] * body)


def prep_pose_forward(gen, real, hw, bw, omits=None):
    """Reference values, tolerances and self-check shifts of one forward case (CPU only)."""
    omits = omits or dict(bone=LAST, hand=LAST, body=LAST)
    r = pose_torch(gen, real, hw, bw, (1.0, 1.0), torch.float64)
    c = types.SimpleNamespace(**r)
    for k, v in (('bone', R.bone_loss(gen, real) if real is not None else 0.0),
                 ('hand', R.angle_loss(gen, 'hand')), ('body', R.angle_loss(gen, 'body'))):
        assert abs(v - r[k]) <= 1e-11 * abs(r[k]), k        # the formulas the self-check perturbs
    c.angle = _f32(hw) * c.hand + _f32(bw) * c.body
    c.bone_tol = 8.0 * e32()['bone'] * c.bone
    c.angle_tol = angle_tol(hw, bw, c.hand, c.body)
    c.bone_shift = [abs(R.bone_loss(gen, real, omits['bone']) - c.bone)] if real is not None else []
    c.angle_shift = [_f32(w) * abs(R.angle_loss(gen, part, omits[part]) - r[part])
                     for part, w in (('hand', hw), ('body', bw)) if w > 0]
    return c


def prep_pose_backward(gen, real, hw, bw, go, omits=None):
    omits = omits or dict(bone=LAST, hand=LAST, body=LAST)
    ref = pose_torch(gen, real, hw, bw, go, torch.float64)['dgen']
    r32 = pose_torch(gen, real, hw, bw, go, torch.float32)['dgen']
    assert rel_err(pose_manual(gen, real, hw, bw, go), ref) < 1e-11
    parts = [p for p, w in (('bone', go[0] if real is not None else 0), ('hand', go[1] * hw), ('body', go[1] * bw)) if w > 0]
    sens = [pose_manual(gen, real, hw, bw, go, p, omits[p]) for p in parts]
    return ref, r32, sens


def run_pose_forward(gen_d, real_d, hw, bw):
    from a2m import functional as F
    return _np(F.pose_losses(gen_d, real_d, (hw, bw)))


def run_pose_backward(gen_d, real_d, hw, bw, go, dgen=None):
    from a2m import functional as F
    B, T = gen_d.shape[:2]
    dgen = torch.zeros(B, T, 104, device=DEV) if dgen is None else dgen
    F.pose_losses_bwd(gen_d, real_d, torch.tensor(go, dtype=torch.float32, device=DEV), dgen, (hw, bw))
    return _np(dgen)


def _backward_cases():
    """(weights, grad_out) pairs: the bone gradient alone once, the angle gradient alone and both
    together under every weighting."""
    return [(POSE_WEIGHTS[0], GRAD_OUTS[0])] + [(w, go) for go in GRAD_OUTS[1:] for w in POSE_WEIGHTS]


def _pid(B, T):
    return f'B{B}-T{T}'


# ------------------------------------------------------------------------------ pose: tests
@pytest.mark.parametrize('hw,bw', POSE_WEIGHTS, ids=lambda w: None)
@pytest.mark.parametrize('B,T', POSE_SHAPES, ids=[_pid(*s) for s in POSE_SHAPES])
def test_pose_losses_forward(B, T, hw, bw, request):
    """T = 15, 17, 37, 100 run the min(16, T - t0) chunk tails; T = 1 a chunk of one frame."""
    _, gen, real = pose_inputs(B, T)
    c = prep_pose_forward(gen, real, hw, bw)
    out = run_pose_forward(_t(gen, torch.float32).to(DEV), _t(real, torch.float32).to(DEV), hw, bw)
    fails, name = [], request.node.callspec.id
    check_scalar('1-pose-fwd', name, 'bone', out[0], c.bone, c.bone_tol, c.bone_shift, fails)
    check_scalar('1-pose-fwd', name, 'angle', out[1], c.angle, c.angle_tol, c.angle_shift, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('w,go', _backward_cases(), ids=lambda v: None)
@pytest.mark.parametrize('B,T', POSE_SHAPES, ids=[_pid(*s) for s in POSE_SHAPES])
def test_pose_losses_backward(B, T, w, go, request):
    """T = 100 is the mean-bone-length loop's second lane trip with a ragged tail."""
    _, gen, real = pose_inputs(B, T)
    ref, r32, sens = prep_pose_backward(gen, real, w[0], w[1], go)
    got = run_pose_backward(_t(gen, torch.float32).to(DEV), _t(real, torch.float32).to(DEV), w[0], w[1], go)
    fails, name = [], request.node.callspec.id
    check_tensor('1-pose-bwd', name, 'dgen', got, ref, r32, sens, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('B,T', [(2, 17), (3, 37)], ids=[_pid(2, 17), _pid(3, 37)])
def test_pose_losses_without_real(B, T, request):
    """real = NULL: the bone loss is exactly 0 and grad_out[0] moves nothing."""
    _, gen, _ = pose_inputs(B, T)
    hw, bw = POSE_WEIGHTS[0]
    c = prep_pose_forward(gen, None, hw, bw)
    gen_d = _t(gen, torch.float32).to(DEV)
    out = run_pose_forward(gen_d, None, hw, bw)
    fails, name = [], request.node.callspec.id
    assert out[0] == 0.0
    check_scalar('1-pose-noreal', name, 'angle', out[1], c.angle, c.angle_tol, c.angle_shift, fails)
    go = GRAD_OUTS[2]
    ref, r32, sens = prep_pose_backward(gen, None, hw, bw, go)
    got = run_pose_backward(gen_d, None, hw, bw, go)
    check_tensor('1-pose-noreal', name, 'dgen', got, ref, r32, sens, fails)
    assert np.array_equal(got, run_pose_backward(gen_d, None, hw, bw, (123.0, go[1])))
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_pose_losses_strided_operands(request):
    """gen a [:, :, :104] view of [B][T][130], real a view of [B + 1][T + 3][104]."""
    B, T = STRIDED_SHAPE
    _, gen, real = pose_inputs(B, T)
    hw, bw = POSE_WEIGHTS[0]
    gbuf = torch.full((B, T, 130), 55.5)
    gbuf[:, :, :104] = _t(gen, torch.float32)
    rbuf = torch.full((B + 1, T + 3, 104), -44.5)
    rbuf[:B, :T] = _t(real, torch.float32)
    gen_d, real_d = gbuf.to(DEV)[:, :, :104], rbuf.to(DEV)[:B, :T]
    assert not gen_d.is_contiguous() and not real_d.is_contiguous()
    c = prep_pose_forward(gen, real, hw, bw)
    out = run_pose_forward(gen_d, real_d, hw, bw)
    fails, name = [], 'strided-' + _pid(B, T)
    check_scalar('1-pose-strided', name, 'bone', out[0], c.bone, c.bone_tol, c.bone_shift, fails)
    check_scalar('1-pose-strided', name, 'angle', out[1], c.angle, c.angle_tol, c.angle_shift, fails)
    go = GRAD_OUTS[2]
    ref, r32, sens = prep_pose_backward(gen, real, hw, bw, go)
    got = run_pose_backward(gen_d, real_d, hw, bw, go)
    check_tensor('1-pose-strided', name, 'dgen', got, ref, r32, sens, fails)
    # the same bits as from contiguous operands: the strides only move the loads
    same = run_pose_backward(_t(gen, torch.float32).to(DEV), _t(real, torch.float32).to(DEV), hw, bw, go)
    assert np.array_equal(got, same)
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_pose_losses_backward_adds_into_dgen():
    """dgen is added to: base + grad in one float32 add, bitwise."""
    B, T = (2, 17)
    _, gen, real = pose_inputs(B, T)
    hw, bw = POSE_WEIGHTS[0]
    go = GRAD_OUTS[2]
    gen_d, real_d = _t(gen, torch.float32).to(DEV), _t(real, torch.float32).to(DEV)
    grad = run_pose_backward(gen_d, real_d, hw, bw, go)
    base = torch.randn(B, T, 104, generator=torch.Generator().manual_seed(5)) * 1e-3
    got = run_pose_backward(gen_d, real_d, hw, bw, go, dgen=base.to(DEV))
    assert grad.any() and np.array_equal(got, base.numpy() + grad)


def test_pose_losses_default_weight_entries():
    """a2m_pose_losses_f32 and a2m_pose_losses_bwd_f32 are the weighted entries at (0.7, 0.3), bitwise."""
    from a2m import _native as N
    from a2m import functional as F
    B, T = (2, 17)
    _, gen, real = pose_inputs(B, T)
    gen_d, real_d = _t(gen, torch.float32).to(DEV), _t(real, torch.float32).to(DEV)
    go = GRAD_OUTS[2]
    out = torch.empty(2, device=DEV)
    F._with_ws(DEV, lambda wp, wn: N.lib.a2m_pose_losses_f32(
        F._p(gen_d), gen_d.stride(0), gen_d.stride(1), F._p(real_d), real_d.stride(0), real_d.stride(1), B, T,
        F._p(out), wp, wn, F._stream()))
    assert np.array_equal(_np(out), run_pose_forward(gen_d, real_d, 0.7, 0.3))
    dgen, go_d = torch.zeros(B, T, 104, device=DEV), torch.tensor(go, dtype=torch.float32, device=DEV)
    F._with_ws(DEV, lambda wp, wn: N.lib.a2m_pose_losses_bwd_f32(
        F._p(gen_d), gen_d.stride(0), gen_d.stride(1), F._p(real_d), real_d.stride(0), real_d.stride(1), B, T,
        F._p(go_d), F._p(dgen), wp, wn, F._stream()))
    assert dgen.any() and np.array_equal(_np(dgen), run_pose_backward(gen_d, real_d, 0.7, 0.3, go))


def degenerate_pose_omits():
    gen, real = degenerate_pose()
    return dict(bone=LAST, hand=last_nonzero(R.angle_terms(gen, 'hand')), body=last_nonzero(R.angle_terms(gen, 'body')))


@pytest.mark.parametrize('w,go', [(POSE_WEIGHTS[0], go) for go in GRAD_OUTS], ids=lambda v: None)
def test_pose_losses_degenerate_inputs(w, go, request):
    """A bone of length 0 (v = 0: atan2(0, 0)) and a collinear triple (an angle of exactly 0, on the
    hand loss's kink): finite, zero gradient through them as torch gives, within the usual bounds."""
    gen, real = degenerate_pose()
    B, T = DEGEN_SHAPE
    assert R.bone_lengths(gen)[0, 3, 13] == 0 and R.angles(gen, 'hand')[0, 3, 2] == 0    # bone 13 -> 14, triple (2, 3, 4)
    assert R.angles(gen, 'hand')[1, 16, 5] == 0                                        # triple (6, 7, 8)
    omits = degenerate_pose_omits()
    c = prep_pose_forward(gen, real, w[0], w[1], omits)
    gen_d, real_d = _t(gen, torch.float32).to(DEV), _t(real, torch.float32).to(DEV)
    out = run_pose_forward(gen_d, real_d, w[0], w[1])
    fails, name = [], 'degenerate-' + request.node.callspec.id
    check_scalar('1-pose-degenerate', name, 'bone', out[0], c.bone, c.bone_tol, c.bone_shift, fails)
    check_scalar('1-pose-degenerate', name, 'angle', out[1], c.angle, c.angle_tol, c.angle_shift, fails)
    ref, r32, sens = prep_pose_backward(gen, real, w[0], w[1], go, omits)
    got = run_pose_backward(gen_d, real_d, w[0], w[1], go)
    check_tensor('1-pose-degenerate', name, 'dgen', got, ref, r32, sens, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


# ------------------------------------------------------------------------------ motion terms
@functools.lru_cache(maxsize=None)
def motion_inputs(B, T, Fd):
    """float32 (fake, real) [B][T][Fd]; the last element of fake carries a sentinel, which reaches
    the last term of all three sums; redrawn while a motion difference lies within 1e-5 of 0 or one
    of those last terms is below 3 (the sentinel met a draw that cancels it)."""
    for bump in range(64):
        rng = np.random.default_rng(1000 * T + 10 * Fd + B + 7919 * bump)
        fake = rng.standard_normal((B, T, Fd)).astype(F32)
        real = rng.standard_normal((B, T, Fd)).astype(F32)
        fake[-1, -1, -1] += F32(4.0)
        fm = np.diff(fake.astype(np.float64), axis=1)
        d = fm - np.diff(real.astype(np.float64), axis=1)
        last = [abs(a[LAST]) for a in (d, np.diff(fm, 1, axis=1), np.diff(fm, 2, axis=1)) if a.shape[1]]
        if np.abs(d).min() >= 1e-5 and min(last) >= 3.0:
            return fake, real
    raise AssertionError('no draw without a motion difference on the L1 kink')


@functools.lru_cache(maxsize=None)
def degenerate_motion():
    """MOTION_DEGEN in small integers: clip 0 has fake = real (every L1 sign is 0), clip 1 is
    a + b t (every acceleration norm is exactly 0), clip 2 is c t^2 (every jerk norm is exactly 0)."""
    B, T, Fd = MOTION_DEGEN
    rng = np.random.default_rng(77)
    t = np.arange(T, dtype=np.float64)[:, None]
    real = rng.integers(-4, 5, (B, T, Fd)).astype(np.float64)
    fake = real.copy()
    fake[1] = rng.integers(-3, 4, (1, Fd)) + rng.integers(-3, 4, (1, Fd)) * t
    fake[2] = rng.integers(1, 4, (1, Fd)) * t * t
    real[1:] += 0.5 * t     # no motion difference of clips 1 and 2 is zero: integers against halves
    return fake.astype(F32), real.astype(F32)


def motion_torch(fake, real, gterms, dtype):
    """((l1, smooth, jerk), dfake): oracle.model.motion_terms under torch-CPU autograd; a term over
    no frames (an empty mean, NaN in torch) is 0 and has no gradient."""
    f = _t(fake, dtype).requires_grad_(gterms is not None)
    r = _t(real if real is not None else fake, dtype)
    terms = list(OM.motion_terms(r, f))
    T = fake.shape[1]
    live = [real is not None, T > 2, T > 3]
    vals = tuple(t.item() if ok else 0.0 for t, ok in zip(terms, live))
    if gterms is None:
        return vals, None
    total = sum(_f32(g) * t for g, t, ok in zip(gterms, terms, live) if ok and g != 0)
    if not torch.is_tensor(total):
        return vals, np.zeros(fake.shape)
    total.backward()
    return vals, f.grad.numpy()


def prep_motion(fake, real, gterms, omit=LAST, omits=None):
    T = fake.shape[1]
    E = e32()
    omits = omits or dict(l1=omit, smooth=omit, jerk=omit)
    vals, ref = motion_torch(fake, real, gterms, torch.float64)
    _, r32 = motion_torch(fake, real, gterms, torch.float32)
    man = R.motion_terms(fake, real)
    live = dict(l1=real is not None, smooth=T > 2, jerk=T > 3)
    c = types.SimpleNamespace(vals=vals, ref=ref, r32=r32, tols=[], shifts=[], sens=[])
    for i, k in enumerate(('l1', 'smooth', 'jerk')):
        assert abs(man[i] - vals[i]) <= 1e-11 * abs(vals[i]), k
        c.tols.append(8.0 * E[k] * vals[i])
        c.shifts.append([abs(R.motion_terms(fake, real, {k: omits[k]})[i] - vals[i])] if live[k] else [])
    if gterms is not None:
        g = [_f32(v) for v in gterms]
        assert rel_err(R.motion_grad(fake, real, g), ref) < 1e-11
        for i, k in enumerate(('l1', 'smooth', 'jerk')):
            if live[k] and g[i] != 0:
                one = [v if j == i else 0.0 for j, v in enumerate(g)]
                # the term's own gradient with its last element lost, the other terms' whole
                c.sens.append(ref - R.motion_grad(fake, real, one) + R.motion_grad(fake, real, one, {k: omits[k]}))
    return c


def run_motion(fake, real, gterms):
    from a2m import functional as F
    gt = None if gterms is None else torch.tensor(gterms, dtype=torch.float32, device=DEV)
    terms, dfake = F.motion_losses(_t(fake, torch.float32).to(DEV),
                                   None if real is None else _t(real, torch.float32).to(DEV), gt)
    return _np(terms), _np(dfake)


def check_motion(part, name, c, terms, dfake):
    fails = []
    for i, k in enumerate(('l1', 'smooth', 'jerk')):
        if c.shifts[i]:
            check_scalar(part, name, k, terms[i], c.vals[i], c.tols[i], c.shifts[i], fails)
        else:
            assert terms[i] == 0.0, f'{k} over no frames is 0'
    if c.ref is not None:
        assert dfake.shape == c.ref.shape
        check_tensor(part, name, 'dfake', dfake, c.ref, c.r32, c.sens, fails)
    else:
        assert dfake is None
    assert not fails, f'{name}: ' + '; '.join(fails)


def _mid(s):
    return 'B%d-T%d-F%d' % s


@pytest.mark.parametrize('grad', [False, True], ids=['terms', 'grad'])
@pytest.mark.parametrize('shape', MOTION_SHAPES, ids=_mid)
def test_motion_losses(shape, grad, request):
    """T = 2, 3, 4: terms over no frames and over one; T = 65: the quad loop's second trip; T = 512:
    the LDS arrays' size; Fd = 1, 3, 6, 7: quads with idle lanes and ragged feature tails."""
    fake, real = motion_inputs(*shape)
    c = prep_motion(fake, real, MOTION_GTERMS if grad else None)
    terms, dfake = run_motion(fake, real, MOTION_GTERMS if grad else None)
    if shape[1] == 2 and grad:
        assert np.abs(c.ref).max() > 0            # the L1 gradient alone
    check_motion('2-motion', request.node.callspec.id, c, terms, dfake)


@pytest.mark.parametrize('gterms', [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)], ids=['l1', 'smooth', 'jerk'])
@pytest.mark.parametrize('shape', [(2, 65, 104), (2, 33, 7)], ids=_mid)
def test_motion_losses_one_gradient_at_a_time(shape, gterms, request):
    """Each term's gradient alone, so that the max-normalised error of one cannot hide another's."""
    fake, real = motion_inputs(*shape)
    c = prep_motion(fake, real, gterms)
    terms, dfake = run_motion(fake, real, gterms)
    check_motion('2-motion-one', request.node.callspec.id, c, terms, dfake)


@pytest.mark.parametrize('shape', [(2, 2, 104), (2, 3, 104), (2, 65, 104), (2, 33, 7)], ids=_mid)
def test_motion_losses_without_real(shape, request):
    """real = NULL: term 0 is exactly 0 and there is no L1 gradient (none at all at T = 2)."""
    fake, _ = motion_inputs(*shape)
    c = prep_motion(fake, None, MOTION_GTERMS)
    terms, dfake = run_motion(fake, None, MOTION_GTERMS)
    assert terms[0] == 0.0
    if shape[1] == 2:
        assert not dfake.any()
    check_motion('2-motion-noreal', request.node.callspec.id, c, terms, dfake)


def degenerate_motion_omits():
    fake, real = degenerate_motion()
    f = fake.astype(np.float64)
    fm = np.diff(f, axis=1)
    acc = fm[:, 1:] - fm[:, :-1]
    jerk = acc[:, 1:] - acc[:, :-1]
    return dict(l1=last_nonzero(fm - np.diff(real.astype(np.float64), axis=1)), smooth=last_nonzero(acc),
                jerk=last_nonzero(jerk))


def test_motion_losses_degenerate_clips(request):
    """Zero acceleration norms, zero jerk norms and fake = real: finite, and 0 through each as torch."""
    fake, real = degenerate_motion()
    f = fake.astype(np.float64)
    acc = np.diff(f, 2, axis=1)
    assert not acc[1].any() and acc[2].any() and not np.diff(f, 3, axis=1)[2].any() and np.array_equal(fake[0], real[0])
    c = prep_motion(fake, real, MOTION_GTERMS, omits=degenerate_motion_omits())
    terms, dfake = run_motion(fake, real, MOTION_GTERMS)
    check_motion('2-motion-degenerate', 'B3-T9-F8', c, terms, dfake)


# ------------------------------------------------------------------------------ mse
@functools.lru_cache(maxsize=None)
def mse_inputs(n, variant):
    rng = np.random.default_rng(31 * n + variant)
    pred, target = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    pred[-1] = target[-1] + F32(3.0)              # the sentinel the self-check leaves out
    return pred, target


def prep_mse(n, variant, gl):
    pred, target = mse_inputs(n, variant)
    c = types.SimpleNamespace(pred=pred, target=target)
    out = {}
    for dtype in (torch.float64, torch.float32):
        p = _t(pred, dtype).requires_grad_(True)
        loss = TF.mse_loss(p, _t(target, dtype))
        (loss * (1.0 if gl is None else _f32(gl))).backward()
        out[dtype] = (loss.item(), p.grad.numpy())
    c.loss, c.ref = out[torch.float64]
    c.r32 = out[torch.float32][1]
    assert abs(R.mse_loss(pred, target) - c.loss) <= 1e-11 * c.loss
    assert rel_err(R.mse_grad(pred, target, 1.0 if gl is None else _f32(gl)), c.ref) < 1e-11
    c.tol = 8.0 * e32()['mse'] * c.loss
    c.shift = [abs(R.mse_loss(pred, target, -1) - c.loss)]
    return c


@pytest.mark.parametrize('want', [False, True], ids=['loss', 'dpred'])
@pytest.mark.parametrize('gl', [None, MSE_GL], ids=['gl_null', 'gl_dev'])
@pytest.mark.parametrize('n', MSE_N, ids=lambda n: f'n{n}')
def test_mse_loss(n, gl, want, request):
    """n = 65537 is 256 workgroups x 256 threads plus one: the grid-stride loop wraps."""
    from a2m import _native as N
    from a2m import functional as F
    c = prep_mse(n, 2 * (gl is not None) + want, gl)
    pred, target = torch.from_numpy(c.pred).to(DEV), torch.from_numpy(c.target).to(DEV)
    gl_d = None if gl is None else torch.tensor([gl], dtype=torch.float32, device=DEV)
    if gl is None or want:
        loss, d = F.mse_loss(pred, target, gl_d, want_grad=want)
    else:                      # a grad_loss but no dpred: no wrapper asks for that
        loss, d = torch.empty((), device=DEV), None
        F._with_ws(DEV, lambda wp, wn: N.lib.a2m_mse_loss_f32(F._p(pred), F._p(target), n, F._p(loss), F._p(gl_d),
                                                             None, wp, wn, F._stream()))
    assert (d is not None) == want
    fails, name = [], request.node.callspec.id
    check_scalar('3-mse', name, 'loss', loss.item(), c.loss, c.tol, c.shift, fails)
    if want:
        check_tensor('3-mse', name, 'dpred', _np(d), c.ref, c.r32, None, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


# ------------------------------------------------------------------------------ diff_time
@pytest.mark.parametrize('shape', DIFF_SHAPES, ids=_mid)
def test_diff_time_bitwise(shape):
    """(41, 250, 104) is past 4096 x 256 elements: the grid-stride loops wrap."""
    from a2m import functional as F
    B, T, Fd = shape
    g = torch.Generator().manual_seed(B + T + Fd)
    x = torch.randn(B, T, Fd, generator=g)
    y = F.diff_time(x.to(DEV))
    assert np.array_equal(_np(y), torch.diff(x, dim=1).numpy())
    dy = torch.randn(B, T - 1, Fd, generator=g).numpy()
    want = np.zeros((B, T, Fd), dtype=F32)
    want[:, 1:] += dy
    want[:, :-1] -= dy
    assert want.dtype == F32
    got = F.diff_time_bwd(torch.from_numpy(dy).to(DEV))
    assert np.array_equal(_np(got), want)
    base = torch.randn(B, T, Fd, generator=g)
    acc = base.to(DEV)
    F.diff_time_bwd(torch.from_numpy(dy).to(DEV), dx=acc, accumulate=True)
    assert np.array_equal(_np(acc), base.numpy() + want)
    over = torch.full((B, T, Fd), 9.5, device=DEV)
    F.diff_time_bwd(torch.from_numpy(dy).to(DEV), dx=over, accumulate=False)
    assert np.array_equal(_np(over), want)


# ------------------------------------------------------------------------------ interp_time
def _interp_inputs(H, W, T):
    g = torch.Generator().manual_seed(100 * H + 10 * W + T)
    x = torch.randn(2, 3, H, W, generator=g) + 1.0
    dy = torch.randn(2, 3, T, generator=g) + 1.0
    dy[:, :, -1] += 4.0                              # the time step the self-check leaves out
    return x, dy


def interp_torch(x, dy, T, dtype):
    xx = x.to(dtype).clone().requires_grad_(True)
    y = TF.interpolate(xx, size=(T, 1), mode='bilinear', align_corners=False).squeeze(-1)
    y.backward(dy.to(dtype))
    return y.detach().numpy(), xx.grad.numpy()


@pytest.mark.parametrize('H,W,T', INTERP_SHAPES, ids=['H%d-W%d-T%d' % s for s in INTERP_SHAPES])
def test_interp_time_and_adjoint(H, W, T, request):
    """Even W (both middle columns at 0.5), W = 1, downsampling (H > T), H = 1, the identity
    (H = T) and T % 4 != 0 (the forward's scalar path)."""
    from a2m import functional as F
    x, dy = _interp_inputs(H, W, T)
    y64, dx64 = interp_torch(x, dy, T, torch.float64)
    y32, dx32 = interp_torch(x, dy, T, torch.float32)
    assert rel_err(R.interp_time(x.numpy(), T), y64) < 1e-11
    assert rel_err(R.interp_time_bwd(dy.numpy(), H, W), dx64) < 1e-11
    y = _np(F.interp_time(x.to(DEV), T))
    dx = _np(F.interp_time_bwd(dy.to(DEV), H, W))
    fails, name = [], request.node.callspec.id
    check_tensor('4-interp', name, 'y', y, y64, y32, None, fails)
    check_tensor('4-interp', name, 'dx', dx, dx64, dx32, [R.interp_time_bwd(dy.numpy(), H, W, omit=-1)], fails)
    lhs = float((y.astype(np.float64) * dy.double().numpy()).sum())
    rhs = float((x.double().numpy() * dx.astype(np.float64)).sum())
    print(f'ERR part=4-interp case={name} q=adjoint kernel={abs(lhs - rhs) / abs(lhs):.3e} torch32=1e-05')
    if not abs(lhs - rhs) <= 1e-5 * abs(lhs):
        fails.append(f'<interp(x), g> = {lhs!r} but <x, interp_bwd(g)> = {rhs!r}')
    assert not fails, f'{name}: ' + '; '.join(fails)


# ------------------------------------------------------------------------------ adam
@functools.lru_cache(maxsize=None)
def adam_inputs(n):
    g = torch.Generator().manual_seed(n % 9973)
    p = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * s for s in (1.0, 0.3, 2.0)]
    return p, grads


def adam_hp(wd):
    """(lr, beta1, beta2, eps, weight_decay) as the C entry points hold them, in float32: the
    reference and torch take these values (float32(0.999) is 1.3e-5 of 1 - beta2 from 0.999)."""
    return tuple(_f32(v) for v in (ADAM_HP['lr'], ADAM_HP['b1'], ADAM_HP['b2'], ADAM_HP['eps'], wd))


def adam_torch(n, wd, dtype):
    """[(p, m, v) after each of three torch.optim.Adam steps]."""
    p0, grads = adam_inputs(n)
    p = p0.to(dtype).clone().requires_grad_(True)
    lr, b1, b2, eps, wd = adam_hp(wd)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    out = []
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
        st = opt.state[p]
        out.append((p.detach().numpy().copy(), st['exp_avg'].numpy().copy(), st['exp_avg_sq'].numpy().copy()))
    return out


def adam_ref(n, wd):
    p0, grads = adam_inputs(n)
    z = np.zeros(n)
    return R.adam(p0.numpy(), [g.numpy() for g in grads], z, z, *adam_hp(wd))


@pytest.mark.parametrize('wd', [0.0, 0.01], ids=['wd0', 'wd0.01'])
@pytest.mark.parametrize('n', ADAM_N, ids=lambda n: f'n{n}')
def test_adam_three_steps(n, wd, request):
    """n = 2,097,229 is past 8192 workgroups x 256 threads: the grid-stride loop wraps."""
    from a2m import functional as F
    p0, grads = adam_inputs(n)
    ref, r32 = adam_ref(n, wd), adam_torch(n, wd, torch.float32)
    p, m, v = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    fails, name = [], request.node.callspec.id
    for k, g in enumerate(grads):
        F.adam_(p, g.to(DEV), m, v, ADAM_HP['lr'], ADAM_HP['b1'], ADAM_HP['b2'], ADAM_HP['eps'], wd, k + 1)
        if k == 2 or n < 10000:
            for q, got, want, w32 in zip('pmv', (p, m, v), ref[k], r32[k]):
                check_tensor('5-adam', name, f'{q}{k + 1}', _np(got), want, w32, None, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('wd', [0.0, 0.01], ids=['wd0', 'wd0.01'])
@pytest.mark.parametrize('n', [1, 4099, ADAM_N[-1]], ids=lambda n: f'n{n}')
def test_adam_dev_is_bitwise_adam(n, wd):
    """Step and learning rate in device memory: the same bits as the host form at steps 1, 2, 3,
    with the learning rate rewritten between launches 2 and 3."""
    from a2m import functional as F
    p0, grads = adam_inputs(n)
    hp = (ADAM_HP['b1'], ADAM_HP['b2'], ADAM_HP['eps'], wd)
    ph, mh, vh = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    pd, md, vd = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    lr_d = torch.tensor([ADAM_HP['lr']], dtype=torch.float32, device=DEV)
    for k, g in enumerate(grads):
        lr = ADAM_HP['lr'] if k < 2 else 0.0125
        if k == 2:
            lr_d.fill_(lr)
        gd = g.to(DEV)
        F.adam_(ph, gd, mh, vh, lr, *hp, k + 1)
        F.adam_dev_(pd, gd, md, vd, lr_d, *hp, step)
        assert int(step.item()) == k + 1
        for q, a, b in zip('pmv', (pd, md, vd), (ph, mh, vh)):
            assert np.array_equal(_np(a).view(np.uint32), _np(b).view(np.uint32)), f'{q} differs at step {k + 1}'
    assert not torch.equal(pd.cpu(), p0)


def test_adam_dev_advances_the_step_with_no_elements():
    from a2m import _native as N
    from a2m import functional as F
    one = torch.full((1,), 2.5, device=DEV)
    step = torch.full((1,), 6, dtype=torch.int32, device=DEV)
    lr_d = torch.tensor([0.05], dtype=torch.float32, device=DEV)
    N.check(N.lib.a2m_adam_dev_f32(F._p(one), F._p(one), F._p(one), F._p(one), 0, F._p(lr_d), 0.9, 0.999, 1e-8, 0.0,
                                   F._p(step), F._stream()))
    assert int(step.item()) == 7 and one.item() == 2.5


# ------------------------------------------------------------------------------ gather_segments
@pytest.mark.parametrize('count', GATHER_COUNTS, ids=lambda c: f'segments{c}')
def test_gather_segments(count):
    """1, 48, 49 and 97 segments: one launch, a full one, one and two more; lengths around the
    float4 path's tail and past one launch row's 64 x 256 x 4 elements; destinations and sources on
    and off 16-byte alignment (the element path); every byte outside the segments keeps its canary."""
    from a2m import functional as F
    rng = np.random.default_rng(count)
    canary = F32(-7777.25)
    segs, want_parts, cursor = [], [], 0
    aligned = {(a, b): 0 for a in (True, False) for b in (True, False)}
    for i in range(count):
        n = GATHER_LENGTHS[(i + count) % len(GATHER_LENGTHS)]
        combo = (i + i // 8) % 4                     # every length meets all four alignments
        off = cursor + (-cursor) % 4 + combo % 2     # on 16 bytes, or one float past
        src_off = combo // 2                         # the source too
        data = rng.standard_normal(n + src_off).astype(F32)
        buf = torch.from_numpy(data).to(DEV)
        assert buf.numel() == 0 or buf.data_ptr() % 16 == 0
        segs.append((off, buf[src_off:]))
        want_parts.append((off, data[src_off:]))
        if n:
            aligned[(off % 4 == 0, src_off == 0)] += 1
        cursor = off + n + 1
    if count >= 48:
        assert all(aligned.values()), aligned
    total = cursor + 5
    want = np.full(total, canary, dtype=F32)
    for off, d in want_parts:
        want[off:off + d.size] = d
    dst = torch.full((total,), float(canary), device=DEV)
    F.gather_segments_(dst, segs)
    assert np.array_equal(_np(dst).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------ evaluation.hip
def _planar_pose(n, seed, offset=0.0):
    return (np.random.default_rng(seed).standard_normal((n, 104)) * 3.0 + offset).astype(F32)


@pytest.mark.parametrize('necksub', [0, 1], ids=['plain', 'necksub'])
@pytest.mark.parametrize('n', MOMENT_FRAMES, ids=lambda n: f'frames{n}')
def test_pose_moments(n, necksub, request):
    """Frames 7, 8, 9 straddle the 8 frame groups; x + 500 would sink a float32 sum; a second
    call into the same acc adds."""
    from a2m import _native as N
    from a2m import functional as F
    a, b = _planar_pose(n, 10 * n + necksub, 500.0), _planar_pose(9, 10 * n + necksub + 5, 500.0)
    acc = torch.zeros(208, dtype=torch.float64, device=DEV)
    fails, name = [], request.node.callspec.id
    want, scale, lost = np.zeros(208), np.zeros(208), np.zeros(208)
    for k, pose in enumerate((a, b)):
        d = torch.from_numpy(pose).to(DEV)
        N.check(N.lib.a2m_pose_moments_f32(F._p(d), pose.shape[0], necksub, F._p(acc), F._stream()))
        m1, m2, a1, a2 = R.pose_moments(pose, necksub)
        o1, o2, _, _ = R.pose_moments(pose, necksub, omit=-1)
        want += np.concatenate([m1, m2])
        scale += np.concatenate([a1, a2])
        lost = np.abs(np.concatenate([o1 - m1, o2 - m2]))
        got = _np(acc)
        tol = 1e-12 * (np.abs(want) + scale)
        live = np.ones(208, bool)
        if necksub:
            live[[0, 52, 104, 156]] = False            # the neck itself: identically zero
            assert not got[[0, 52, 104, 156]].any()
        worst = float(np.max(np.abs(got - want)[live] / tol[live]))
        margin = float(np.min(lost[live] / tol[live]))
        print(f'ERR part=6-moments case={name}-call{k + 1} q=acc kernel={worst:.3e} torch32=1 ratio={worst:.3f} margin={margin:.1f}')
        if not worst <= 1.0:
            fails.append(f'call {k + 1}: {worst:.3f} x the 1e-12 bound')
        if not margin > 4.0:
            fails.append(f'call {k + 1}: self-check margin {margin:.2f} <= 4')
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('n', NORM_FRAMES, ids=lambda n: f'frames{n}')
def test_pose_normalize_denormalize_bitwise(n):
    """10083 frames are just past 4096 x 256 / 104: the grid-stride loop wraps."""
    from a2m import normalization as NM
    rng = np.random.default_rng(n)
    pose = _planar_pose(n, n + 1, 100.0)
    mean = rng.standard_normal(104).astype(F32)
    std = (rng.random(104) + 0.5).astype(F32)
    neck = np.repeat(pose[:, [0, 52]], 52, axis=1)
    want = ((pose - neck) - mean) / std
    assert want.dtype == F32
    mean_d, std_d = torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)
    got = NM.necksub_normalize(torch.from_numpy(pose).to(DEV), mean_d, std_d)
    assert got.shape == (n, 104) and np.array_equal(_np(got).view(np.uint32), want.view(np.uint32))
    back = NM.denormalize(got, mean_d, std_d)
    want_back = want * std + mean
    assert want_back.dtype == F32
    assert back.shape == (n, 104) and np.array_equal(_np(back).view(np.uint32), want_back.view(np.uint32))


def pck_ref(pred, gt, alpha):
    """compute_pck in float64 numpy on the float32 inputs; also the smallest |distance - radius|."""
    p, g = pred.astype(np.float64), gt.astype(np.float64)
    ext = np.maximum(g[:, 0].max(1) - g[:, 0].min(1), g[:, 1].max(1) - g[:, 1].min(1))
    radius = ext * alpha
    dist = np.sqrt(((g - p) ** 2).sum(1))
    return (dist <= radius[:, None]).mean(1), (np.abs(dist - radius[:, None]).min() if dist.size else np.inf)


@pytest.mark.parametrize('alpha', [0.1, 0.2])
@pytest.mark.parametrize('N_,K', PCK_SHAPES, ids=['N%d-K%d' % s for s in PCK_SHAPES])
def test_pck_bitwise(N_, K, alpha):
    """K = 63, 64, 65, 130 straddle the wave's lanes; N = 5, 9 leave the last workgroup's waves
    idle.  Redrawn until no distance is within 1e-9 of the radius."""
    from a2m.evaluation import compute_pck
    for bump in range(16):
        rng = np.random.default_rng(1000 * N_ + K + 7919 * bump)
        gt = (rng.standard_normal((N_, 2, K)) * 10).astype(F32)
        pred = (gt + rng.standard_normal((N_, 2, K)) * (1.5 * alpha * 20)).astype(F32)
        want, gap = pck_ref(pred, gt, alpha)
        if gap >= 1e-9 or K == 1:
            break
    else:
        raise AssertionError('no draw without a distance on the radius')
    got = compute_pck(pred, gt, alpha)
    assert got.dtype == np.float64 and got.shape == (N_,)
    assert np.array_equal(got, want)
    if K > 1 and N_ > 0:
        assert 0.0 < want.mean() < 1.0               # hits and misses both occur
    assert np.array_equal(compute_pck(gt, gt, alpha), np.ones(N_))      # K = 1: radius 0, distance 0


def test_pck_exact_radius():
    """A gt extent of 20 with alpha 0.25: an offset of exactly (3, 4) is a hit (5 <= 5), (3, 4.000001) a miss."""
    from a2m.evaluation import compute_pck
    K = 52
    gt = np.zeros((2, 2, K), dtype=F32)
    gt[:, 0] = np.linspace(0, 20, K, dtype=F32)
    gt[:, 0, -1] = 20.0
    gt[:, 1] = np.arange(K, dtype=F32) % 7
    pred = gt.copy()
    pred[0, :, 0] = gt[0, :, 0] + F32((3.0, 4.0))
    pred[1, :, 0] = gt[1, :, 0] + F32((3.0, 4.000001))
    assert pred[1, 1, 0] > F32(4.0)
    got = compute_pck(pred, gt, 0.25)
    assert np.array_equal(got, np.array([1.0, (K - 1) / K]))
    assert np.array_equal(got, pck_ref(pred, gt, 0.25)[0])


def _window_std(C):
    """std with the three values around the loader's threshold where C has room for them."""
    std = (np.random.default_rng(C).random(C) + 0.5).astype(F32)
    edge = F32(1e-7)
    special = [np.nextafter(edge, F32(0)), edge, F32(0)]      # replaced by 1, divides, replaced by 1
    for c, s in zip(range(C), special):
        std[c] = s
    return std


@pytest.mark.parametrize('norm', [False, True], ids=['raw', 'standardised'])
@pytest.mark.parametrize('nw', WINDOW_N, ids=lambda n: f'windows{n}')
@pytest.mark.parametrize('C', WINDOW_C, ids=lambda c: f'C{c}')
@pytest.mark.parametrize('window,interval', WINDOWS, ids=['w%d-i%d' % w for w in WINDOWS])
def test_window_gather_bitwise(window, interval, C, nw, norm):
    """130 windows x 64 x 128 are past 4096 x 256 elements: the grid-stride loop wraps."""
    from a2m.windowing import gather_windows
    rng = np.random.default_rng(window + 10 * interval + C + nw)
    L = 300
    data = rng.standard_normal((L, C)).astype(F32)
    starts = rng.integers(0, L - window + 1, nw).astype(np.int64)
    if nw:
        starts[-1] = L - window                         # the last admissible window
    nj = -(-window // interval)
    want = np.stack([data[s:s + window:interval] for s in starts]) if nw else np.zeros((0, nj, C), F32)
    mean = std = None
    if norm:
        mean, std = rng.standard_normal(C).astype(F32), _window_std(C)
        s = np.where(std < F32(1e-7), F32(1), std)
        with np.errstate(over='ignore'):
            want = (want - mean) / s
        assert want.dtype == F32 and (C == 1 or s[1] == F32(1e-7)) and s[0] == 1
        mean, std = torch.from_numpy(mean).to(DEV), torch.from_numpy(std).to(DEV)
    got = gather_windows(torch.from_numpy(data).to(DEV), starts, window, interval, mean, std)
    assert tuple(got.shape) == (nw, nj, C)
    assert np.array_equal(_np(got).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------ for the CPU module
def cases():
    """Every input the tests here draw, for tests/test_loss_ref_cpu.py: the references are proved
    and the input conditions checked at exactly these."""
    return dict(
        pose=[dict(B=B, T=T, seed=pose_inputs(B, T)[0], gen=pose_inputs(B, T)[1], real=pose_inputs(B, T)[2])
              for B, T in POSE_SHAPES],
        pose_degenerate=degenerate_pose(),
        motion=[motion_inputs(*s) for s in MOTION_SHAPES],
        motion_degenerate=degenerate_motion(),
        mse=[mse_inputs(n, v) for n in MSE_N for v in range(4)],
        interp=[(s,) + _interp_inputs(*s) for s in INTERP_SHAPES],
        adam=[(n, wd) for n in ADAM_N for wd in (0.0, 0.01)],
        weights=POSE_WEIGHTS, grad_outs=GRAD_OUTS, gterms=MOTION_GTERMS)
