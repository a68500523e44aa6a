"""csrc/train_norm.hip against float64: training / eval / sync BatchNorm with dropout at every
launch shape, the dropout hash, sum_bt and the LayerNorm backward.

References are torch-CPU float64 autograd of `mask -> batch_norm -> act -> mask` (layer_norm for
part 6); dropout masks come from tests/dropout_ref.py, never from the device.

Tolerances (none is tuned to the kernels):
  save_mean, running_mean   |err| <= 2^-22 (|value| + std)   the kernels accumulate in float64 and
  save_rstd, running_var    |err| <= 2^-22 value             round once: one fp32 rounding, x4
  y, dx, dgamma, dbeta      rel_err <= 8 x the rel_err torch-CPU float32 makes on the same inputs
                            against the same float64 reference (summation order, FMA contraction,
                            the max over up to 80 k elements)
  dbias (train mode)        zero in exact arithmetic; |dbias| <= 2^-20 sum_i gamma rstd (|g_i| +
                            |mean g| + |xhat_i mean(g xhat)|) pre_i: every dx_i is a three-term fp32
                            expression whose operands carry a few roundings each (xhat's are
                            amplified by |mean| / std <= 4 here); 16 roundings of the terms'
                            magnitudes, all aligned, bound their sum
Elements whose float64 pre-activation lies within 1e-5 of an activation kink are left out of the
dx comparison (at most 8 per case, else the case fails); inputs whose pre-activation comes within
1e-6 of a kink are redrawn, because dgamma / dbeta are discontinuous there.

Sensitivity self-check (CPU, every case): the float64 reference recomputed with the channel's last
kept sentinel left out of every per-channel sum must move each bounded quantity by more than 4 x
its tolerance (for dbias: that element's dx must exceed 4 x the bound).

Seen on an MI355X (every case prints its figures; run with -s): the largest kernel rel_err /
torch-float32 rel_err (bound 8), the largest statistics or dbias error / its bound (bound 1), and
the smallest self-check margin, reference shift / tolerance (must exceed 4).  torch float32 itself
is 2e-8 .. 9e-7 from float64 on these inputs.

  part                                   kernel / torch32   stat err / bound   self-check margin
  2  train, 9 launch shapes x 6 modes    2.98 (dx, N 255)   0.30               26
  3  strided operands                    1.73               0.25               21
  3  optional operands                   1.43               0.24               82
  3  ill-conditioned channels (y)        1.00               0.19               -
  3  seed offset                         1.44               0.20               489
  4  eval backward                       1.73               -                  21035 (dgamma, dbeta)
  5  sync phases, whole-batch reference  2.37               0.22               13
  6  LayerNorm backward                  1.78               -                  -
  6  sum_bt                              -                  0.16               -
The train-mode dbias reached 0.055 of its bound (smallest self-check margin 4.9).  No case
failed: the module found no bug in the kernels.
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import dropout_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS, MOM, SLOPE = 1e-5, 0.1, 0.2
ACT_NONE, ACT_RELU, ACT_LRELU = 0, 1, 2
C = 5
CH_STATS = [(0.0, 1.0), (0.3, 1.5), (-2.0, 0.5), (1.0, 1.0), (0.5, 2.0)]
ILL_STATS = [(30.0, 0.05), (-1000.0, 1.0), (0.0, 1e-3), (1.0, 1.0), (0.5, 2.0)]
SENTINELS = (0, 63, 64, 255, 256, 1023, 1024)
STAT_TOL = 2.0 ** -22
SEED_BEFORE, SEED_CH, SEED_AFTER = 1234, 99, 7
COUNTER = 3

# (B, L) -> launch shape; L divides neither 64 nor the thread count
SHAPES = [((3, 85), 'chan256x1'), ((1, 257), 'chan256x2'), ((3, 171), 'chan256x4'),
          ((5, 205), 'chan512x4'), ((3, 683), 'chan1024x4'), ((17, 241), 'chan1024x8'),
          ((3, 2731), 'chan1024x16'), ((64, 256), 'chan1024x16_last'), ((5, 3277), 'sliced17')]
# DROP_BEFORE_CH wants B >= 4 (>= 20 mask units) and L = H W: the smallest such N in each bucket
CH_SHAPES = [((5, 3, 17), 'chan256x1'), ((4, 5, 13), 'chan256x2'), ((9, 3, 19), 'chan256x4'),
             ((5, 5, 41), 'chan512x4'), ((5, 10, 41), 'chan1024x4'), ((5, 20, 41), 'chan1024x8'),
             ((5, 11, 149), 'chan1024x16'), ((64, 16, 16), 'chan1024x16_last'),
             ((5, 29, 113), 'sliced17')]
MODES = [('none_lrelu', R.DROP_NONE, 0.0, ACT_LRELU, 0), ('none_relu', R.DROP_NONE, 0.0, ACT_RELU, 0),
         ('none_linear', R.DROP_NONE, 0.0, ACT_NONE, 0),
         ('before_p0.4_lrelu', R.DROP_BEFORE, 0.4, ACT_LRELU, SEED_BEFORE),
         ('before_ch_p0.4_lrelu', R.DROP_BEFORE_CH, 0.4, ACT_LRELU, SEED_CH),
         ('after_p0.25_lrelu', R.DROP_AFTER, 0.25, ACT_LRELU, SEED_AFTER)]
SYNC_HALVES = [((2, 37), 'slices1'), ((3, 700), 'slices3'), ((2, 8193), 'slices9')]
SYNC_MODES = [MODES[0], MODES[3], MODES[5]]
OFFSET_MODES = [MODES[3], MODES[5]]
OFFSET_SHAPE = (5, 205)
STRIDED_SHAPES = [(3, 171), (5, 3277)]
EVAL_SHAPES = [(3, 683), (5, 3277)]
DROPOUT_CASES = [(1, 0.3, 7), (255, 0.3, 7), (257, 0.3, 1234), (2097153 + 77, 0.2, 99)]


def sentinel_indices(N, ranks=1):
    """Logical per-channel indices of the sentinels, counted within each rank's part of the batch."""
    Nr = N // ranks
    return sorted({k * Nr + i for k in range(ranks) for i in SENTINELS + (Nr - 1,) if i < Nr})


def pick_seed(base, B, L, p, mode, ranks=1, counter=0):
    """The first seed from `base` upwards under which every channel keeps the input of at least one
    sentinel, so that the sensitivity self-check has an element to leave out in every channel.
    (B, L) is one rank's shape; the ranks hash the same local indices."""
    if mode in (R.DROP_NONE, R.DROP_AFTER):
        return base
    sent = sentinel_indices(B * L)
    for seed in range(base, base + 64):
        pre = R.bn_scales(R.offset_seed(seed, counter), B, C, L, p, mode)[0]
        if all(any(pre[i // L, c, i % L] != 0.0 for i in sent) for c in range(C)):
            return seed
    raise AssertionError('no seed keeps a sentinel in every channel')


def _train_cases():
    out = []
    for mi, m in enumerate(MODES):
        for si in range(len(SHAPES)):
            if m[1] == R.DROP_BEFORE_CH:
                (B, H, W), path = CH_SHAPES[si]
                shape = (B, C, H, W)
            else:
                (B, L), path = SHAPES[si]
                shape = (B, C, L)
            L = int(np.prod(shape[2:]))
            mm = m[:4] + (pick_seed(m[4], B, L, m[2], m[1]),)
            out.append(pytest.param(shape, mm, 100 * mi + si, id=f'{path}-N{B * L}-{m[0]}'))
    return out


def mask_uses():
    """Every (units, p, seed, per_clip_channel) the tests here hash: read by test_dropout_ref_cpu."""
    uses = []
    for prm in _train_cases():
        shape, (_, mode, p, _, seed), _ = prm.values
        if mode == R.DROP_NONE:
            continue
        n = shape[0] * C if mode == R.DROP_BEFORE_CH else int(np.prod(shape))
        uses.append((n, p, seed, mode == R.DROP_BEFORE_CH))
    for B, L in STRIDED_SHAPES + EVAL_SHAPES:
        uses.append((B * C * L, 0.4, pick_seed(SEED_BEFORE, B, L, 0.4, R.DROP_BEFORE), False))
    for _, mode, p, _, seed in OFFSET_MODES:
        B, L = OFFSET_SHAPE
        seed = pick_seed(seed, B, L, p, mode, counter=COUNTER)
        uses.append((B * C * L, p, R.offset_seed(seed, COUNTER), False))
    for (B, L), _ in SYNC_HALVES:
        for _, mode, p, _, seed in SYNC_MODES[1:]:
            uses.append((B * C * L, p, pick_seed(seed, B, L, p, mode), False))
    for n, p, seed in DROPOUT_CASES:
        uses.append((n, p, seed, False))
    return uses


# ------------------------------------------------------------------------------ inputs / references
class Inputs:
    pass


def make_inputs(B, L, gen_seed, stats=CH_STATS, sentinel=8.0, ranks=1):
    """float32 CPU operands of a [B, C, L] case; sentinels at the logical per-channel indices where
    a stripe, wave, workgroup or slice begins or ends (counted within each rank's part of the batch)."""
    g = torch.Generator().manual_seed(gen_seed)
    inp = Inputs()
    inp.B, inp.L, inp.N = B, L, B * L
    x = torch.randn(B, C, L, generator=g)
    dy = torch.randn(B, C, L, generator=g)
    for c, (m, s) in enumerate(stats):
        x[:, c] = x[:, c] * s + m
    inp.sent = sentinel_indices(inp.N, ranks)
    for i in inp.sent:
        b, l = divmod(i, L)
        for c, (_, s) in enumerate(stats):
            x[b, c, l] += sentinel * s
        dy[b, :, l] += sentinel
    inp.x, inp.dy = x, dy
    inp.gamma = torch.rand(C, generator=g) + 0.5
    inp.beta = torch.randn(C, generator=g) * 0.1
    inp.rm0 = torch.randn(C, generator=g) * 0.5
    inp.rv0 = torch.rand(C, generator=g) + 0.5
    return inp


def _act(t, act):
    if act == ACT_RELU:
        return torch.relu(t)
    if act == ACT_LRELU:
        return TF.leaky_relu(t, SLOPE)
    return t


def bn_autograd(inp, pre, post, act, dtype, training=True, affine=True, running=True):
    """torch-CPU autograd of mask -> batch_norm -> act -> mask in `dtype`."""
    x = inp.x.to(dtype).clone().requires_grad_(True)
    gam = inp.gamma.to(dtype).clone().requires_grad_(True) if affine else None
    bet = inp.beta.to(dtype).clone().requires_grad_(True) if affine else None
    rm = inp.rm0.to(dtype).clone() if running else None
    rv = inp.rv0.to(dtype).clone() if running else None
    pre_t, post_t = torch.from_numpy(pre).to(dtype), torch.from_numpy(post).to(dtype)
    z = x * pre_t
    pa = TF.batch_norm(z, rm, rv, gam, bet, training, MOM, EPS)
    y = _act(pa, act) * post_t
    y.backward(inp.dy.to(dtype))
    zd = z.detach()
    if training:
        mean, var = zd.mean((0, 2)), zd.var((0, 2), unbiased=False)
    else:
        mean, var = rm.clone(), rv.clone()
    out = dict(y=y.detach(), pa=pa.detach(), mean=mean, rstd=1.0 / torch.sqrt(var + EPS),
               std=zd.var((0, 2), unbiased=False).sqrt(), dx=x.grad, dbias=x.grad.sum((0, 2)))
    if running:
        out['rm'], out['rv'] = rm, rv
    if affine:
        out['dg'], out['db'] = gam.grad, bet.grad
    return {k: v.numpy() for k, v in out.items()}


def bn_manual(inp, pre, post, act, omit=None, training=True):
    """The same operation by the kernels' formulas in float64 numpy; `omit` [C] flat indices (or
    None) of one element per channel left out of every per-channel sum, the divisor unchanged: what
    a kernel computes that loses an element at an edge.  Also returns the train-mode dbias scale."""
    x, dy = inp.x.double().numpy(), inp.dy.double().numpy()
    gam, bet = inp.gamma.double().numpy()[None, :, None], inp.beta.double().numpy()[None, :, None]
    N = inp.N
    w = np.ones_like(x)
    if omit is not None:
        for c, i in enumerate(omit):
            if i is not None:
                w[i // inp.L, c, i % inp.L] = 0.0
    z = x * pre
    if training:
        mean = (w * z).sum((0, 2)) / N
        var = np.maximum((w * z * z).sum((0, 2)) / N - mean * mean, 0.0)
    else:
        mean, var = inp.rm0.double().numpy(), inp.rv0.double().numpy()
    rstd = 1.0 / np.sqrt(var + EPS)
    xh = (z - mean[None, :, None]) * rstd[None, :, None]
    pa = xh * gam + bet
    slope = {ACT_NONE: 1.0, ACT_RELU: 0.0, ACT_LRELU: SLOPE}[act]
    y = np.where(pa > 0, pa, pa * slope) * post
    g = dy * np.where(pa > 0, 1.0, slope) * post
    sg, sgx = (w * g).sum((0, 2)), (w * g * xh).sum((0, 2))
    mg, mgx = (sg / N, sgx / N) if training else (0.0 * sg, 0.0 * sgx)
    gr = gam * rstd[None, :, None]
    dx = gr * (g - mg[None, :, None] - xh * mgx[None, :, None]) * pre
    terms = (gr * (np.abs(g) + np.abs(mg)[None, :, None] + np.abs(xh * mgx[None, :, None])) * pre).sum((0, 2))
    unb = var * N / (N - 1) if N > 1 else var
    return dict(y=y, mean=mean, rstd=rstd, dx=dx, dg=sgx, db=sg, dbias=dx.sum((0, 2)),
                rm=(1 - MOM) * inp.rm0.double().numpy() + MOM * mean,
                rv=(1 - MOM) * inp.rv0.double().numpy() + MOM * unb, terms=terms)


def last_kept_sentinels(inp, pre):
    """per channel: the last sentinel index whose input the mask keeps (None: every one dropped)."""
    out = []
    for c in range(C):
        kept = [i for i in inp.sent if pre[i // inp.L, c, i % inp.L] != 0.0]
        out.append(kept[-1] if kept else None)
    return out


def draw_case(B, L, gen_seed, pre_post, act, stats=CH_STATS, training=True, ranks=1):
    """Inputs (redrawn while a float64 pre-activation lies within 1e-6 of a kink), masks, float64 ref."""
    for bump in range(16):
        inp = make_inputs(B, L, gen_seed + 7919 * bump, stats, ranks=ranks)
        pre, post = pre_post(inp)
        ref = bn_autograd(inp, pre, post, act, torch.float64, training)
        if act == ACT_NONE or np.abs(ref['pa']).min() >= 1e-6:
            return inp, pre, post, ref
    raise AssertionError('no draw without a pre-activation on a kink')


def _record(part, name, q, kernel, torch32, margin=None):
    """One line per comparison (shown with -s): the figures the module docstring tabulates."""
    ratio = kernel / torch32 if torch32 > 0 else (0.0 if kernel == 0 else float('inf'))
    print(f'ERR part={part} case={name} q={q} kernel={kernel:.3e} torch32={torch32:.3e} ratio={ratio:.3f}'
          + ('' if margin is None else f' margin={margin:.1f}'))


def check_bn(part, name, inp, pre, post, act, ref, got, training=True, affine=True, running=True):
    """Every comparison of parts 2-5 for one case.  `got`: the kernels' outputs as CPU float32
    numpy arrays shaped like the reference's."""
    r32 = bn_autograd(inp, pre, post, act, torch.float32, training, affine, running)
    man = bn_manual(inp, pre, post, act, None, training)
    omit = last_kept_sentinels(inp, pre)
    sens = bn_manual(inp, pre, post, act, omit, training)
    if affine:     # the formulas the self-check perturbs are the reference's
        for q in ('y', 'dx', 'dg', 'db', 'mean', 'rstd'):
            assert rel_err(man[q], ref[q]) < 1e-10, (name, q)
    near = (np.abs(ref['pa']) < 1e-5) if act != ACT_NONE else np.zeros(ref['pa'].shape, bool)
    assert near.sum() <= 8, f'{name}: {near.sum()} elements on an activation kink'
    keep = ~near
    fails = []

    def self_check(q, tol, shift):
        if shift is None:
            return None
        margin = float(np.min(shift / np.maximum(tol, 1e-300)))
        if not margin > 4.0:
            fails.append(f'{q}: self-check margin {margin:.2f} <= 4')
        return margin

    # statistics: absolute bounds, per channel
    if training:
        std = ref['std']
        stat_q = [('mean', got['mean'], STAT_TOL * (np.abs(ref['mean']) + std)),
                  ('rstd', got['rstd'], STAT_TOL * ref['rstd'])]
        if running:
            stat_q += [('rm', got['rm'], STAT_TOL * (np.abs(ref['rm']) + std)),
                       ('rv', got['rv'], STAT_TOL * ref['rv'])]
        for q, val, tol in stat_q:
            err = np.abs(val.astype(np.float64) - ref[q])
            margin = self_check(q, tol, np.abs(sens[q] - ref[q]))
            worst = float(np.max(err / tol))
            print(f'STAT part={part} case={name} q={q} err/bound={worst:.3f}'
                  + ('' if margin is None else f' margin={margin:.1f}'))
            if not worst <= 1.0:
                fails.append(f'{q}: error {worst:.3f} x its bound')
    # tensors: 8 x torch float32's error
    tens = [('y', slice(None))]
    tens.append(('dx', keep))
    if affine:
        tens += [('dg', slice(None)), ('db', slice(None))]
    if not training:
        tens.append(('dbias', slice(None)))
    for q, sel in tens:
        e_k = rel_err(got[q].astype(np.float64)[sel], ref[q][sel])
        e_t = rel_err(r32[q].astype(np.float64)[sel], ref[q][sel])
        tol = 8.0 * e_t
        shift = None
        if training or q in ('dg', 'db'):      # eval mode: only these two are sums over the channel
            shift = rel_err(sens[q][sel], ref[q][sel])
        margin = self_check(q, tol, shift)
        _record(part, name, q, e_k, e_t, margin)
        if not e_k <= tol:
            fails.append(f'{q}: rel_err {e_k:.3e} > 8 x torch float32 {e_t:.3e}')
    if training and got.get('dbias') is not None:
        bound = 2.0 ** -20 * man['terms']
        err = np.abs(got['dbias'].astype(np.float64) - ref['dbias'])
        worst = float(np.max(err / np.maximum(bound, 1e-300)))
        # a sum that loses the sentinel's dx is off by that dx
        lost = np.array([abs(ref['dx'][i // inp.L, c, i % inp.L]) for c, i in enumerate(omit)])
        margin = self_check('dbias', bound, lost)
        print(f'STAT part={part} case={name} q=dbias err/bound={worst:.3f} margin={margin:.1f}')
        if not worst <= 1.0:
            fails.append(f'dbias: {worst:.3f} x its bound')
    assert not fails, f'{name}: ' + '; '.join(fails)


def pre_post_for(mode, p, seed):
    def f(inp):
        return R.bn_scales(seed, inp.B, C, inp.L, p, mode)
    return f


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def run_fused(F, inp, shape, mode, p, seed, act, affine=True, running=True, want_bias=True, x=None,
              dy=None, out=None):
    x = inp.x.view(shape).to(DEV) if x is None else x
    dy = inp.dy.view(shape).to(DEV) if dy is None else dy
    gam, bet = (inp.gamma.to(DEV), inp.beta.to(DEV)) if affine else (None, None)
    rm, rv = (inp.rm0.to(DEV), inp.rv0.to(DEV)) if running else (None, None)
    y, mean, rstd = F.bn_train(x, gam, bet, rm, rv, MOM, EPS, p, mode, seed, act, SLOPE, out=out)
    dx, dg, db, dbias = F.bn_train_bwd(dy, x, gam, bet, mean, rstd, p, mode, seed, act, SLOPE,
                                       want_bias=want_bias)
    assert dx.is_contiguous() and dx.shape == x.shape
    B, L = inp.B, inp.L
    return dict(y=_np(y).reshape(B, C, L), mean=_np(mean), rstd=_np(rstd), rm=_np(rm), rv=_np(rv),
                dx=_np(dx).reshape(B, C, L), dg=_np(dg), db=_np(db), dbias=_np(dbias))


def assert_bitwise(a, b, name):
    for k in a:
        if a[k] is None:
            assert b[k] is None
            continue
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), f'{name}: {k} differs between runs'


@pytest.fixture(autouse=True)
def _plain_seeds():
    from a2m import functional as F
    F.set_dropout_seed_offset(None)
    yield
    F.set_dropout_seed_offset(None)


# ------------------------------------------------------------------------------ part 2
@pytest.mark.parametrize('shape,m,gen_seed', _train_cases())
def test_bn_train_every_launch_shape(shape, m, gen_seed, request):
    from a2m import functional as F
    name, mode, p, act, seed = m
    B, L = shape[0], int(np.prod(shape[2:]))
    inp, pre, post, ref = draw_case(B, L, gen_seed, pre_post_for(mode, p, seed), act)
    got = run_fused(F, inp, shape, mode, p, seed, act)
    again = run_fused(F, inp, shape, mode, p, seed, act)
    assert_bitwise(got, again, request.node.callspec.id)
    check_bn('2-train', request.node.callspec.id, inp, pre, post, act, ref, got)


# ------------------------------------------------------------------------------ part 3
@pytest.mark.parametrize('B,L', STRIDED_SHAPES, ids=['chan256x4-N513', 'sliced17-N16385'])
def test_bn_train_strided_operands(B, L, request):
    from a2m import functional as F
    mode, p, act = R.DROP_BEFORE, 0.4, ACT_LRELU
    seed = pick_seed(SEED_BEFORE, B, L, p, mode)
    inp, pre, post, ref = draw_case(B, L, 700 + B, pre_post_for(mode, p, seed), act)
    xbuf = torch.full((B, C + 3, L), 55.5)
    xbuf[:, 2:2 + C] = inp.x
    dybuf = torch.full((B, C + 1, L + 5), -44.5)
    dybuf[:, 1:, :L] = inp.dy
    canary = 777.25
    ybuf = torch.full((B, C + 4, L + 3), canary, device=DEV)
    xv, dyv, yv = xbuf.to(DEV)[:, 2:2 + C], dybuf.to(DEV)[:, 1:, :L], ybuf[:, 1:1 + C, :L]
    assert not xv.is_contiguous() and not dyv.is_contiguous() and not yv.is_contiguous()
    got = run_fused(F, inp, (B, C, L), mode, p, seed, act, x=xv, dy=dyv, out=yv)
    outside = torch.ones(ybuf.shape, dtype=torch.bool)
    outside[:, 1:1 + C, :L] = False
    assert bool((ybuf.cpu()[outside] == canary).all()), 'bytes outside the output slice were written'
    check_bn('3-strided', request.node.callspec.id, inp, pre, post, act, ref, got)


@pytest.mark.parametrize('leg', ['no_affine', 'no_running', 'no_bias'])
@pytest.mark.parametrize('B,L', [(3, 171), (5, 3277)], ids=['chan256x4-N513', 'sliced17-N16385'])
def test_bn_train_optional_operands(B, L, leg, request):
    from a2m import functional as F
    mode, p, seed, act = R.DROP_NONE, 0.0, 0, ACT_LRELU
    affine, running, want_bias = leg != 'no_affine', leg != 'no_running', leg != 'no_bias'
    inp = make_inputs(B, L, 800 + B)
    if not affine:
        inp.gamma, inp.beta = torch.ones(C), torch.zeros(C)   # what the reference formulas then use
    pre, post = pre_post_for(mode, p, seed)(inp)
    ref = bn_autograd(inp, pre, post, act, torch.float64, True, affine, running)
    got = run_fused(F, inp, (B, C, L), mode, p, seed, act, affine, running, want_bias)
    if not affine:
        assert got['dg'] is None and got['db'] is None
    if not want_bias:
        assert got['dbias'] is None
    check_bn('3-optional', request.node.callspec.id, inp, pre, post, act, ref, got, True, affine, running)


@pytest.mark.parametrize('B,L', [(3, 683), (5, 3277)], ids=['chan1024x4-N2049', 'sliced17-N16385'])
def test_bn_train_ill_conditioned_channels(B, L, request):
    """Channels whose mean is large against their spread: E[z^2] - mean^2 must survive, and with
    the saved fp32 statistics taken as exact what remains of y's error is elementwise rounding."""
    from a2m import functional as F
    act = ACT_LRELU
    inp = make_inputs(B, L, 900 + B, ILL_STATS)
    one = np.ones((B, C, L))
    ref = bn_autograd(inp, one, one, act, torch.float64)
    rm, rv = inp.rm0.to(DEV), inp.rv0.to(DEV)
    y, mean, rstd = F.bn_train(inp.x.to(DEV), inp.gamma.to(DEV), inp.beta.to(DEV), rm, rv, MOM, EPS, 0.0,
                               R.DROP_NONE, 0, act, SLOPE)
    fails = []
    for q, val, tol in [('mean', mean, STAT_TOL * (np.abs(ref['mean']) + ref['std'])),
                        ('rstd', rstd, STAT_TOL * ref['rstd']),
                        ('rm', rm, STAT_TOL * (np.abs(ref['rm']) + ref['std'])),
                        ('rv', rv, STAT_TOL * ref['rv'])]:
        worst = float(np.max(np.abs(_np(val).astype(np.float64) - ref[q]) / tol))
        print(f'STAT part=3-ill case={request.node.callspec.id} q={q} err/bound={worst:.3f}')
        if not worst <= 1.0:
            fails.append(f'{q}: {worst:.3f} x its bound')

    def expr(dtype):
        mu, rs = mean.cpu().to(dtype)[None, :, None], rstd.cpu().to(dtype)[None, :, None]
        g, b = inp.gamma.to(dtype)[None, :, None], inp.beta.to(dtype)[None, :, None]
        return _act((inp.x.to(dtype) - mu) * rs * g + b, act).numpy()
    y64, y32 = expr(torch.float64), expr(torch.float32)
    e_k, e_t = rel_err(_np(y), y64), rel_err(y32, y64)
    _record('3-ill', request.node.callspec.id, 'y', e_k, e_t)
    if not e_k <= 8 * e_t:
        fails.append(f'y: rel_err {e_k:.3e} > 8 x torch float32 {e_t:.3e}')
    assert not fails, '; '.join(fails)


@pytest.mark.parametrize('m', OFFSET_MODES, ids=lambda m: m[0])
def test_bn_train_seed_offset(m, request):
    """With a device counter holding 3 registered, forward and backward hash seed + 3 K."""
    from a2m import functional as F
    name, mode, p, act, seed = m
    B, L = OFFSET_SHAPE
    seed = pick_seed(seed, B, L, p, mode, counter=COUNTER)
    eff = R.offset_seed(seed, COUNTER)
    assert eff != seed
    inp, pre, post, ref = draw_case(B, L, 1000 + mode, pre_post_for(mode, p, eff), act)
    plain = R.bn_scales(seed, B, C, L, p, mode)
    assert (plain[0] != pre).any() or (plain[1] != post).any()
    counter = torch.tensor([COUNTER], dtype=torch.int64, device=DEV)
    F.set_dropout_seed_offset(counter)
    try:
        got = run_fused(F, inp, (B, C, L), mode, p, seed, act)
    finally:
        F.set_dropout_seed_offset(None)
    check_bn('3-offset', request.node.callspec.id, inp, pre, post, act, ref, got)


# ------------------------------------------------------------------------------ part 4
@pytest.mark.parametrize('B,L', EVAL_SHAPES, ids=['chan1024x4-N2049', 'sliced17-N16385'])
def test_bn_eval_backward(B, L, request):
    from a2m import functional as F
    mode, p, act = R.DROP_BEFORE, 0.4, ACT_LRELU
    seed = pick_seed(SEED_BEFORE, B, L, p, mode)
    inp, pre, post, ref = draw_case(B, L, 1100 + B, pre_post_for(mode, p, seed), act, training=False)
    x, dy = inp.x.to(DEV), inp.dy.to(DEV)
    gam, bet, rm, rv = (t.to(DEV) for t in (inp.gamma, inp.beta, inp.rm0, inp.rv0))
    y, mean, rstd = F.bn_eval(x, gam, bet, rm, rv, EPS, act, SLOPE, p=p, mode=mode, seed=seed)
    dx, dg, db, dbias = F.bn_eval_bwd(dy, x, gam, bet, mean, rstd, act, SLOPE, p=p, mode=mode, seed=seed)
    assert torch.equal(rm.cpu(), inp.rm0) and torch.equal(rv.cpu(), inp.rv0)
    assert torch.equal(mean.cpu(), inp.rm0)
    assert np.all(np.abs(_np(rstd).astype(np.float64) - ref['rstd']) <= STAT_TOL * ref['rstd'])
    got = dict(y=_np(y), dx=_np(dx), dg=_np(dg), db=_np(db), dbias=_np(dbias))
    check_bn('4-eval', request.node.callspec.id, inp, pre, post, act, ref, got, training=False)


# ------------------------------------------------------------------------------ part 5
def _run_sync(F, N, halves, mode, p, seed, act):
    """Two ranks' stats / apply / bwd_stats / bwd_apply phases with the float64 sums added between."""
    n_total = sum(h.B * h.L for h in halves)
    xs, dys = [h.x.to(DEV) for h in halves], [h.dy.to(DEV) for h in halves]
    gam, bet = halves[0].gamma.to(DEV), halves[0].beta.to(DEV)
    sums = []
    for h, x in zip(halves, xs):
        s = torch.empty(C, 2, device=DEV, dtype=torch.float64)
        F._with_ws(DEV, lambda wp, wn: N.lib.a2m_bn_sync_stats_f32(
            F._p(x), x.stride(0), x.stride(1), h.B, C, h.L, p, mode, seed, F._p(s), wp, wn, F._stream()))
        sums.append(s)
    tot = sums[0] + sums[1]
    outs = []
    for h, x in zip(halves, xs):
        rm, rv = h.rm0.to(DEV), h.rv0.to(DEV)
        y = torch.empty_like(x)
        mean, rstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        N.check(N.lib.a2m_bn_sync_apply_f32(
            F._p(x), x.stride(0), x.stride(1), h.B, C, h.L, F._p(tot), n_total, F._p(gam), F._p(bet), F._p(rm),
            F._p(rv), MOM, EPS, p, mode, seed, act, SLOPE, F._p(y), y.stride(0), y.stride(1), F._p(mean),
            F._p(rstd), F._stream()))
        outs.append(dict(y=y, mean=mean, rstd=rstd, rm=rm, rv=rv))
    for k in ('mean', 'rstd', 'rm', 'rv'):
        assert torch.equal(outs[0][k], outs[1][k]), f'ranks disagree on {k}'
    mean, rstd = outs[0]['mean'], outs[0]['rstd']
    bsums, dgs, dbs = [], [], []
    for h, x, dy in zip(halves, xs, dys):
        s = torch.empty(C, 2, device=DEV, dtype=torch.float64)
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        F._with_ws(DEV, lambda wp, wn: N.lib.a2m_bn_sync_bwd_stats_f32(
            F._p(dy), dy.stride(0), dy.stride(1), F._p(x), x.stride(0), x.stride(1), h.B, C, h.L, F._p(gam),
            F._p(bet), F._p(mean), F._p(rstd), p, mode, seed, act, SLOPE, F._p(s), F._p(dg), F._p(db), wp, wn,
            F._stream()))
        bsums.append(s); dgs.append(dg); dbs.append(db)
    btot = bsums[0] + bsums[1]
    dxs, dbiases = [], []
    for h, x, dy in zip(halves, xs, dys):
        dx, dbias = torch.empty_like(x), torch.empty(C, device=DEV)
        F._with_ws(DEV, lambda wp, wn: N.lib.a2m_bn_sync_bwd_apply_f32(
            F._p(dy), dy.stride(0), dy.stride(1), F._p(x), x.stride(0), x.stride(1), h.B, C, h.L, F._p(gam),
            F._p(bet), F._p(mean), F._p(rstd), p, mode, seed, act, SLOPE, F._p(btot), n_total, F._p(dx),
            F._p(dbias), wp, wn, F._stream()))
        dxs.append(dx); dbiases.append(dbias)
    f32 = np.float32
    return dict(y=_np(torch.cat([o['y'] for o in outs])), mean=_np(mean), rstd=_np(rstd), rm=_np(outs[0]['rm']),
                rv=_np(outs[0]['rv']), dx=_np(torch.cat(dxs)),
                dg=(_np(dgs[0]).astype(np.float64) + _np(dgs[1])).astype(f32),
                db=(_np(dbs[0]).astype(np.float64) + _np(dbs[1])).astype(f32),
                dbias=(_np(dbiases[0]).astype(np.float64) + _np(dbiases[1])).astype(f32))


@pytest.mark.parametrize('m', SYNC_MODES, ids=lambda m: m[0])
@pytest.mark.parametrize('half,path', SYNC_HALVES, ids=[f'sync_{p}' for _, p in SYNC_HALVES])
def test_bn_sync_phases_against_fp64(half, path, m, request):
    """Two half-batches through the SyncBN phases against the float64 reference of the whole
    batch; each rank hashes its local b, so the reference takes dropout_ref's mask per half."""
    from a2m import _native as N
    from a2m import functional as F
    name, mode, p, act, seed = m
    Bh, L = half
    seed = pick_seed(seed, Bh, L, p, mode)

    def pre_post(whole):
        one = R.bn_scales(seed, Bh, C, L, p, mode)
        return np.concatenate([one[0], one[0]]), np.concatenate([one[1], one[1]])
    whole, pre, post, ref = draw_case(2 * Bh, L, 1200 + Bh + mode, pre_post, act, ranks=2)
    halves = []
    for k in range(2):
        h = Inputs()
        h.B, h.L = Bh, L
        h.x, h.dy = whole.x[k * Bh:(k + 1) * Bh].contiguous(), whole.dy[k * Bh:(k + 1) * Bh].contiguous()
        h.gamma, h.beta, h.rm0, h.rv0 = whole.gamma, whole.beta, whole.rm0, whole.rv0
        halves.append(h)
    got = _run_sync(F, N, halves, mode, p, seed, act)
    again = _run_sync(F, N, halves, mode, p, seed, act)
    assert_bitwise(got, again, request.node.callspec.id)
    check_bn('5-sync', request.node.callspec.id, whole, pre, post, act, ref, got)


# ------------------------------------------------------------------------------ part 6
@pytest.mark.parametrize('n,p,seed', DROPOUT_CASES, ids=[f'n{n}' for n, _, _ in DROPOUT_CASES])
def test_dropout_matches_reference_mask(n, p, seed):
    """n = 2,097,230 is past the 8192-workgroup grid cap: the grid-stride loop's second trip runs."""
    from a2m import functional as F
    x = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    x[x == 0] = 1.0
    y = F.dropout(x.to(DEV), p, seed).cpu().numpy()
    keep = R.keep_mask(seed, n, p)
    assert np.array_equal(y != 0, keep), 'keep pattern differs from the reference hash'
    assert np.all(y[~keep].view(np.uint32) << 1 == 0)           # exactly (+-) zero
    want = x.numpy().astype(np.float64)[keep] / (1.0 - float(np.float32(p)))
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert np.all(np.abs(y[keep] - want) <= 2 * ulp)


@pytest.mark.parametrize('accumulate', [False, True], ids=['store', 'accumulate'])
@pytest.mark.parametrize('layout', ['contiguous', 'permuted'])
@pytest.mark.parametrize('B,Cc,T', [(1, 1, 1), (3, 5, 85), (7, 3, 1000)])
def test_sum_bt(B, Cc, T, layout, accumulate):
    from a2m import functional as F
    g = torch.Generator().manual_seed(B * 100 + T)
    x = torch.randn(B, Cc, T, generator=g) + 0.25
    y0 = torch.randn(Cc, generator=g) * 10
    xd = x.to(DEV) if layout == 'contiguous' else x.permute(0, 2, 1).contiguous().to(DEV).permute(0, 2, 1)
    assert layout == 'contiguous' or xd.stride(2) == Cc
    out = y0.to(DEV)
    res = F.sum_bt(xd, out=out, accumulate=accumulate)
    assert res.data_ptr() == out.data_ptr()
    want = x.double().sum((0, 2)) + (y0.double() if accumulate else 0.0)
    bound = STAT_TOL * (x.double().abs().sum((0, 2)) + (y0.double().abs() if accumulate else 0.0))
    err = (out.cpu().double() - want).abs()
    print(f'STAT part=6-sum_bt case={B}x{Cc}x{T}-{layout}-{accumulate} err/bound={(err / bound).max().item():.3f}')
    assert bool((err <= bound).all())


LN_CASES = [(R_, D) for D in (1, 63, 64, 65, 200, 512) for R_ in (1, 5, 17)] + [(16 * 1024 + 1, 65)]


def _ln_case(Rr, D):
    Bn, T = (5, Rr // 5) if Rr % 5 == 0 else (1, Rr)
    g = torch.Generator().manual_seed(Rr * 1000 + D)
    x = torch.randn(Rr, D, generator=g) * 1.5 + 0.5
    dy = torch.randn(Bn, D, T, generator=g)                    # the [B, D, T] layout of the caller
    w = torch.rand(D, generator=g) + 0.5
    b = torch.randn(D, generator=g) * 0.1
    return Bn, T, x, dy, w, b


def _ln_ref(x, dy_rows, w, b, dtype):
    xx, ww, bb = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
    TF.layer_norm(xx, (x.shape[1],), ww, bb, EPS).backward(dy_rows.to(dtype))
    return dict(dx=xx.grad.numpy(), dw=ww.grad.numpy(), db=bb.grad.numpy())


@pytest.mark.parametrize('Rr,D', LN_CASES, ids=[f'R{r}-D{d}' for r, d in LN_CASES])
def test_layernorm_bwd(Rr, D):
    """R = 16385 caps the grid at 1024 workgroups of 17 rows with a ragged last one; D = 65 puts
    the dw | db boundary of reduce_cols inside a 64-column workgroup."""
    from a2m import functional as F
    Bn, T, x, dy, w, b = _ln_case(Rr, D)
    dy_rows = dy.permute(0, 2, 1).reshape(Rr, D)
    x64 = x.double()
    mean64, var64 = x64.mean(1), x64.var(1, unbiased=False)
    mean, rstd = mean64.float(), (1.0 / torch.sqrt(var64 + EPS)).float()
    dx, dw, db = (_np(t) for t in F.layernorm_bwd(dy.to(DEV), x.to(DEV), w.to(DEV), mean.to(DEV),
                                                  rstd.to(DEV), T))
    ref, r32 = _ln_ref(x, dy_rows, w, b, torch.float64), _ln_ref(x, dy_rows, w, b, torch.float32)
    name = f'R{Rr}-D{D}'
    if D == 1:
        # one element per row: xhat = 0 and g - mean(g) = 0 exactly, in any arithmetic
        assert not dx.any() and not dw.any() and np.abs(ref['dx']).max() < 1e-9
        qs = ['db']
    else:
        qs = ['dx', 'dw', 'db']
    fails = []
    for q, val in (('dx', dx), ('dw', dw), ('db', db)):
        if q not in qs:
            continue
        e_k, e_t = rel_err(val, ref[q]), rel_err(r32[q], ref[q])
        _record('6-layernorm', name, q, e_k, e_t)
        if not e_k <= 8 * e_t:
            fails.append(f'{q}: rel_err {e_k:.3e} > 8 x torch float32 {e_t:.3e}')
    if D == 65:
        tw = 8 * rel_err(r32['dw'], ref['dw']) * np.abs(ref['dw']).max()
        tb = 8 * rel_err(r32['db'], ref['db']) * np.abs(ref['db']).max()
        if not abs(float(dw[64]) - ref['dw'][64]) <= tw:
            fails.append('dw[64] (the last column before the segment boundary)')
        if not abs(float(db[0]) - ref['db'][0]) <= tb:
            fails.append('db[0] (the first column after the segment boundary)')
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_layernorm_bwd_rejects_wide_rows():
    """The kernel holds 8 elements per lane (D <= 512): D = 513 is an error, not truncated gradients."""
    from a2m import _native as N
    from a2m import functional as F
    Rr, D = 4, 513
    z = torch.zeros(Rr, D, device=DEV)
    with pytest.raises(N.A2MError):
        F.layernorm_bwd(torch.zeros(1, D, Rr, device=DEV), z, torch.ones(D, device=DEV),
                        torch.zeros(Rr, device=DEV), torch.ones(Rr, device=DEV), Rr)


# ------------------------------------------------------------------------------ part 7
def _raw_entries(F, N, B, L, canary=None):
    """name -> (call(p, mode, ws_ptr, ws_bytes) -> rc, needed workspace bytes, output tensors)."""
    S = -(-B * L // 1024)
    fill = 0.0 if canary is None else canary
    x = torch.randn(B, C, L, device=DEV)
    dy = torch.randn(B, C, L, device=DEV)
    gam, bet = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    mean, rstd = torch.zeros(C, device=DEV), torch.ones(C, device=DEV)
    t = lambda *shape, dtype=torch.float32: torch.full(shape, fill, device=DEV, dtype=dtype)
    y, dx, sm, sr, dg, db, dbias = t(B, C, L), t(B, C, L), t(C), t(C), t(C), t(C), t(C)
    rm, rv = t(C), t(C)
    sums = t(C, 2, dtype=torch.float64)
    sb, sc, st, n_total = C * L, L, F._stream(), 2 * B * L
    lib, P = N.lib, F._p
    return {
        'bn_train_fwd': (lambda p, mode, wp, wn: lib.a2m_bn_train_fwd_f32(
            P(x), sb, sc, B, C, L, P(gam), P(bet), P(rm), P(rv), MOM, EPS, p, mode, 1, ACT_LRELU, SLOPE, P(y),
            sb, sc, P(sm), P(sr), wp, wn, st), 16 * C * S, [y, sm, sr, rm, rv]),
        'bn_train_bwd': (lambda p, mode, wp, wn: lib.a2m_bn_train_bwd_f32(
            P(dy), sb, sc, P(x), sb, sc, B, C, L, P(gam), P(bet), P(mean), P(rstd), p, mode, 1, ACT_LRELU,
            SLOPE, P(dx), P(dg), P(db), P(dbias), wp, wn, st), 24 * C * S, [dx, dg, db, dbias]),
        'bn_sync_stats': (lambda p, mode, wp, wn: lib.a2m_bn_sync_stats_f32(
            P(x), sb, sc, B, C, L, p, mode, 1, P(sums), wp, wn, st), 16 * C * S, [sums]),
        'bn_sync_apply': (lambda p, mode, wp, wn: lib.a2m_bn_sync_apply_f32(
            P(x), sb, sc, B, C, L, P(sums), n_total, P(gam), P(bet), P(rm), P(rv), MOM, EPS, p, mode, 1,
            ACT_LRELU, SLOPE, P(y), sb, sc, P(sm), P(sr), st), None, [y, sm, sr, rm, rv]),
        'bn_sync_bwd_stats': (lambda p, mode, wp, wn: lib.a2m_bn_sync_bwd_stats_f32(
            P(dy), sb, sc, P(x), sb, sc, B, C, L, P(gam), P(bet), P(mean), P(rstd), p, mode, 1, ACT_LRELU,
            SLOPE, P(sums), P(dg), P(db), wp, wn, st), 16 * C * S, [sums, dg, db]),
        'bn_sync_bwd_apply': (lambda p, mode, wp, wn: lib.a2m_bn_sync_bwd_apply_f32(
            P(dy), sb, sc, P(x), sb, sc, B, C, L, P(gam), P(bet), P(mean), P(rstd), p, mode, 1, ACT_LRELU,
            SLOPE, P(sums), n_total, P(dx), P(dbias), wp, wn, st), 8 * C * S + 8 * C + 16, [dx, dbias]),
    }


ENTRIES = ['bn_train_fwd', 'bn_train_bwd', 'bn_sync_stats', 'bn_sync_apply', 'bn_sync_bwd_stats',
           'bn_sync_bwd_apply']


@pytest.mark.parametrize('p,mode', [(1.0, R.DROP_BEFORE), (-0.1, R.DROP_AFTER), (0.25, 4)],
                         ids=['p1.0', 'p-0.1', 'mode4'])
@pytest.mark.parametrize('entry', ENTRIES)
def test_bn_entries_reject_bad_dropout(entry, p, mode):
    """p = 1 would give an infinite keep-scale; every entry refuses it before launching anything."""
    from a2m import _native as N
    from a2m import functional as F
    canary = 321.5
    call, _, outs = _raw_entries(F, N, 2, 37, canary)[entry]
    ws = F.WS.get(DEV)
    rc = call(p, mode, ctypes.c_void_p(ws.data_ptr()), ws.numel())
    assert rc == N.A2M_EINVAL
    assert 'bad dropout' in N.last_error()
    with pytest.raises(N.A2MError):
        N.check(rc)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == canary).all()), 'a rejected call wrote its outputs'


def test_bn_wrappers_raise_on_bad_dropout():
    from a2m import _native as N
    from a2m import functional as F
    x = torch.randn(2, C, 37, device=DEV)
    ones = torch.ones(C, device=DEV)
    for p, mode in [(1.0, R.DROP_BEFORE), (-0.1, R.DROP_AFTER), (0.25, 4)]:
        with pytest.raises(N.A2MError):
            F.bn_train(x, None, None, None, None, MOM, EPS, p, mode, 1, ACT_LRELU)
        with pytest.raises(N.A2MError):
            F.bn_train_bwd(x, x, None, None, ones, ones, p, mode, 1, ACT_LRELU)


@pytest.mark.parametrize('entry', [e for e in ENTRIES if e != 'bn_sync_apply'])
@pytest.mark.parametrize('B,L', [(3, 171), (5, 3277)], ids=['N513', 'N16385'])
def test_bn_entries_report_small_workspace(entry, B, L):
    """One byte short: A2M_EWS, the needed size in last_error(), nothing launched."""
    from a2m import _native as N
    from a2m import functional as F
    canary = 321.5
    call, need, outs = _raw_entries(F, N, B, L, canary)[entry]
    ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    rc = call(0.25, R.DROP_BEFORE, ctypes.c_void_p(ws.data_ptr()), need - 1)
    assert rc == N.A2M_EWS
    assert f'< {need} bytes' in N.last_error(), N.last_error()
    with pytest.raises(N.WorkspaceTooSmall):
        N.check(rc)
    torch.cuda.synchronize()
    for o in outs:
        assert bool((o == canary).all()), 'a refused call wrote its outputs'
    assert bool((ws == 0x5A).all()), 'a refused call wrote its workspace'
    assert call(0.25, R.DROP_BEFORE, ctypes.c_void_p(ws.data_ptr()), need) == 0   # exactly enough runs
    torch.cuda.synchronize()
