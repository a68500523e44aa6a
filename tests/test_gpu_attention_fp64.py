"""csrc/attn_core.hip, csrc/train_attn.hip and the attention entries of csrc/ops.hip against float64 on
every route and at edge shapes: SelfAttention forward with the intermediates kept (the attention core,
the wide core and the general path, a2m_self_attention_route says which), the fused inference kernel
and its grouped launch, the SelfAttention backward through the wrapper and through the C entry, and
ChannelAttention forward and backward.

Reference: tests/attn_ref.py (float64 numpy, gradients written out, proved to 1e-12 against torch
float64 autograd by tests/test_attn_ref_cpu.py at exactly the cases used here).  Inputs are float32
draws of numpy's default_rng; the parity regime is tests/test_gpu_parity.py's scale (weights C^-0.5,
biases 0.1, gamma 0.37), where the largest attention weight of a row is 0.3 to 0.9 at C <= 256 and 1.000
at C = 2048.  One shape per route also runs diffuse (q / k weights scaled by 0.5 (C/8)^-1/4: every row's
largest weight <= 4 / T) and peaked (scaled so that the median largest weight is near 0.75, within
[0.5, 0.95]: A (.) (G - rowdot) cancels and the non-maximal scores still count).

Tolerances (none is tuned to the kernels):
  qkv, attn, y, dx, dW, db   rel_err (max-norm) <= 8 x the rel_err torch-CPU float32 makes on the same
                             inputs by conv1d / bmm / softmax / adaptive_max_pool1d and autograd
  dgamma                     |err| <= 8 x E32 x |value|, E32 the largest relative error torch float32
                             makes on dgamma over every backward case of the module
  dbk                        exactly 0 in exact arithmetic (the softmax ignores a shift of the key bias):
                             max |dbk| / sum_{b,t} |dK| <= 8 x the same figure of torch float32 on that
                             case, or of all cases pooled where torch gives exactly 0
  rows of attn               sum to 1 within 4 ulp x T
  bitwise (np.array_equal)   gamma = 0: y = x (+ res), dx = dy, every weight and bias gradient 0;
                             T = 1: attn = 1, dwq, dwk, dbq, dbk = 0; V chunks of 64 against 128 and a
                             padded against a dense batch stride in the fused kernel; the unstacked
                             against the packed entry; qkv / attn with against without res; dres = dy;
                             ChannelAttention in place against out of place and at a 4-, 8-, 12-byte
                             offset against aligned; sentinels: every output overwritten and not added
                             to, nothing written between strided clips, between unpacked gradients,
                             after the workspace's stated size or by a refused call
Input conditions (checked on the CPU by tests/test_attn_ref_cpu.py through cases()): the stated softmax
regime; every self-check margin above 4; dgamma no more cancelled than sum |rowdot| <= 4 sqrt(B T)
|dgamma| (see dgamma_well_conditioned); every live hidden pre-activation of the ChannelAttention MLP at
least 1e-4 of the largest away from the ReLU kink; the tie cases hold exactly their ties.  The first
seed from 100 upwards (1100, 2100 for the further problems of the grouped launch) that meets them is
used; x and the q / k weights are drawn first so that a seed whose attention matrix fails is passed
over before the C x C value weights are drawn.

Sensitivity self-check (CPU, every comparison of a sum): the reference recomputed with one term left
out must move the bounded quantity by more than 4 x its tolerance -- the last key of the last query
row of the last clip for attn and y (T = 1 has none: the last input channel instead), the last input
channel for qkv, the last row of Wcat^T dqkv for dx, the last (b, t) outer product for dW, db and dbk,
the last rowdot for dgamma, the last time step of the average pool for ChannelAttention's att, y and
dx, the last clip for its weight gradients.

Seen on an MI355X (every comparison prints an ERR line; run with -s): the largest kernel error /
torch-float32 error (bound 8) and the smallest self-check margin, reference shift / tolerance (must
exceed 4).  E32 of dgamma 3.05e-6 (the kernel's largest error 0.89 of it, at (2, 64, 65)); the pooled
dbk figure 2.2e-8 (no case needed it: torch's dbk is never exactly 0; the kernel's largest dbk is 2.02
x torch's, at (3, 2048, 4)).  58 tests, 640 comparisons, 8.6 s in all, 5.7 s of it the references of
all backward cases, prepared by the first test that needs E32.  Every test passes.

  part                                         cases  kernel / torch32               smallest margin
  1  forward, saved intermediates, 19 shapes      38  5.57 (qkv, (1, 128, 1))        13.8 (y, (2, 256, 64))
  2  backward through the wrapper                 19  2.63 (dwk, (1, 384, 17))       55.4 (dbq, (2, 2048, 6))
  1  diffuse and peaked, forward                  12  1.40 (y, (2, 128, 33) peaked)  5.0 (attn, same)
  2  diffuse and peaked, backward                  6  1.61 (dbq, (2, 128, 33) diff.) 1091 (dx, (2, 2048, 20))
  1  padded batch stride                           6  1.27 (attn, (2, 128, 33))      30.7 (y)
  1  gamma = 0 (qkv, attn, dgamma)                 6  1.27 (attn), 0.52 (dgamma)     41.1 (attn)
  2  direct entry, 9 output layouts x 2 shapes    18  1.52 (dwk, (2, 128, 33))       94.3 (dx, (2, 2048, 4))
  3  fused eval, 6 shapes x chunk x res x stride  48  1.54 (y, (2, 128, 4))          13.8 (y, (2, 256, 64))
  3  grouped launch, G = 3                         6  1.01                           516
  4  ChannelAttention forward, 8 shapes            8  1.60 (att, (2, 256, 64, 16))   4115 (y, (2, 256, 60, 32))
  5  ChannelAttention backward                     8  0.96 (dx, (1, 8, 1, 1))        37657 (dx, (3, 256, 64, 32))
  4, 5  ties and MLP edges                         4  1.04 forward, 0.79 (db2, mlp)  4432
  4  offset view, 2048 channels                    2  1.35, 1.07                     14144
Every bitwise comparison holds.

The module found four things, fixed with it:
  channel_attention_bwd_kernel ran the per-clip chain from the pools to dh in float32.  dh = W2^T dz
    sums signed terms that cancel (24-fold at (1, 8, 1, 1)), and every rounding upstream of it
    reached db1 and dW1 multiplied by that: 5.49e-7 on dw1 there, 8.24 x torch float32, where torch's
    order of the 8-term sum lands 0.6 ulp from float64 by luck and the exact sum of the same float32
    terms 5.3 ulp.  The chain (pooled means, MLP, sigmoids, dz, dh: O(C Cr) beside the O(C T) pass
    over x) now runs in float64 and is rounded once on store: 3.4e-8 on that dw1, at most 0.96 x
    torch anywhere in the backward; 28.8 against 26.4 us a call at (64, 256, 64, 32).  Its LDS grows
    from 4 (10 C + 4 Cr) to 4 (11 C + 8 Cr) bytes (C = 1024, Cr = 128 takes 48 KiB).
  a2m_self_attention_eval_f32, _ex_f32 and _group_f32 took T = 0 and T = -4 (multiples of 4 below
    64) for shapes that fit and launched on them; attn_fused_eval_fits now asks T >= 4, and
    a2m_self_attention_eval_fits answers 0 there.
  channel_scale_kernel took its float4 path on T % 4 == 0 alone, so a contiguous view that starts
    4 bytes into an allocation reached 16-byte loads and stores at a 4-byte-aligned address; the host
    now passes a flag, set only when x and y are 16-byte aligned (the offset test ran after the fix only).
  oracle.model.channel_attention pooled with amax, whose backward splits a tie's gradient evenly; the
    reference layer's AdaptiveMaxPool1d and the kernel send it to the first maximum.  The oracle now
    uses adaptive_max_pool1d; no golden fixture moves.
"""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import attn_ref as R
from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)

SEED_BASE = 100
SEED_TRIES = 400
GAMMA = 0.37
SENTINEL = 12345.0

# (B, C, T) by the kernel a2m_self_attention_route(C, T, 1) names
SA_CORE = [(1, 128, 1), (2, 128, 33), (2, 128, 64), (3, 256, 63), (2, 256, 64), (1, 384, 17), (2, 512, 12)]
SA_WIDE = [(3, 2048, 4), (2, 2048, 20), (2, 2048, 32), (2, 1024, 8), (1, 1536, 12)]
SA_GENERAL = [(3, 16, 5), (1, 8, 1), (2, 64, 65), (1, 64, 130), (2, 256, 65), (2, 2048, 6), (1, 2048, 36)]
SA_SHAPES = SA_CORE + SA_WIDE + SA_GENERAL
# one shape per route in the diffuse and the peaked regime, with gamma = 0, and with a padded batch stride
SA_REGIME_SHAPES = [(2, 128, 33), (2, 2048, 20), (2, 64, 65)]
# the q / k weight scale (in units of C^-0.5) that puts the median largest weight near 0.75
SA_PEAKED_SCALE = {(2, 128, 33): 1.1, (2, 2048, 20): 0.6, (2, 64, 65): 1.5}
SA_GAMMA0_SHAPES = [(2, 128, 33), (2, 2048, 4), (3, 16, 5)]
SA_STRIDED = [((2, 128, 33), 5), ((2, 2048, 20), 4), ((3, 16, 5), 7)]     # (shape, floats between clips)
SA_DIRECT_SHAPES = [(2, 128, 33), (2, 2048, 4)]
SA_UNSTACKED_SHAPE = (2, 128, 33)
FUSED_SHAPES = [(2, 128, 4), (3, 128, 36), (2, 128, 64), (2, 256, 12), (2, 256, 60), (2, 256, 64)]
FUSED_PAD = 8
GROUP_SHAPE, GROUP_G = (2, 256, 12), 3

# (B, C, T, Cr)
CA_SHAPES = [(1, 8, 1, 1), (2, 12, 7, 3), (2, 64, 20, 8), (2, 128, 33, 16), (2, 256, 60, 32), (3, 256, 64, 32),
             (2, 256, 64, 16), (1, 1024, 9, 128)]
CA_SPECIAL_SHAPES = [(2, 64, 20, 8), (2, 256, 64, 32)]       # ties and MLP cases
CA_FUSED_SHAPE = (3, 256, 64, 32)
CA_OFFSET_SHAPE = (2, 256, 64, 16)
CA_WIDE_SHAPE = (1, 2048, 4, 256)       # the forward takes it, the backward's LDS does not
TIE_ZERO, TIE_LANES, TIE_SAME, TIE_LAST = 0, 1, 2, 3      # the channels the tie cases rewrite
DEAD_ZERO, DEAD_NEG = 0, 1                                # hidden units of the MLP case
SAT_HI, SAT_LO = 4, 5                                     # its saturated output channels


def _t(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def _np(t):
    return None if t is None else t.detach().cpu().numpy()


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(DEV)


def _record(part, name, q, kernel, torch32, margin=None):
    """One line per comparison (shown with -s): the figures the module docstring tabulates."""
    ratio = kernel / torch32 if torch32 > 0 else (0.0 if kernel == 0 else float('inf'))
    print(f'ERR part={part} case={name} q={q} kernel={kernel:.3e} torch32={torch32:.3e} ratio={ratio:.3f}'
          + ('' if margin is None else f' margin={margin:.1f}'))


def _margin(shift, e32):
    return shift / max(8.0 * e32, 1e-300)


# ------------------------------------------------------------------------------ SelfAttention: inputs
def sa_make(B, C, T, regime, seed, gamma=GAMMA, early=None):
    """float32 inputs of one case, or None.  regime: 'parity' (tests/test_gpu_parity.py's scale:
    q ~ N(0, 1)), 'diffuse', 'peaked' (the q / k weights and biases rescaled) or 'gamma0' (parity with
    gamma = 0).  x and the q / k projection are drawn first; `early`, if given, sees them and may turn
    the seed down before the C x C value weights are drawn (the same stream either way)."""
    rng = np.random.default_rng(seed)
    Cq = C // 8
    s = {'diffuse': 0.5 * Cq ** -0.25, 'peaked': SA_PEAKED_SCALE.get((B, C, T), 1.0)}.get(regime, 1.0)

    def r(*shape, scale=1.0):
        return rng.standard_normal(shape, dtype=F32) * F32(scale)
    c = types.SimpleNamespace(
        B=B, C=C, T=T, regime=regime, seed=seed, x=r(B, C, T),
        wq=r(Cq, C, scale=s * C ** -0.5), bq=r(Cq, scale=0.1 * s), wk=r(Cq, C, scale=s * C ** -0.5),
        bk=r(Cq, scale=0.1 * s), gamma=np.array([0.0 if regime == 'gamma0' else gamma], dtype=F32))
    if early is not None and not early(c):
        return None
    c.wv, c.bv, c.res, c.dy = r(C, C, scale=C ** -0.5), r(C, scale=0.1), r(B, C, T), r(B, C, T)
    return c


def sa_attention_ok(c):
    """The conditions that rest on x and the q / k projection alone: the softmax regime and the attention
    matrix's self-check margin, by the very operations sa_prepare and sa_torch use for them."""
    qk = R.project(c.x, np.concatenate([c.wq, c.wk]).astype(np.float64), np.concatenate([c.bq, c.bk]).astype(np.float64))
    Cq = c.C // 8
    attn = R.softmax_scores(qk[:, :Cq], qk[:, Cq:])
    if not sa_regime_ok(types.SimpleNamespace(c=c, ref=dict(attn=attn))):
        return False
    if c.T == 1:
        return True
    x = _t(c.x)
    q = TF.conv1d(x, _t(c.wq)[:, :, None], _t(c.bq))
    k = TF.conv1d(x, _t(c.wk)[:, :, None], _t(c.bk))
    a32 = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=-1).numpy()
    shift = rel_err(R.softmax_scores(qk[:, :Cq], qk[:, Cq:], omit='key'), attn)
    return _margin(shift, rel_err(a32, attn)) > 4.0


def sa_weights(c):
    return c.wq, c.bq, c.wk, c.bk, c.wv, c.bv, c.gamma


def sa_torch(c, dtype, with_res=True, backward=True):
    """torch-CPU SelfAttention by conv1d / bmm / softmax, and autograd of <y, dy>."""
    leaf = {k: _t(getattr(c, k), dtype).requires_grad_(backward)
            for k in ('x', 'res', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv', 'gamma')}
    x = leaf['x']
    q = TF.conv1d(x, leaf['wq'][:, :, None], leaf['bq'])
    k = TF.conv1d(x, leaf['wk'][:, :, None], leaf['bk'])
    v = TF.conv1d(x, leaf['wv'][:, :, None], leaf['bv'])
    a = torch.softmax(torch.bmm(q.transpose(1, 2), k), dim=-1)
    y0 = leaf['gamma'] * torch.bmm(v, a.transpose(1, 2)) + x
    y = y0 + leaf['res'] if with_res else y0
    out = dict(qkv=_np(torch.cat([q, k, v], 1)), attn=_np(a), y=_np(y), y0=_np(y0))
    if backward:
        y.backward(_t(c.dy, dtype))
        for k_ in ('x', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv'):
            out['d' + k_] = _np(leaf[k_].grad)
        out['dres'] = _np(leaf['res'].grad) if with_res else None
        out['dgamma'] = float(leaf['gamma'].grad.item())
    return out


SA_GRADS = ('dx', 'dwq', 'dbq', 'dwk', 'dwv', 'dbv')      # tensors bounded by rel_err; dbk and dgamma apart


def sa_exact_zero(c):
    """The gradients whose exact value is 0 (compared with np.array_equal)."""
    if c.regime == 'gamma0':
        return ('dwq', 'dbq', 'dwk', 'dbk', 'dwv', 'dbv')
    return ('dwq', 'dbq', 'dwk', 'dbk') if c.T == 1 else ()


def sa_prepare(c):
    """Reference, torch-float32 errors and self-check shifts of one case, as scalars per quantity:
    p.ref[q] float64, p.e32[q] = rel_err(torch float32, ref), p.shift[q] = rel_err(ref without its
    omit term, ref).  y is held with the residual (ref['y']) and without (ref['y0'])."""
    w = sa_weights(c)
    Cq, g = c.C // 8, float(c.gamma[0])
    res = c.res.astype(np.float64)
    qkv, attn, y = R.self_attention(c.x, *w, res=c.res)
    ref = dict(qkv=qkv, attn=attn, y=y, y0=y - res)
    fomit = 'key' if c.T > 1 else 'channel'          # T = 1 has no key to lose
    sens = {}
    if fomit == 'key':      # the projection is untouched: only the softmax and PV are redone
        sens['qkv'] = rel_err(R.project(c.x, *R.stack_qkv(*w[:6]), omit='channel'), qkv)
        o_attn = R.softmax_scores(qkv[:, :Cq], qkv[:, Cq:2 * Cq], omit='key')
        o_y0 = g * np.matmul(qkv[:, 2 * Cq:], o_attn.transpose(0, 2, 1)) + c.x
    else:
        o_qkv, o_attn, o_y = R.self_attention(c.x, *w, res=c.res, omit='channel')
        sens['qkv'], o_y0 = rel_err(o_qkv, qkv), o_y - res
    sens['attn'] = rel_err(o_attn, attn)
    sens['y'] = rel_err(o_y0 + res, y)
    sens['y0'] = rel_err(o_y0, ref['y0'])
    t32 = sa_torch(c, torch.float32, True, backward=False)
    e32 = dict(qkv=rel_err(t32['qkv'], qkv), attn=rel_err(t32['attn'], attn), y=rel_err(t32['y'], y),
               y0=rel_err(t32['y0'], ref['y0']))
    return types.SimpleNamespace(c=c, ref=ref, e32=e32, shift=sens, fomit=fomit, bwd=False)


def sa_prepare_bwd(p):
    """The backward's part of sa_prepare, added to p."""
    c, w = p.c, sa_weights(p.c)
    g = R.self_attention_bwd(c.dy, c.x, *w, qkv=p.ref['qkv'], attn=p.ref['attn'])
    t32 = sa_torch(c, torch.float32, True)
    zero = sa_exact_zero(c)
    for q in SA_GRADS:
        p.ref[q] = g[q]
        p.e32[q] = rel_err(t32[q], g[q])
    p.ref['dbk'], p.ref['dgamma'] = g['dbk'], g['dgamma']
    p.dk_l1 = float(np.abs(g['dqkv'][:, c.C // 8:2 * (c.C // 8)]).sum())
    p.dbk32 = float(np.abs(t32['dbk']).max()) / max(p.dk_l1, 1e-300)      # torch float32's |dbk| / sum |dK|
    p.dgamma32 = abs(t32['dgamma'] - g['dgamma']) / max(abs(g['dgamma']), 1e-300)
    p.dgamma_cond = float(np.abs(g['rowdot']).sum()) / max(abs(g['dgamma']), 1e-300)
    if c.regime != 'gamma0':
        o = R.self_attention_bwd(c.dy, c.x, *w, qkv=p.ref['qkv'], attn=p.ref['attn'], omit='wrow')
        p.shift['dx'] = rel_err(o['dx'], g['dx'])
        o = R.self_attention_bwd(c.dy, c.x, *w, qkv=p.ref['qkv'], attn=p.ref['attn'], omit='outer')
        for q in SA_GRADS[1:]:
            if q not in zero:
                p.shift[q] = rel_err(o[q], g[q])
        p.dbk_shift = float(np.abs(o['dbk']).max()) / max(p.dk_l1, 1e-300)
    o = R.self_attention_bwd(c.dy, c.x, *w, qkv=p.ref['qkv'], attn=p.ref['attn'], omit='rowdot')
    p.dgamma_shift = abs(o['dgamma'] - g['dgamma']) / max(abs(g['dgamma']), 1e-300)
    p.bwd = True
    return p


def sa_regime_ok(p):
    """The softmax regime a case states: diffuse, every row's largest weight <= 4 / T; peaked, the
    median largest weight in [0.5, 0.95]."""
    top = p.ref['attn'].max(-1)
    if p.c.regime == 'diffuse':
        return bool(top.max() <= 4.0 / p.c.T)
    if p.c.regime == 'peaked':
        return bool(0.5 <= np.median(top) <= 0.95)
    return True


def sa_forward_margins(p):
    # gamma = 0: y is exact; T = 1: the attention matrix is 1, exactly
    qs = ['qkv'] + (['attn'] if p.c.T > 1 else []) + ([] if p.c.regime == 'gamma0' else ['y', 'y0'])
    return {q: _margin(p.shift[q], p.e32[q]) for q in qs}


def sa_backward_margins(p, e32_dgamma, dbk_pool):
    """Needs the module-wide figures, so it is no part of the seed condition's first stage."""
    m = {q: _margin(p.shift[q], p.e32[q]) for q in SA_GRADS if q in p.shift}
    m['dgamma'] = _margin(p.dgamma_shift, e32_dgamma)
    if hasattr(p, 'dbk_shift') and 'dbk' not in sa_exact_zero(p.c):
        m['dbk'] = _margin(p.dbk_shift, p.dbk32 if p.dbk32 > 0 else dbk_pool)
    return m


def dgamma_well_conditioned(p):
    """dgamma is a sum of B T signed rowdots: sum |rowdot| / |dgamma| is about 0.8 sqrt(B T) when the sum
    lands where a random walk typically does, and unbounded when it lands near 0.  A float32 sum's relative
    error grows with that ratio, and E32 is the largest over all cases, so one cancelled dgamma would
    loosen the bound of every case: a seed whose ratio exceeds 4 sqrt(B T) is passed over."""
    return p.dgamma_cond <= 4.0 * np.sqrt(p.c.B * p.c.T)


def _tensor_margins_ok(p):
    """The part of the seed condition that needs no module-wide figure."""
    return dgamma_well_conditioned(p) and all(_margin(p.shift[q], p.e32[q]) > 4.0 for q in SA_GRADS if q in p.shift)


def sa_case(B, C, T, regime='parity', variant=0, backward=True):
    return _sa_case(B, C, T, regime, variant, backward)


@functools.lru_cache(maxsize=None)
def _sa_case(B, C, T, regime, variant, backward):
    """The prepared case of the first seed from SEED_BASE + 1000 variant upwards that meets the input
    conditions: the regime, every forward self-check margin above 4 and, with `backward`, every
    tensor gradient's.  (dgamma's and dbk's margins rest on module-wide figures and are asserted, not
    searched.)  Variant g, a further problem of the grouped launch, has gamma = GAMMA + 0.2 g."""
    base = SEED_BASE + 1000 * variant
    for seed in range(base, base + SEED_TRIES):
        c = sa_make(B, C, T, regime, seed, GAMMA + 0.2 * variant, early=sa_attention_ok)
        if c is None:
            continue
        p = sa_prepare(c)
        if not (sa_regime_ok(p) and min(sa_forward_margins(p).values()) > 4.0):
            continue
        if backward and not _tensor_margins_ok(sa_prepare_bwd(p)):
            continue
        return p
    raise AssertionError(f'no seed meets the input conditions of {(B, C, T, regime, variant)}')


def sa_backward_keys():
    """Every case that runs a backward: the whole forward list, the regimes, gamma = 0, the direct shapes."""
    keys = [(s, 'parity') for s in SA_SHAPES]
    keys += [(s, r) for s in SA_REGIME_SHAPES for r in ('diffuse', 'peaked')]
    keys += [(s, 'gamma0') for s in SA_GAMMA0_SHAPES]
    keys += [(s, 'parity') for s in SA_DIRECT_SHAPES if s not in SA_SHAPES]
    return keys


def sa_forward_only_keys():
    keys = [(s, 'parity', 0) for s in FUSED_SHAPES if s not in SA_SHAPES]
    keys += [(GROUP_SHAPE, 'parity', g) for g in range(1, GROUP_G)]
    return keys


@functools.lru_cache(maxsize=None)
def sa_pooled():
    """(E32 of dgamma, pooled dbk figure): the largest relative error torch float32 makes on dgamma,
    and the largest |dbk| / sum |dK| it produces, over every backward case of the module."""
    ps = [sa_case(*s, r) for s, r in sa_backward_keys()]
    return max(p.dgamma32 for p in ps), max(p.dbk32 for p in ps)


# ------------------------------------------------------------------------------ SelfAttention: checks
def check_tensor(part, name, q, got, ref, e32, shift, fails):
    """rel_err(got) <= 8 rel_err(torch float32), and the reference that lost a term moved by > 4 x that."""
    got = np.asarray(got, dtype=np.float64)
    e_k = rel_err(got, ref)
    margin = None if shift is None else _margin(shift, e32)
    _record(part, name, q, e_k, e32, margin)
    if margin is not None and not margin > 4.0:
        fails.append(f'{q}: self-check margin {margin:.2f} <= 4')
    if not (np.isfinite(got).all() and e_k <= 8.0 * e32):
        fails.append(f'{q}: rel_err {e_k:.3e} > 8 x torch float32 {e32:.3e}')


def check_rows_sum_to_one(attn, T, fails):
    s = np.asarray(attn, dtype=np.float64).sum(-1)
    if not np.abs(s - 1.0).max() <= 4.0 * EPS32 * T:
        fails.append(f'attn rows sum to 1 +- {np.abs(s - 1.0).max():.3e} > 4 ulp x T')


def check_sa_forward(part, name, p, y, qkv, attn, with_res, fails):
    yk = 'y' if with_res else 'y0'
    if qkv is not None:
        check_tensor(part, name, 'qkv', qkv, p.ref['qkv'], p.e32['qkv'], p.shift['qkv'], fails)
        if p.c.T == 1:
            if not np.array_equal(attn, np.ones_like(attn)):
                fails.append('attn: T = 1 must give exactly 1')
        else:
            check_tensor(part, name, 'attn', attn, p.ref['attn'], p.e32['attn'], p.shift['attn'], fails)
        check_rows_sum_to_one(attn, p.c.T, fails)
    if p.c.regime == 'gamma0':
        want = p.c.x + p.c.res if with_res else p.c.x
        if not np.array_equal(y, want):
            fails.append('y: gamma = 0 must give x (+ res) bitwise')
    else:
        check_tensor(part, name, yk, y, p.ref[yk], p.e32[yk], p.shift[yk], fails)


def check_sa_backward(part, name, p, g, fails, skip=()):
    """g: dict of numpy gradients (dx, dwq, dbq, dwk, dbk, dwv, dbv, dgamma); `skip`: those not asked for."""
    c = p.c
    e32_dgamma, dbk_pool = sa_pooled()
    margins = sa_backward_margins(p, e32_dgamma, dbk_pool)
    zero = sa_exact_zero(c)
    for q in SA_GRADS:
        if q in skip:
            continue
        if q in zero:
            if not np.array_equal(g[q], np.zeros_like(g[q])):
                fails.append(f'{q}: must be exactly 0, max |.| = {np.abs(g[q]).max():.3e}')
        elif q == 'dx' and c.regime == 'gamma0':
            if not np.array_equal(g[q], c.dy):
                fails.append('dx: gamma = 0 must give dy bitwise')
        else:
            check_tensor(part, name, q, g[q], p.ref[q], p.e32[q], p.shift[q], fails)
    if 'dbk' not in skip:
        if 'dbk' in zero:
            if not np.array_equal(g['dbk'], np.zeros_like(g['dbk'])):
                fails.append(f'dbk: must be exactly 0, max |.| = {np.abs(g["dbk"]).max():.3e}')
        else:
            t32 = p.dbk32 if p.dbk32 > 0 else dbk_pool
            got = float(np.abs(np.asarray(g['dbk'], dtype=np.float64)).max()) / max(p.dk_l1, 1e-300)
            _record(part, name, 'dbk', got, t32, margins['dbk'])
            if not margins['dbk'] > 4.0:
                fails.append(f'dbk: self-check margin {margins["dbk"]:.2f} <= 4')
            if not (np.isfinite(g['dbk']).all() and got <= 8.0 * t32):
                fails.append(f'dbk: |dbk| / sum |dK| = {got:.3e} > 8 x torch float32 {t32:.3e}')
    ref = p.ref['dgamma']
    err = abs(float(g['dgamma']) - ref) / max(abs(ref), 1e-300)
    _record(part, name, 'dgamma', err, e32_dgamma, margins['dgamma'])
    if not margins['dgamma'] > 4.0:
        fails.append(f'dgamma: self-check margin {margins["dgamma"]:.2f} <= 4')
    if not (np.isfinite(g['dgamma']) and err <= 8.0 * e32_dgamma):
        fails.append(f'dgamma: relative error {err:.3e} > 8 x E32 {e32_dgamma:.3e}')


# ------------------------------------------------------------------------------ SelfAttention: GPU runs
def _strided(a, pad):
    """(buffer, [B][C][T] view of it) with `pad` sentinel floats after every clip."""
    B, C, T = a.shape
    buf = torch.full((B, C * T + pad), SENTINEL, device=DEV)
    view = buf[:, :C * T].unflatten(1, (C, T))
    view.copy_(_dev(a))
    return buf, view


def _pad_intact(buf, n):
    return bool((buf[:, n:] == SENTINEL).all().item())


def run_sa_forward(c, with_res, save=True, pad=0, fails=None):
    """F.self_attention on the case's inputs -> (y, qkv, attn) as numpy; save = False asks for the
    inference route (no intermediates)."""
    from a2m import functional as F
    n = c.C * c.T
    _, x = _strided(c.x, pad)
    rbuf, res = _strided(c.res, pad) if with_res else (None, None)
    ybuf, y = _strided(np.full_like(c.x, SENTINEL), pad)
    keep = {} if save else None
    out = F.self_attention(x, *[_dev(w) for w in sa_weights(c)], res=res, out=y, save=keep)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    if pad and fails is not None and not _pad_intact(ybuf, n):
        fails.append('y: the floats between the clips were written')
    return _np(y), (_np(keep['qkv']) if save else None), (_np(keep['attn']) if save else None)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_sa_unstacked(c):
    """a2m_self_attention_fwd_f32, the entry that stacks the three weights itself."""
    from a2m import _native as N
    B, C, T = c.B, c.C, c.T
    d = {k: _dev(getattr(c, k)) for k in ('x', 'res', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv', 'gamma')}
    y = torch.full((B, C, T), SENTINEL, device=DEV)
    qkv = torch.full((B, C // 4 + C, T), SENTINEL, device=DEV)
    attn = torch.full((B, T, T), SENTINEL, device=DEV)
    ws = torch.empty(64 << 20, dtype=torch.uint8, device=DEV)
    N.check(N.lib.a2m_self_attention_fwd_f32(
        _ptr(d['x']), C * T, B, C, T, _ptr(d['wq']), _ptr(d['bq']), _ptr(d['wk']), _ptr(d['bk']), _ptr(d['wv']),
        _ptr(d['bv']), _ptr(d['gamma']), _ptr(d['res']), _ptr(y), C * T, _ptr(qkv), _ptr(attn), _ptr(ws),
        ws.numel(), _stream()))
    torch.cuda.synchronize()
    return _np(y), _np(qkv), _np(attn)


def run_sa_backward(c, qkv, attn):
    """F.self_attention_bwd (the gradients packed, as the layer has them) on the forward's own qkv / attn."""
    from a2m import functional as F
    dx, g = F.self_attention_bwd(_dev(c.dy), _dev(c.x), tuple(_dev(w) for w in sa_weights(c)), _dev(qkv), _dev(attn))
    torch.cuda.synchronize()
    out = dict(zip(('dwq', 'dbq', 'dwk', 'dbk', 'dwv', 'dbv', 'dgamma'), (_np(t) for t in g)))
    out['dx'] = _np(dx)
    out['dgamma'] = float(out['dgamma'][0])
    return out


CANARY = 4096


def run_sa_backward_direct(c, qkv, attn, packed_w, packed_b, null=(), short=0):
    """a2m_self_attention_bwd_f32 itself.  Every output is prefilled with SENTINEL; the unpacked
    gradients lie in one buffer in the order v, k, q with 64 sentinel floats between them (never back to
    back); the workspace is exactly a2m_self_attention_bwd_ws_bytes long less `short`, and CANARY
    patterned bytes follow it in the same allocation.  -> (rc, gradients or None, complaints)."""
    from a2m import _native as N
    B, C, T, Cq = c.B, c.C, c.T, c.C // 8
    d = {k: _dev(getattr(c, k)) for k in ('x', 'dy', 'wq', 'bq', 'wk', 'bk', 'wv', 'bv', 'gamma')}
    d['qkv'], d['attn'] = _dev(qkv), _dev(attn)
    rows = dict(q=Cq, k=Cq, v=C)
    gap = 64

    def carve(width, packed):
        order = 'qkv' if packed else 'vkq'
        sizes = [rows[s] * width for s in order]
        buf = torch.full((sum(sizes) + (0 if packed else gap * 2),), SENTINEL, device=DEV)
        views, off = {}, 0
        for s, n in zip(order, sizes):
            views[s] = buf[off:off + n]
            off += n + (0 if packed else gap)
        return buf, views
    wbuf, dw = carve(C, packed_w)
    bbuf, db = carve(1, packed_b)
    dx = torch.full((B, C, T), SENTINEL, device=DEV)
    dg = torch.full((1,), SENTINEL, device=DEV)
    need = N.lib.a2m_self_attention_bwd_ws_bytes(B, C, T)
    pattern = (torch.arange(CANARY, device=DEV) % 251).to(torch.uint8)
    ws = torch.zeros(need + CANARY, dtype=torch.uint8, device=DEV)
    ws[need:] = pattern
    dbp = {s: (None if s in null else db[s]) for s in 'qkv'}
    rc = N.lib.a2m_self_attention_bwd_f32(
        _ptr(d['dy']), _ptr(d['x']), C * T, B, C, T, _ptr(d['wq']), _ptr(d['bq']), _ptr(d['wk']), _ptr(d['bk']),
        _ptr(d['wv']), _ptr(d['bv']), _ptr(d['gamma']), _ptr(d['qkv']), _ptr(d['attn']), _ptr(dx), _ptr(dw['q']),
        _ptr(dbp['q']), _ptr(dw['k']), _ptr(dbp['k']), _ptr(dw['v']), _ptr(dbp['v']), _ptr(dg), _ptr(ws),
        need - short, _stream())
    torch.cuda.synchronize()
    bad = []
    if not torch.equal(ws[need:], pattern):
        bad.append('the bytes after the workspace were written')
    if rc != 0:
        for name, t in (('dx', dx), ('dw', wbuf), ('db', bbuf), ('dgamma', dg)):
            if not bool((t == SENTINEL).all().item()):
                bad.append(f'{name} written by a refused call')
        return rc, None, bad
    g = dict(dx=_np(dx), dgamma=float(dg.item()))
    for s in 'qkv':
        g['dw' + s] = _np(dw[s]).reshape(rows[s], C)
        g['db' + s] = _np(db[s])
        if s in null and not np.all(g['db' + s] == SENTINEL):
            bad.append(f'db{s} written though NULL was passed')
    for name, arr, skip in [('dx', g['dx'], False), ('dgamma', np.array(g['dgamma']), False)] + \
            [('dw' + s, g['dw' + s], False) for s in 'qkv'] + [('db' + s, g['db' + s], s in null) for s in 'qkv']:
        if not skip and np.any(arr == SENTINEL):
            bad.append(f'{name}: the sentinel survives')
    for name, buf, views in (('dw', wbuf, dw), ('db', bbuf, db)):
        mask = torch.ones_like(buf, dtype=torch.bool)
        base = buf.data_ptr()
        for v in views.values():
            o = (v.data_ptr() - base) // 4
            mask[o:o + v.numel()] = False
        if not bool((buf[mask] == SENTINEL).all().item()):
            bad.append(f'{name}: the floats between the gradients were written')
    return rc, g, bad


# ------------------------------------------------------------------------------ SelfAttention: tests
def _sid(s):
    return 'x'.join(str(v) for v in s)


def _route(shape, keep=1):
    from a2m import _native as N
    return N.lib.a2m_self_attention_route(shape[1], shape[2], keep)


def _forward_and_backward(part, name, p, fails, pad=0):
    """The training route: forward with the intermediates saved, with and without res, then the
    backward on the saved qkv / attn."""
    c = p.c
    y, qkv, attn = run_sa_forward(c, True, pad=pad, fails=fails)
    check_sa_forward(part, name + '-res', p, y, qkv, attn, True, fails)
    y0, qkv0, attn0 = run_sa_forward(c, False, pad=pad, fails=fails)
    check_sa_forward(part, name, p, y0, qkv0, attn0, False, fails)
    if not (np.array_equal(qkv, qkv0) and np.array_equal(attn, attn0)):
        fails.append('qkv / attn differ with and without res')
    return qkv, attn


@pytest.mark.parametrize('shape', SA_SHAPES, ids=_sid)
def test_self_attention_train_route(shape, request):
    """Every route of a2m_self_attention_packed_fwd_f32 and the backward, at the parity test's scale."""
    want = 1 if shape in SA_CORE else 2 if shape in SA_WIDE else 0
    assert _route(shape) == want
    p = sa_case(*shape)
    fails, name = [], request.node.callspec.id
    qkv, attn = _forward_and_backward('1-sa-fwd', name, p, fails)
    check_sa_backward('2-sa-bwd', name, p, run_sa_backward(p.c, qkv, attn), fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('regime', ['diffuse', 'peaked'])
@pytest.mark.parametrize('shape', SA_REGIME_SHAPES, ids=_sid)
def test_self_attention_softmax_regimes(shape, regime, request):
    """Diffuse: every key matters (largest weight <= 4 / T).  Peaked: the median largest weight in
    [0.5, 0.95], so A (.) (G - rowdot) cancels and the non-maximal scores still count."""
    p = sa_case(*shape, regime)
    fails, name = [], request.node.callspec.id
    qkv, attn = _forward_and_backward('1-sa-regime', name, p, fails)
    check_sa_backward('2-sa-regime', name, p, run_sa_backward(p.c, qkv, attn), fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('shape,pad', SA_STRIDED, ids=[_sid(s) for s, _ in SA_STRIDED])
def test_self_attention_padded_batch_stride(shape, pad, request):
    """x, res and y as views into bigger buffers (batch stride C T + pad); the floats between stay."""
    p = sa_case(*shape)
    fails, name = [], request.node.callspec.id
    _forward_and_backward('1-sa-strided', name, p, fails, pad=pad)
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_self_attention_unstacked_entry_is_bitwise_packed():
    c = sa_case(*SA_UNSTACKED_SHAPE).c
    a = run_sa_forward(c, True)
    b = run_sa_unstacked(c)
    for q, u, v in zip(('y', 'qkv', 'attn'), a, b):
        assert np.array_equal(u, v), q


@pytest.mark.parametrize('shape', SA_GAMMA0_SHAPES, ids=_sid)
def test_self_attention_gamma_zero(shape, request):
    """The layer's initial value: y = x (+ res) and dx = dy bitwise, every weight and bias gradient
    exactly 0, dgamma against float64."""
    p = sa_case(*shape, 'gamma0')
    fails, name = [], request.node.callspec.id
    qkv, attn = _forward_and_backward('1-sa-gamma0', name, p, fails)
    check_sa_backward('2-sa-gamma0', name, p, run_sa_backward(p.c, qkv, attn), fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_self_attention_autograd_passes_dy_to_res():
    """The layer's autograd function: dres is dy itself, dx the backward entry's."""
    from a2m import autograd as AG
    p = sa_case(*SA_UNSTACKED_SHAPE)
    c = p.c
    x, res = _dev(c.x).requires_grad_(True), _dev(c.res).requires_grad_(True)
    y = AG._SelfAttn.apply(x, res, *[_dev(w) for w in sa_weights(c)])
    y.backward(_dev(c.dy))
    torch.cuda.synchronize()
    assert np.array_equal(_np(res.grad), c.dy)
    fails = []
    check_tensor('2-sa-autograd', _sid(SA_UNSTACKED_SHAPE), 'dx', _np(x.grad), p.ref['dx'], p.e32['dx'], p.shift['dx'], fails)
    assert not fails, '; '.join(fails)


DIRECT_VARIANTS = [(True, True, ()), (False, False, ()), (True, False, ()), (False, True, ()),
                   (True, False, ('q',)), (True, False, ('k',)), (False, False, ('v',)), (True, False, ('q', 'k', 'v')),
                   (False, False, ('q', 'k', 'v'))]


@pytest.mark.parametrize('shape', SA_DIRECT_SHAPES, ids=_sid)
def test_self_attention_backward_direct_entry(shape, request):
    """a2m_self_attention_bwd_f32: packed and unpacked dw and db, NULL bias gradients, outputs
    overwritten and not added to, a workspace of exactly the stated size, one byte less refused."""
    from a2m import _native as N
    p = sa_case(*shape)
    _, qkv, attn = run_sa_forward(p.c, False)
    fails, name = [], request.node.callspec.id
    for packed_w, packed_b, null in DIRECT_VARIANTS:
        tag = f'{name}-w{int(packed_w)}b{int(packed_b)}' + ''.join(null)
        rc, g, bad = run_sa_backward_direct(p.c, qkv, attn, packed_w, packed_b, null)
        fails += [f'{tag}: {b}' for b in bad]
        if rc != 0:
            fails.append(f'{tag}: rc {rc} {N.last_error()}')
            continue
        sub = []
        check_sa_backward('2-sa-direct', tag, p, g, sub, skip=tuple('db' + s for s in null))
        fails += [f'{tag}: {s}' for s in sub]
    rc, _, bad = run_sa_backward_direct(p.c, qkv, attn, True, True, short=1)
    if rc != N.A2M_EWS:
        fails.append(f'a workspace one byte short gave rc {rc}')
    fails += bad
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('shape', FUSED_SHAPES, ids=_sid)
def test_self_attention_fused_eval(shape, request):
    """a2m_self_attention_eval_ex_f32 (no save, fp32 operands) with and without res, with a padded
    batch stride, and with V chunks of 64 and 128 channels (bitwise equal)."""
    from a2m import _native as N
    assert _route(shape, 0) == 3 and N.lib.a2m_get_gemm_precision() == 0
    p = sa_case(*shape, backward=shape in SA_SHAPES)
    fails, name = [], request.node.callspec.id
    outs = {}
    try:
        for nv in (64, 128):
            N.check(N.lib.a2m_set_attn_eval_chunk(nv))
            for with_res in (True, False):
                for pad in (0, FUSED_PAD):
                    y, _, _ = run_sa_forward(p.c, with_res, save=False, pad=pad, fails=fails)
                    outs[nv, with_res, pad] = y
                    check_sa_forward('3-sa-fused', f'{name}-nv{nv}-res{int(with_res)}-pad{pad}', p, y, None, None,
                                     with_res, fails)
    finally:
        N.check(N.lib.a2m_set_attn_eval_chunk(64))
    for with_res in (True, False):
        for key in ((128, with_res, 0), (64, with_res, FUSED_PAD), (128, with_res, FUSED_PAD)):
            if not np.array_equal(outs[64, with_res, 0], outs[key]):
                fails.append(f'chunk / stride {key} is not bitwise the chunk-64 dense result')
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('with_res', [True, False])
def test_self_attention_eval_group(with_res):
    """G = 3 problems of distinct inputs, weights and gamma in one launch, each against float64."""
    from a2m import functional as F
    B, C, T = GROUP_SHAPE
    ps = [sa_case(B, C, T, 'parity', g, backward=False) for g in range(GROUP_G)]
    xs = torch.stack([_dev(p.c.x) for p in ps])
    res = torch.stack([_dev(p.c.res) for p in ps]) if with_res else None
    out = torch.full((GROUP_G, B, C, T), SENTINEL, device=DEV)
    st = [F.stacked_qkv(*[_dev(w) for w in sa_weights(p.c)[:6]]) for p in ps]
    F.self_attention_group(list(xs), torch.stack([s[0] for s in st]), torch.stack([s[1] for s in st]),
                           _dev(np.concatenate([p.c.gamma for p in ps])), list(out),
                           res=list(res) if with_res else None)
    torch.cuda.synchronize()
    fails = []
    for g, p in enumerate(ps):
        check_sa_forward('3-sa-group', f'g{g}-res{int(with_res)}', p, _np(out[g]), None, None, with_res, fails)
    assert not fails, '; '.join(fails)


# ------------------------------------------------------------------------------ ChannelAttention: inputs
def ca_make(B, C, T, Cr, kind, seed):
    """kind: 'plain', 'ties' (four channels of every clip rewritten, see ca_expected_ties), 'mlp' (one
    hidden unit exactly 0 and one negative for both pools, two saturated sigmoids) or 'grid' (x on a grid
    of 1/16 so that every pooling sum is exact in any order)."""
    rng = np.random.default_rng(seed)

    def r(*shape, scale=1.0):
        return (rng.standard_normal(shape) * scale).astype(F32)
    c = types.SimpleNamespace(B=B, C=C, T=T, Cr=Cr, kind=kind, seed=seed, x=r(B, C, T), dy=r(B, C, T),
                              w1=r(Cr, C, scale=C ** -0.5), b1=r(Cr, scale=0.1), w2=r(C, Cr, scale=Cr ** -0.5),
                              b2=r(C, scale=0.1))
    if kind == 'grid':
        c.x = (rng.integers(-64, 65, (B, C, T)) / 16.0).astype(F32)
    if kind == 'ties':
        top = F32(np.ceil(np.abs(c.x).max()) + 1.0)
        c.x[:, TIE_ZERO] = 0.0
        c.x[:, TIE_LANES, 5] = c.x[:, TIE_LANES, 8] = top
        c.x[:, TIE_SAME, 3] = c.x[:, TIE_SAME, 11] = top
        c.x[:, TIE_LAST, T - 1] = top
    if kind == 'mlp':
        c.w1[DEAD_ZERO], c.b1[DEAD_ZERO] = 0.0, 0.0
        c.w1[DEAD_NEG], c.b1[DEAD_NEG] = 0.0, -1.0
        c.w2[SAT_HI], c.b2[SAT_HI] = 0.0, 15.0
        c.w2[SAT_LO], c.b2[SAT_LO] = 0.0, -15.0
    return c


def ca_expected_ties(c):
    """[B][C] how many t hold the row's maximum, and [B][C] the first of them, as the case claims (-1
    where the case leaves it to the random draw)."""
    count = np.ones((c.B, c.C), dtype=np.int64)
    first = -np.ones((c.B, c.C), dtype=np.int64)
    if c.kind == 'ties':
        count[:, TIE_ZERO], first[:, TIE_ZERO] = c.T, 0
        count[:, TIE_LANES], first[:, TIE_LANES] = 2, 5
        count[:, TIE_SAME], first[:, TIE_SAME] = 2, 3
        count[:, TIE_LAST], first[:, TIE_LAST] = 1, c.T - 1
    return count, first


def ca_weights(c):
    return c.w1, c.b1, c.w2, c.b2


def ca_torch(c, dtype, backward=True):
    """torch-CPU ChannelAttention with F.adaptive_max_pool1d (the reference layer's pool: a tie's whole
    gradient goes to the first maximum), and autograd of <y, dy>."""
    leaf = {k: _t(getattr(c, k), dtype).requires_grad_(backward) for k in ('x', 'w1', 'b1', 'w2', 'b2')}
    x = leaf['x']

    def mlp(z):
        return torch.sigmoid(TF.linear(TF.relu(TF.linear(z, leaf['w1'], leaf['b1'])), leaf['w2'], leaf['b2']))
    att = mlp(x.mean(-1)) + mlp(TF.adaptive_max_pool1d(x, 1).squeeze(-1))
    y = x * att.unsqueeze(-1)
    out = dict(att=_np(att), y=_np(y))
    if backward:
        y.backward(_t(c.dy, dtype))
        out.update({'d' + k: _np(v.grad) for k, v in leaf.items()})
    return out


CA_FWD = ('att', 'y')
CA_GRADS = ('dx', 'dw1', 'db1', 'dw2', 'db2')


def ca_prepare(c, backward=True):
    w = ca_weights(c)
    parts = R.channel_attention_parts(c.x, *w)
    ref = dict(att=parts['att'], y=parts['y'])
    t32 = ca_torch(c, torch.float32, backward)
    o_att, o_y = R.channel_attention(c.x, *w, omit='time')
    shift = dict(att=rel_err(o_att, ref['att']), y=rel_err(o_y, ref['y']))
    if backward:
        ref.update(R.channel_attention_bwd(c.dy, c.x, *w))
        shift['dx'] = rel_err(R.channel_attention_bwd(c.dy, c.x, *w, omit='time')['dx'], ref['dx'])
        o = R.channel_attention_bwd(c.dy, c.x, *w, omit='clip')
        shift.update({q: rel_err(o[q], ref[q]) for q in CA_GRADS[1:]})
    e32 = {q: rel_err(t32[q], ref[q]) for q in ref}
    pre = parts['pre']
    live = np.ones(pre.shape[-1], dtype=bool)
    if c.kind == 'mlp':
        live[[DEAD_ZERO, DEAD_NEG]] = False
    kink = float(np.abs(pre[..., live]).min() / np.abs(pre).max()) if live.any() else 1.0
    return types.SimpleNamespace(c=c, ref=ref, e32=e32, shift=shift, kink=kink, parts=parts, bwd=backward)


def ca_margins(p):
    return {q: _margin(p.shift[q], p.e32[q]) for q in p.shift}


def ca_ok(p):
    """Every live hidden pre-activation at least 1e-4 of the largest from the ReLU kink, every margin above 4."""
    return p.kink >= 1e-4 and min(ca_margins(p).values()) > 4.0


def ca_case(B, C, T, Cr, kind='plain', backward=True):
    return _ca_case(B, C, T, Cr, kind, backward)


@functools.lru_cache(maxsize=None)
def _ca_case(B, C, T, Cr, kind, backward):
    for seed in range(SEED_BASE, SEED_BASE + SEED_TRIES):
        p = ca_prepare(ca_make(B, C, T, Cr, kind, seed), backward)
        if ca_ok(p):
            return p
    raise AssertionError(f'no seed meets the input conditions of {(B, C, T, Cr, kind)}')


# ------------------------------------------------------------------------------ ChannelAttention: GPU runs
def run_ca_forward(c, in_place=False, offset=0):
    """F.channel_attention -> (att, y); offset: x and y start `offset` floats into their allocations."""
    from a2m import functional as F
    n = c.B * c.C * c.T

    def place(a):
        buf = torch.full((n + offset + 4,), SENTINEL, device=DEV)
        v = buf[offset:offset + n].view(c.B, c.C, c.T)
        v.copy_(_dev(a))
        return buf, v
    xbuf, x = place(c.x)
    ybuf, y = (xbuf, x) if in_place else place(np.full_like(c.x, SENTINEL))
    assert x.data_ptr() % 16 == 4 * (offset % 4) and x.is_contiguous()
    att = torch.full((c.B, c.C), SENTINEL, device=DEV)
    out = F.channel_attention(x, *[_dev(w) for w in ca_weights(c)], out=y, att=att)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    assert bool((ybuf[:offset] == SENTINEL).all().item()) and bool((ybuf[offset + n:] == SENTINEL).all().item())
    return _np(att), _np(y)


def run_ca_backward(c):
    from a2m import functional as F
    dx, g = F.channel_attention_bwd(_dev(c.dy), _dev(c.x), *[_dev(w) for w in ca_weights(c)])
    torch.cuda.synchronize()
    out = dict(zip(CA_GRADS[1:], (_np(t) for t in g)))
    out['dx'] = _np(dx)
    return out


def check_ca(part, name, p, got, qs, fails):
    for q in qs:
        check_tensor(part, name, q, got[q], p.ref[q], p.e32[q], p.shift[q], fails)


# ------------------------------------------------------------------------------ ChannelAttention: tests
@pytest.mark.parametrize('shape', CA_SHAPES, ids=_sid)
def test_channel_attention(shape, request):
    """Forward and backward; (3, 256, 64, 32) is the fused forward kernel, run in place too.  At
    (1, 8, 1, 1) db1 and dw1 hang on one 8-term sum that cancels 24-fold (module docstring)."""
    p = ca_case(*shape)
    fails, name = [], request.node.callspec.id
    att, y = run_ca_forward(p.c)
    check_ca('4-ca-fwd', name, p, dict(att=att, y=y), CA_FWD, fails)
    if shape == CA_FUSED_SHAPE:
        att2, y2 = run_ca_forward(p.c, in_place=True)
        if not (np.array_equal(att, att2) and np.array_equal(y, y2)):
            fails.append('in place differs from out of place')
    check_ca('5-ca-bwd', name, p, run_ca_backward(p.c), CA_GRADS, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


@pytest.mark.parametrize('kind', ['ties', 'mlp'])
@pytest.mark.parametrize('shape', CA_SPECIAL_SHAPES, ids=_sid)
def test_channel_attention_ties_and_mlp_edges(shape, kind, request):
    """ties: an all-zero channel, a maximum at t = 5 and 8 (two lanes of the backward's 8-lane group, the
    later lane holding the earlier index), at t = 3 and 11 (one lane) and at T - 1; the whole gradient
    of the max pool goes to the first maximum.  mlp: a hidden unit exactly 0 and one negative for both
    pools (relu' = 0), and sigmoids saturated at logits of +-15."""
    p = ca_case(*shape, kind)
    fails, name = [], request.node.callspec.id
    att, y = run_ca_forward(p.c)
    check_ca('4-ca-edge', name, p, dict(att=att, y=y), CA_FWD, fails)
    check_ca('5-ca-edge', name, p, run_ca_backward(p.c), CA_GRADS, fails)
    assert not fails, f'{name}: ' + '; '.join(fails)


def test_channel_attention_offset_view_is_bitwise_aligned(request):
    """x and y one float into their allocations at T % 4 == 0: the generic path must leave its float4
    loads and stores for the scalar loop.  The inputs lie on a grid of 1/16, so the pooled sums are
    exact in either order and the two results must agree bitwise."""
    p = ca_case(*CA_OFFSET_SHAPE, 'grid', backward=False)
    fails = []
    att, y = run_ca_forward(p.c)
    check_ca('4-ca-offset', 'aligned', p, dict(att=att, y=y), CA_FWD, fails)
    for off in (1, 2, 3):
        att1, y1 = run_ca_forward(p.c, offset=off)
        if not (np.array_equal(att, att1) and np.array_equal(y, y1)):
            fails.append(f'offset {off} differs from the aligned result')
    assert not fails, '; '.join(fails)


def test_channel_attention_backward_refuses_offset_dy():
    from a2m import functional as F, _native as N
    c = ca_case(*CA_OFFSET_SHAPE, 'grid', backward=False).c
    n = c.B * c.C * c.T
    buf = torch.zeros(n + 4, device=DEV)
    dy = buf[1:1 + n].view(c.B, c.C, c.T)
    x, dx = _dev(c.x), torch.full((c.B, c.C, c.T), SENTINEL, device=DEV)
    w = [_dev(a) for a in ca_weights(c)]
    g = [torch.full_like(a, SENTINEL) for a in w]
    ws = F.WS.get(DEV, 4 * c.B * (2 * c.Cr * c.C + c.Cr + c.C))
    rc = N.lib.a2m_channel_attention_bwd_f32(_ptr(dy), _ptr(x), c.B, c.C, c.T, _ptr(w[0]), _ptr(w[1]), c.Cr, _ptr(w[2]),
                                             _ptr(w[3]), _ptr(dx), *[_ptr(a) for a in g], _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == N.A2M_EINVAL and 'aligned' in N.last_error()
    assert bool((dx == SENTINEL).all().item()) and all(bool((a == SENTINEL).all().item()) for a in g)


def test_channel_attention_forward_takes_2048_channels(request):
    """The forward's LDS holds C = 2048 (the backward's does not: tests/test_attn_ref_cpu.py)."""
    p = ca_case(*CA_WIDE_SHAPE, backward=False)
    fails = []
    att, y = run_ca_forward(p.c)
    check_ca('4-ca-wide', _sid(CA_WIDE_SHAPE), p, dict(att=att, y=y), CA_FWD, fails)
    assert not fails, '; '.join(fails)


# ------------------------------------------------------------------------------ for the CPU module
def cases():
    """Every input the tests here draw, for tests/test_attn_ref_cpu.py: the references are proved and
    the input conditions checked at exactly these."""
    sa = [sa_case(*s, r) for s, r in sa_backward_keys()]
    sa += [sa_case(*s, r, v, backward=False) for s, r, v in sa_forward_only_keys()]
    ca = [ca_case(*s) for s in CA_SHAPES] + [ca_case(*s, k) for s in CA_SPECIAL_SHAPES for k in ('ties', 'mlp')]
    ca += [ca_case(*CA_OFFSET_SHAPE, 'grid', backward=False), ca_case(*CA_WIDE_SHAPE, backward=False)]
    return dict(sa=sa, ca=ca, fused=FUSED_SHAPES, group=GROUP_SHAPE, core=SA_CORE, wide=SA_WIDE, general=SA_GENERAL)
