"""tests/attn_ref.py proved against torch float64 autograd at every case tests/test_gpu_attention_fp64.py
uses, the input conditions of those cases, the coverage of a2m_self_attention_route by them, and the
argument checks of the attention entry points that return before any launch.  No GPU here.

The argument checks pass host memory as the operands: every call made here is refused by a check that
stands before the entry's first launch or copy (read in csrc/ops.hip and csrc/train_attn.hip), so the
memory is never touched.  An entry whose refusal comes later -- a2m_self_attention_fwd_f32 stacks the
weights before it looks at B and T -- is asked only what it refuses at once."""
import ctypes

import numpy as np
import pytest
import torch

import attn_ref as R
import test_gpu_attention_fp64 as G
from conftest import rel_err

CASES = G.cases()
TOL64 = 1e-12


def _id(p):
    c = p.c
    tail = f'-{c.regime}-s{c.seed}' if hasattr(c, 'regime') else f'x{c.Cr}-{c.kind}-s{c.seed}'
    return f'{c.B}x{c.C}x{c.T}{tail}'


# ------------------------------------------------------------------------------ attn_ref against torch float64
@pytest.mark.parametrize('p', CASES['sa'], ids=_id)
def test_self_attention_ref_matches_torch_float64(p):
    c = p.c
    t = G.sa_torch(c, torch.float64, True, backward=p.bwd)
    qkv, attn, y = R.self_attention(c.x, *G.sa_weights(c), res=c.res)
    for q, a in (('qkv', qkv), ('attn', attn), ('y', y)):
        assert rel_err(a, t[q]) <= TOL64, q
    assert rel_err(R.self_attention(c.x, *G.sa_weights(c))[2], G.sa_torch(c, torch.float64, False, False)['y']) <= TOL64
    if not p.bwd:
        return
    g = R.self_attention_bwd(c.dy, c.x, *G.sa_weights(c))
    for q in ('dx', 'dres', 'dwq', 'dbq', 'dwk', 'dwv', 'dbv'):
        assert rel_err(g[q], t[q]) <= TOL64, q
    # dbk is 0 up to rounding in either; both are measured against the sum they cancel from
    scale = max(np.abs(g['dqkv'][:, c.C // 8:c.C // 4]).sum(), 1e-300)
    assert np.abs(g['dbk']).max() <= TOL64 * scale and np.abs(t['dbk']).max() <= TOL64 * scale
    assert abs(g['dgamma'] - t['dgamma']) <= TOL64 * abs(t['dgamma'])
    for q in G.sa_exact_zero(c):
        assert not g[q].any() and not t[q].any(), q


@pytest.mark.parametrize('p', CASES['ca'], ids=_id)
def test_channel_attention_ref_matches_torch_float64(p):
    c = p.c
    t = G.ca_torch(c, torch.float64, backward=p.bwd)
    att, y = R.channel_attention(c.x, *G.ca_weights(c))
    assert rel_err(att, t['att']) <= TOL64 and rel_err(y, t['y']) <= TOL64
    if p.bwd:
        g = R.channel_attention_bwd(c.dy, c.x, *G.ca_weights(c))
        for q in G.CA_GRADS:
            assert rel_err(g[q], t[q]) <= TOL64, q


def test_max_pool_gradient_goes_to_the_first_maximum():
    """[0, 2, 2, 1] -> [0, 1, 0, 0] and a constant row -> [1, 0, 0, 0], in torch's adaptive max pool,
    in the oracle and in attn_ref; amax would split the gradient evenly."""
    from oracle import model as OM
    x = np.array([[[0, 2, 2, 1], [3, 3, 3, 3]]], dtype=np.float64)
    w1, b1, w2, b2 = np.eye(2), np.ones(2), np.eye(2), np.zeros(2)
    dy = np.ones_like(x)
    g = R.channel_attention_bwd(dy, x, w1, b1, w2, b2)['dx']
    sd = {'c.fc.0.weight': torch.from_numpy(w1), 'c.fc.0.bias': torch.from_numpy(b1),
          'c.fc.2.weight': torch.from_numpy(w2), 'c.fc.2.bias': torch.from_numpy(b2)}
    xt = torch.from_numpy(x).requires_grad_(True)
    OM.channel_attention(OM.Ctx(sd), 'c', xt).backward(torch.from_numpy(dy))
    assert rel_err(g, xt.grad.numpy()) <= TOL64
    # dy att and the average pool's share are the same at every t of a row: what differs is the max pool's
    assert g[0, 0, 1] != g[0, 0, 2] and g[0, 0, 2] == g[0, 0, 3] == g[0, 0, 0]
    assert g[0, 1, 0] != g[0, 1, 1] and g[0, 1, 1] == g[0, 1, 2] == g[0, 1, 3]
    t = torch.tensor([[[0., 2., 2., 1.], [3., 3., 3., 3.]]], dtype=torch.float64, requires_grad=True)
    torch.nn.functional.adaptive_max_pool1d(t, 1).sum().backward()
    assert t.grad.tolist() == [[[0, 1, 0, 0], [1, 0, 0, 0]]]


# ------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize('p', CASES['sa'], ids=_id)
def test_self_attention_case_conditions(p):
    c = p.c
    assert G.sa_regime_ok(p)
    top = p.ref['attn'].max(-1)
    print(f'COND {_id(p)} median top weight {np.median(top):.3f} largest {top.max():.3f} (4/T = {4 / c.T:.3f})')
    m = G.sa_forward_margins(p)
    if p.bwd:
        m.update({'bwd-' + k: v for k, v in G.sa_backward_margins(p, *G.sa_pooled()).items()})
    print(f'MARGIN {_id(p)} ' + ' '.join(f'{k}={v:.1f}' for k, v in m.items()))
    assert min(m.values()) > 4.0, m
    base = G.SEED_BASE + 1000 * ((c.seed - G.SEED_BASE) // 1000)
    assert base <= c.seed < base + G.SEED_TRIES
    if c.T > 1:
        assert p.fomit == 'key'
    zero = G.sa_exact_zero(c)
    if p.bwd:
        assert G.dgamma_well_conditioned(p)
        for q in G.SA_GRADS:
            assert (q in p.shift) != (q in zero or (q == 'dx' and c.regime == 'gamma0')), q


def test_self_attention_seeds_are_the_first_that_meet_the_conditions():
    """The search itself, replayed on the two cheapest cases: no earlier seed passes."""
    for key in ((3, 16, 5), (2, 128, 33)):
        p = G.sa_case(*key)
        for seed in range(G.SEED_BASE, p.c.seed):
            q = G.sa_prepare(G.sa_make(*key, 'parity', seed))
            assert not (min(G.sa_forward_margins(q).values()) > 4.0 and G._tensor_margins_ok(G.sa_prepare_bwd(q))), seed


def test_self_attention_pooled_figures():
    e32, dbk = G.sa_pooled()
    print(f'POOLED E32(dgamma)={e32:.3e} dbk={dbk:.3e}')
    assert 0 < e32 < 1e-4 and 0 < dbk < 1e-4


@pytest.mark.parametrize('p', CASES['ca'], ids=_id)
def test_channel_attention_case_conditions(p):
    c = p.c
    assert p.kink >= 1e-4
    m = G.ca_margins(p)
    print(f'MARGIN {_id(p)} kink={p.kink:.2e} ' + ' '.join(f'{k}={v:.1f}' for k, v in m.items()))
    assert min(m.values()) > 4.0, m
    count, first = G.ca_expected_ties(c)
    mx = c.x.max(-1, keepdims=True)
    if c.kind != 'grid':            # a grid holds ties by nature; its case runs no backward
        assert np.array_equal((c.x == mx).sum(-1), count)
    got = (c.x == mx).argmax(-1)
    assert np.array_equal(got[first >= 0], first[first >= 0])
    assert np.array_equal(p.parts['argmax'], got)
    if c.kind == 'ties':
        assert not c.x[:, G.TIE_ZERO].any() and c.T > 11
    if c.kind == 'mlp':
        pre, z = p.parts['pre'], np.log(p.parts['s'] / (1 - p.parts['s']))
        assert not pre[..., G.DEAD_ZERO].any() and (pre[..., G.DEAD_NEG] == -1).all()
        assert np.allclose(z[..., G.SAT_HI], 15, atol=1e-6) and np.allclose(z[..., G.SAT_LO], -15, atol=1e-6)
    if c.kind == 'grid':
        assert np.array_equal(c.x * 16, np.round(c.x * 16)) and np.abs(c.x).max() <= 4


def test_every_omit_term_is_a_term():
    """Each name removes something from the sum it belongs to and nothing from the others."""
    c = G.sa_case(3, 16, 5).c
    w = G.sa_weights(c)
    base = R.self_attention(c.x, *w, res=c.res)
    key = R.self_attention(c.x, *w, res=c.res, omit='key')
    assert np.array_equal(key[0], base[0]) and key[1][-1, -1, -1] == 0 and abs(key[1][-1, -1].sum() - 1) < 1e-15
    assert np.array_equal(key[1][:-1], base[1][:-1]) and np.array_equal(key[2][:-1], base[2][:-1])
    assert not np.array_equal(key[2][-1, :, -1], base[2][-1, :, -1])
    ch = R.self_attention(c.x, *w, res=c.res, omit='channel')
    assert np.abs(ch[0] - base[0]).min() > 0
    g = R.self_attention_bwd(c.dy, c.x, *w)
    for omit, moved in (('outer', ('dwq', 'dbq', 'dwk', 'dbk', 'dwv', 'dbv')), ('wrow', ('dx',)), ('rowdot', ('dgamma',))):
        o = R.self_attention_bwd(c.dy, c.x, *w, omit=omit)
        for q in ('dx', 'dwq', 'dbq', 'dwk', 'dbk', 'dwv', 'dbv', 'dgamma'):
            assert np.array_equal(o[q], g[q]) != (q in moved), (omit, q)
    k = G.ca_case(2, 12, 7, 3).c
    kw = G.ca_weights(k)
    gb = R.channel_attention_bwd(k.dy, k.x, *kw)
    o = R.channel_attention_bwd(k.dy, k.x, *kw, omit='clip')
    assert np.array_equal(o['dx'], gb['dx']) and all(not np.array_equal(o[q], gb[q]) for q in G.CA_GRADS[1:])
    assert not np.array_equal(R.channel_attention(k.x, *kw, omit='time')[0], R.channel_attention(k.x, *kw)[0])


# ------------------------------------------------------------------------------ route coverage
def test_route_coverage():
    """a2m_self_attention_route at every case: each kernel at every C/8 and edge T the module promises."""
    from a2m import _native as N
    route = N.lib.a2m_self_attention_route
    seen = {r: set() for r in range(4)}
    for p in CASES['sa']:
        if p.bwd:
            seen[route(p.c.C, p.c.T, 1)].add((p.c.C, p.c.T))
    for B, C, T in CASES['fused'] + [CASES['group']]:
        assert N.lib.a2m_self_attention_eval_fits(C, T) == 1
        seen[route(C, T, 0)].add((C, T))
    for name, want in (('core', 1), ('wide', 2), ('general', 0)):
        for B, C, T in CASES[name]:
            assert route(C, T, 1) == want, (name, C, T)
    print('ROUTES ' + ' | '.join(f'{r}: {sorted(v)}' for r, v in seen.items()))
    core, wide, general, fused = seen[1], seen[2], seen[0], seen[3]
    assert {C // 8 for C, T in core} == {16, 32, 48, 64}
    assert any(T % 2 == 1 and T > 1 for C, T in core) and any(T == 1 for C, T in core) and any(T == 64 for C, T in core)
    assert {C // 8 for C, T in wide} == {128, 192, 256}
    assert {4, 32} <= {T for C, T in wide}
    assert any((C // 8) % 16 != 0 for C, T in general)
    assert any(C == 256 and T > 64 for C, T in general)
    assert any(C == 2048 and T % 4 != 0 and T <= 32 for C, T in general)
    assert any(C == 2048 and T > 32 and T % 4 == 0 for C, T in general)
    assert {C for C, T in fused} == {128, 256} and {4, 64} <= {T for C, T in fused}
    # keep = 0 returns 3 exactly where the fused kernel fits; bad shapes name the general path
    for C in (8, 64, 128, 256, 512, 2048):
        for T in (1, 4, 6, 64, 68):
            fits = N.lib.a2m_self_attention_eval_fits(C, T) == 1
            assert (route(C, T, 0) == 3) == fits
            assert route(C, T, 1) != 3 and (fits or route(C, T, 0) == route(C, T, 1))
    assert route(12, 4, 1) == 0 and route(0, 4, 0) == 0 and route(128, 0, 0) == 0


# ------------------------------------------------------------------------------ argument checks
def _host(n=64):
    return (ctypes.c_float * n)()


def _sa_fwd_packed(N, h, **kw):
    a = dict(x=h, x_bs=128 * 4, B=2, C=128, T=4, w=h, b=h, gamma=h, res=None, y=h, y_bs=128 * 4, qkv=h, attn=h,
             ws=None, ws_bytes=0)
    a.update(kw)
    return N.lib.a2m_self_attention_packed_fwd_f32(a['x'], a['x_bs'], a['B'], a['C'], a['T'], a['w'], a['b'], a['gamma'],
                                                   a['res'], a['y'], a['y_bs'], a['qkv'], a['attn'], a['ws'],
                                                   a['ws_bytes'], None)


def _sa_bwd(N, h, **kw):
    a = dict(dy=h, x=h, B=2, C=128, T=4, wq=h, wk=h, wv=h, gamma=h, qkv=h, attn=h, dx=h, dwq=h, dwk=h, dwv=h,
             dgamma=h, ws=None, ws_bytes=0)
    a.update(kw)
    return N.lib.a2m_self_attention_bwd_f32(a['dy'], a['x'], a['C'] * a['T'], a['B'], a['C'], a['T'], a['wq'], h, a['wk'], h,
                                            a['wv'], h, a['gamma'], a['qkv'], a['attn'], a['dx'], a['dwq'], None,
                                            a['dwk'], None, a['dwv'], None, a['dgamma'], a['ws'], a['ws_bytes'], None)


def test_self_attention_argument_checks():
    from a2m import _native as N
    h = _host()
    for kw in (dict(C=12), dict(C=4), dict(C=0), dict(T=0), dict(T=-1), dict(B=0), dict(B=-2), dict(x=None),
               dict(w=None), dict(b=None), dict(gamma=None), dict(y=None), dict(qkv=None), dict(attn=None),
               dict(y_bs=128 * 4 + 4)):
        assert _sa_fwd_packed(N, h, **kw) == N.A2M_EINVAL, kw
        assert 'self_attention' in N.last_error()
    for kw in (dict(C=12), dict(C=4), dict(T=0), dict(B=0), dict(dy=None), dict(x=None), dict(wq=None), dict(wk=None),
               dict(wv=None), dict(gamma=None), dict(qkv=None), dict(attn=None), dict(dx=None), dict(dwq=None),
               dict(dwk=None), dict(dwv=None), dict(dgamma=None)):
        assert _sa_bwd(N, h, ws=h, ws_bytes=1 << 40, **kw) == N.A2M_EINVAL, kw
    need = N.lib.a2m_self_attention_bwd_ws_bytes(2, 128, 4)
    assert need > 0
    for ws, nbytes in ((None, need), (h, 0), (h, need - 1)):
        assert _sa_bwd(N, h, ws=ws, ws_bytes=nbytes) == N.A2M_EWS
        assert 'workspace too small' in N.last_error()
    # the unstacked entry: NULL operands and C at once, then the room for the stacked weights
    f = N.lib.a2m_self_attention_fwd_f32
    args = [h, 512, 2, 128, 4, h, h, h, h, h, h, h, None, h, 512, h, h, None, 0, None]
    for i in (0, 5, 7, 9, 11, 13, 15, 16):
        bad = list(args)
        bad[i] = None
        assert f(*bad) == N.A2M_EINVAL, i
    for C in (12, 4, 0):
        bad = list(args)
        bad[3] = C
        assert f(*bad) == N.A2M_EINVAL, C
    wcat = (((160 * 128 + 160) * 4 + 255) // 256) * 256
    assert f(*args) == N.A2M_EWS
    short = list(args)
    short[17], short[18] = h, wcat - 1
    assert f(*short) == N.A2M_EWS
    # the fused inference entries
    e = N.lib.a2m_self_attention_eval_f32
    ok = [h, 512, 2, 128, 4, h, h, h, None, h, 512, None]
    for i in (0, 5, 6, 7, 9):
        bad = list(ok)
        bad[i] = None
        assert e(*bad) == N.A2M_EINVAL, i
    for i, v in ((2, 0), (3, 64), (3, 512), (4, 6), (4, 68), (4, 0), (4, -4), (1, 514), (10, 516)):
        bad = list(ok)
        bad[i] = v
        assert e(*bad) == N.A2M_EINVAL, (i, v)
    assert N.lib.a2m_self_attention_eval_group_f32(h, 1024, 512, 0, 2, 128, 4, h, h, h, None, 0, h, 1024, None) == N.A2M_EINVAL
    assert N.lib.a2m_self_attention_eval_group_f32(h, 1026, 512, 2, 2, 128, 4, h, h, h, None, 0, h, 1024, None) == N.A2M_EINVAL
    assert N.lib.a2m_stack_qkv_f32(h, h, h, h, h, h, 12, h, h, None) == N.A2M_EINVAL
    assert N.lib.a2m_set_attn_eval_chunk(96) == N.A2M_EINVAL and '96' in N.last_error()
    assert N.lib.a2m_set_attn_eval_chunk(64) == 0


def test_channel_attention_argument_checks():
    from a2m import _native as N
    h = _host()
    f = N.lib.a2m_channel_attention_fwd_f32
    ok = [h, 2, 8, 4, h, h, 2, h, h, h, h, None]
    for i in (0, 4, 5, 7, 8, 9, 10):
        bad = list(ok)
        bad[i] = None
        assert f(*bad) == N.A2M_EINVAL, i
    for i in (1, 2, 3, 6):
        bad = list(ok)
        bad[i] = 0
        assert f(*bad) == N.A2M_EINVAL, i
    big = list(ok)
    big[2], big[6] = 8192, 1          # 4 (2 C + 2 Cr) bytes of LDS: 8 over the 64 KiB
    assert f(*big) == N.A2M_EINVAL and 'too large' in N.last_error()
    b = N.lib.a2m_channel_attention_bwd_f32
    okb = [h, h, 1, 2048, 4, h, h, 256, h, h, h, h, h, h, h, h, 1 << 40, None]
    # C = 2048 needs 4 (11 C + 8 Cr) = 98304 bytes of LDS in the backward; the forward's 18432 fit
    assert b(*okb) == N.A2M_EINVAL and 'too large' in N.last_error()
    assert 4 * (2 * 2048 + 2 * 256) <= 64 * 1024 < 4 * (11 * 2048 + 8 * 256)
    small = list(okb)
    small[3], small[7] = 8, 2
    for i in (0, 1, 5, 6, 8, 9, 10, 11, 12, 13, 14):
        bad = list(small)
        bad[i] = None
        assert b(*bad) == N.A2M_EINVAL, i
    need = 4 * 1 * (2 * 2 * 8 + 2 + 8)
    for ws, nbytes in ((None, need), (h, need - 1)):
        bad = list(small)
        bad[15], bad[16] = ws, nbytes
        assert b(*bad) == N.A2M_EWS, (ws, nbytes)
