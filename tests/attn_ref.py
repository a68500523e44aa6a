"""Float64 numpy restatements of SelfAttention and ChannelAttention (csrc/attn_core.hip,
csrc/train_attn.hip and the attention entries of csrc/ops.hip), by the formulas of include/a2m.h:

  SelfAttention     q, k = 1x1 conv C -> C/8, v = 1x1 conv C -> C (qkv stacked [B][C/4 + C][T])
                    S[b][i][j] = sum_c q[b][c][i] k[b][c][j], A = softmax_j S (no 1/sqrt(d))
                    y = gamma * O + x (+ res), O[b][c][i] = sum_j v[b][c][j] A[b][i][j]
    backward        G = dy^T v, rowdot = sum_j A G, dgamma = sum rowdot, dS = gamma A (G - rowdot)
                    dV = gamma dy A, dQ = k dS^T, dK = q dS, dx = dy + Wcat^T dqkv, dres = dy
                    dWcat = sum_{b,t} dqkv x^T, dbcat = sum_{b,t} dqkv
  ChannelAttention  att = sigmoid(mlp(mean_t x)) + sigmoid(mlp(max_t x)), y = x att
                    mlp = Linear(C, Cr) -> ReLU -> Linear(Cr, C); the max pool's gradient goes to the
                    first maximum (nn.AdaptiveMaxPool1d); relu' at 0 is 0

No autograd, no torch and nothing from the package: the gradients are written out.  Every summing
function takes `omit`, the name of one term that is left out of its sum -- what a kernel computes
that loses an element at an edge:

  'key'      the last key of the last query row of the last clip, in the softmax and in PV
  'channel'  the last input channel of the q/k/v projection
  'outer'    the last (b, t) outer product of the weight gradients (and term of the bias gradients)
  'wrow'     the last row of Wcat^T dqkv in dx
  'rowdot'   the last row's rowdot in dgamma
  'clip'     the last clip's contribution to the ChannelAttention weight gradients
  'time'     the last time step of the average pool (and of sum_t dy x in the backward)

A function ignores the names that belong to other sums.  `omit_at` moves a term elsewhere: an index
(b, i, j) for 'key', (b, t) for 'outer', (b, c) for 'time' (that channel's last time step).

Shared by the CPU and GPU tests; the tests treat its outputs as read-only.
"""
import numpy as np


def _f64(a):
    return None if a is None else np.asarray(a, dtype=np.float64)


def stack_qkv(wq, bq, wk, bk, wv, bv):
    """Wcat [C/4 + C][C], bcat [C/4 + C]; a missing bias is zero."""
    ws = [_f64(w).reshape(w.shape[0], -1) for w in (wq, wk, wv)]
    bs = [np.zeros(w.shape[0]) if b is None else _f64(b) for w, b in zip(ws, (bq, bk, bv))]
    return np.concatenate(ws, 0), np.concatenate(bs, 0)


def project(x, wcat, bcat, omit=None):
    """qkv [B][C/4 + C][T].  omit 'channel': the last input channel left out."""
    x = _f64(x)
    if omit == 'channel':
        x, wcat = x[:, :-1], wcat[:, :-1]
    return np.matmul(wcat[None], x) + bcat[None, :, None]


def softmax_scores(q, k, omit=None, omit_at=None):
    """A [B][T][T] of q, k [B][Cq][T].  omit 'key': one (b, i, j), by default the last of each, has
    no part in row (b, i): neither in the denominator nor as a weight."""
    s = np.matmul(q.transpose(0, 2, 1), k)
    e = np.exp(s - s.max(-1, keepdims=True))
    if omit == 'key':
        e[tuple(omit_at) if omit_at is not None else (-1, -1, -1)] = 0.0
    return e / e.sum(-1, keepdims=True)


def self_attention(x, wq, bq, wk, bk, wv, bv, gamma, res=None, omit=None, omit_at=None):
    """(qkv, attn, y).  omit: 'key' or 'channel' (others ignored)."""
    x = _f64(x)
    wcat, bcat = stack_qkv(wq, bq, wk, bk, wv, bv)
    Cq = wcat.shape[1] // 8
    qkv = project(x, wcat, bcat, omit)
    q, k, v = qkv[:, :Cq], qkv[:, Cq:2 * Cq], qkv[:, 2 * Cq:]
    attn = softmax_scores(q, k, omit, omit_at)
    y = float(np.asarray(gamma).reshape(-1)[0]) * np.matmul(v, attn.transpose(0, 2, 1)) + x
    if res is not None:
        y = y + _f64(res)
    return qkv, attn, y


def self_attention_bwd(dy, x, wq, bq, wk, bk, wv, bv, gamma, qkv=None, attn=None, omit=None, omit_at=None):
    """dict(dx, dres, dwq, dbq, dwk, dbk, dwv, dbv, dgamma, dqkv, rowdot) from dy.  qkv and attn default to the
    forward's (with the same omit); omit: any of the SelfAttention names."""
    dy, x = _f64(dy), _f64(x)
    g = float(np.asarray(gamma).reshape(-1)[0])
    wcat, _ = stack_qkv(wq, bq, wk, bk, wv, bv)
    C = x.shape[1]
    Cq = C // 8
    if qkv is None or attn is None:
        qkv, attn, _ = self_attention(x, wq, bq, wk, bk, wv, bv, gamma, None, omit, omit_at)
    qkv, attn = _f64(qkv), _f64(attn)
    q, k, v = qkv[:, :Cq], qkv[:, Cq:2 * Cq], qkv[:, 2 * Cq:]
    G = np.matmul(dy.transpose(0, 2, 1), v)                  # [B][i][j]
    rowdot = (attn * G).sum(-1)                               # [B][i]
    dS = g * attn * (G - rowdot[..., None])
    rd = rowdot.copy()
    if omit == 'rowdot':
        rd[-1, -1] = 0.0
    dgamma = rd.sum()
    dV = g * np.matmul(dy, attn)                              # [B][C][j]
    dQ = np.matmul(k, dS.transpose(0, 2, 1))                  # [B][Cq][i]
    dK = np.matmul(q, dS)                                     # [B][Cq][j]
    dqkv = np.concatenate([dQ, dK, dV], 1)
    if omit == 'wrow':
        dx = dy + np.matmul(wcat[:-1].T[None], dqkv[:, :-1])
    else:
        dx = dy + np.matmul(wcat.T[None], dqkv)
    dq = dqkv
    if omit == 'outer':
        dq = dqkv.copy()
        dq[(omit_at[0], slice(None), omit_at[1]) if omit_at is not None else (-1, slice(None), -1)] = 0.0
    dw = np.matmul(dq.transpose(1, 0, 2).reshape(dq.shape[1], -1), x.transpose(1, 0, 2).reshape(C, -1).T)
    db = dq.sum((0, 2))
    return dict(dx=dx, dres=dy, dgamma=float(dgamma), dqkv=dqkv, rowdot=rowdot,
                dwq=dw[:Cq], dwk=dw[Cq:2 * Cq], dwv=dw[2 * Cq:],
                dbq=db[:Cq], dbk=db[Cq:2 * Cq], dbv=db[2 * Cq:])


# ------------------------------------------------------------------------------ ChannelAttention
def _sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def _pools(x, omit, omit_at):
    T = x.shape[2]
    w = np.ones(x.shape)
    if omit == 'time':
        if omit_at is None:
            w[:, :, -1] = 0.0
        else:
            w[omit_at[0], omit_at[1], -1] = 0.0
    return (x * w).sum(-1) / T, x.max(-1), x.argmax(-1), w      # argmax: the first occurrence


def channel_attention_parts(x, w1, b1, w2, b2, omit=None, omit_at=None):
    """Everything the backward needs: avg, mx, argmax, the hidden pre-activations pre [2][B][Cr] (avg
    pool, max pool), the sigmoids s [2][B][C], att and y."""
    x, w1, b1, w2, b2 = (_f64(a) for a in (x, w1, b1, w2, b2))
    avg, mx, am, wt = _pools(x, omit, omit_at)
    pre = np.stack([p @ w1.T + b1 for p in (avg, mx)])
    h = np.maximum(pre, 0.0)
    s = _sigmoid(h @ w2.T + b2)
    att = s[0] + s[1]
    return dict(avg=avg, mx=mx, argmax=am, pre=pre, h=h, s=s, att=att, y=x * att[..., None], wt=wt)


def channel_attention(x, w1, b1, w2, b2, omit=None, omit_at=None):
    """(att [B][C], y [B][C][T]).  omit: 'time'."""
    p = channel_attention_parts(x, w1, b1, w2, b2, omit, omit_at)
    return p['att'], p['y']


def channel_attention_bwd(dy, x, w1, b1, w2, b2, omit=None, omit_at=None):
    """dict(dx, dw1, db1, dw2, db2).  omit: 'time' or 'clip'."""
    dy, x, w1, w2 = _f64(dy), _f64(x), _f64(w1), _f64(w2)
    p = channel_attention_parts(x, w1, b1, w2, b2, omit, omit_at)
    B, C, T = x.shape
    da = (dy * x * p['wt']).sum(-1)                                   # [B][C]
    dz = da[None] * p['s'] * (1.0 - p['s'])                           # [2][B][C]
    dh = (dz @ w2) * (p['h'] > 0)                                     # [2][B][Cr]
    pooled = np.stack([p['avg'], p['mx']])
    nb = B - 1 if omit == 'clip' else B
    dw2 = np.einsum('pbc,pbr->cr', dz[:, :nb], p['h'][:, :nb])
    db2 = dz[:, :nb].sum((0, 1))
    dw1 = np.einsum('pbr,pbc->rc', dh[:, :nb], pooled[:, :nb])
    db1 = dh[:, :nb].sum((0, 1))
    dpool = dh @ w1                                                   # [2][B][C]
    dx = dy * p['att'][..., None] + (dpool[0] / T)[..., None]
    bi, ci = np.meshgrid(np.arange(B), np.arange(C), indexing='ij')
    dx[bi, ci, p['argmax']] += dpool[1]
    return dict(dx=dx, dw1=dw1, db1=db1, dw2=dw2, db2=db2)
