"""Float64 numpy restatement of the skeleton-graph layer (csrc/graph.hip, csrc/train_graph.hip),
by the formulas of their header comments, with every gradient written out:

  GAT (4 heads, mean)  x'[n,h] = x_n W_h^T, a_src[n,h] = x'[n,h] . att_src[h], a_dst likewise
                       edges: the given ones plus one self loop per node
                       s[j->i,h] = a_src[j,h] + a_dst[i,h], e = LeakyReLU(s, 0.2)
                       alpha = exp(e - max_i) / (sum_i exp(e - max_i) + 1e-16) over the edges into i
                       o_i = 1/4 sum_h sum_{j->i} alpha[j->i,h] x'[j,h] + bias
  GraphConv            o_i = (sum_{j->i} x_j) W_rel^T + x_i W_root^T + bias
  tail (norm_res)      ohat = (o - mean o) rstd, rstd = 1/sqrt(var o + 1e-5), u = ohat ln_w + ln_b,
                       y = LeakyReLU(u, slope) + x;   without it y = o
    backward           du = dy leaky'(u), dln_w = sum_n du ohat, dln_b = sum_n du, g = du ln_w,
                       do = rstd (g - mean g - ohat mean(g ohat)), dx = dy;  without the tail do = dy, dx = 0
                       dbias = sum_n do
      GraphConv        dW_rel = sum_n do_n (x) agg_n, dW_root = sum_n do_n (x) x_n,
                       dx_i += do_i W_root, dx_j += (do_i W_rel) for every edge j->i
      GAT              dout = do / 4 (every head); per edge j->i: dx'[j,h] += alpha dout_i,
                       dalpha = dout_i . x'[j,h]; de = alpha (dalpha - sum_{edges into i} alpha dalpha),
                       ds = de leaky'(s); da_src[j,h] += ds, da_dst[i,h] += ds;
                       dx'[n,h] += da_src[n,h] att_src[h] + da_dst[n,h] att_dst[h],
                       datt_src[h] = sum_n da_src[n,h] x'[n,h], datt_dst likewise,
                       dW_h = sum_n dx'[n,h] (x) x_n, dx_n += sum_h dx'[n,h] W_h

Every sum over edges is a scatter over the edge list in its own order (np.add.at), so directed
graphs, repeated edges and any edge order are handled as a scatter handles them.  No autograd, no
torch and nothing from the package.

`omit` names one term that is left out, what a kernel computes that loses it.  The terms hang on
one node, the `target`: of the last frame, the node of the largest in-degree (the lowest such), and
on its last in-edge in edge order:

  'slot'     that edge's message in the aggregation (forward) and its adjoint (backward: what it
             sends to its source's dx' / dx)
  'self'     the target's GAT self loop, in the same two places
  'reverse'  that edge's ds in its source's da_src
  'frame'    the last frame's rows in dw0, dw1, dbias, dln_w, dln_b
  'head'     the last head's datt_src, datt_dst and block of dw0

A function ignores the names that belong elsewhere, and a topology without an edge ignores the
three edge names.  The backward leaves a term out of its own sums only: it takes the full forward.

Shared by the CPU and GPU tests; the tests treat its outputs as read-only.
"""
import numpy as np

HEADS, FEAT = 4, 64
ATT_SLOPE = 0.2
LN_EPS = 1e-5
OMITS = ('slot', 'self', 'reverse', 'frame', 'head')


# ----------------------------------------------------------------------------- topologies
def symmetric(und):
    """(src, dst) of an undirected edge list: both directions of every pair, pair by pair."""
    src, dst = [], []
    for a, b in und:
        src += [a, b]
        dst += [b, a]
    return src, dst


def random_tree(n, max_deg, seed):
    """Undirected edges of a seeded random tree over n nodes, every degree <= max_deg.  A node
    draws its parent among the earlier nodes below the limit with weight 1 + degree, so that some
    nodes reach the limit."""
    rs = np.random.RandomState(seed)
    deg = [0] * n
    und = []
    for i in range(1, n):
        open_ = [p for p in range(i) if deg[p] < max_deg]
        w = np.array([1.0 + deg[p] for p in open_])
        p = open_[rs.choice(len(open_), p=w / w.sum())]
        und.append((p, i))
        deg[p] += 1
        deg[i] += 1
    return und


def shuffled(src, dst, seed):
    perm = np.random.RandomState(seed).permutation(len(src))
    return [src[i] for i in perm], [dst[i] for i in perm]


def topologies():
    """name -> (J, src, dst) of the topologies that need no skeleton: see test_gpu_graph_fp64.py."""
    t = {}
    t['star7'] = (9,) + symmetric([(0, i) for i in range(1, 8)])
    t['single'] = (1, [], [])
    t['path128'] = (128,) + symmetric([(i, i + 1) for i in range(63)])
    t['tree85'] = (85,) + symmetric(random_tree(85, 7, seed=85))
    t['tree43'] = (43,) + symmetric(random_tree(43, 7, seed=43))
    t['multi'] = (4,) + symmetric([(0, 1), (0, 1), (1, 2), (2, 3)])
    t['directed'] = (9, list(range(1, 8)), [0] * 7)
    return t


def expand(J, src, dst, F):
    """The frame-by-frame edge arrays over F*J nodes."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    off = (np.arange(F, dtype=np.int64) * J)[:, None]
    return (src[None] + off).reshape(-1), (dst[None] + off).reshape(-1)


def target(J, src, dst, F):
    """(node, edge): the omit target node (global index) and its last in-edge (index into the
    expanded edge arrays; None without an edge)."""
    deg = np.bincount(np.asarray(dst, dtype=np.int64), minlength=J) if len(dst) else np.zeros(J, int)
    node = int(np.argmax(deg))
    if deg[node] == 0:
        return (F - 1) * J + node, None
    last = max(e for e in range(len(dst)) if dst[e] == node)
    return (F - 1) * J + node, (F - 1) * len(dst) + last


def in_degree_stats(J, src, dst):
    deg = np.bincount(np.asarray(dst, dtype=np.int64), minlength=J) if len(dst) else np.zeros(J, int)
    return int(deg.max()), int(deg.min())


# ----------------------------------------------------------------------------- forward
def _leaky(v, slope):
    return np.where(v > 0, v, v * slope)


def forward(x, J, src, dst, kind, w0, w1, att_src, att_dst, bias, ln_w=None, ln_b=None, slope=0.2,
            omit=None, dtype=np.float64):
    """dict: y, pre_ln (o, bias included), the intermediates the backward reads, and the margins
    min_u / min_s (None where there is no such kink).  norm_res = ln_w is not None.  dtype float32
    evaluates the same formulas in float32 (for the margins' evaluation error)."""
    c = lambda a: None if a is None else np.asarray(a, dtype=dtype)
    x, w0, w1, bias, ln_w, ln_b = c(x), c(w0), c(w1), c(bias), c(ln_w), c(ln_b)
    N = x.shape[0]
    F = N // J
    es, ed = expand(J, src, dst, F)
    tnode, tedge = target(J, src, dst, F)
    r = dict(kind=kind, J=J, F=F, n_edges=len(es), tnode=tnode, tedge=tedge)
    if kind == 0:
        a_s_p, a_d_p = c(att_src).reshape(HEADS, FEAT), c(att_dst).reshape(HEADS, FEAT)
        xp = (x @ w0.T).reshape(N, HEADS, FEAT)
        a_s, a_d = (xp * a_s_p).sum(-1), (xp * a_d_p).sum(-1)
        loop = np.arange(N, dtype=np.int64)
        es, ed = np.concatenate([es, loop]), np.concatenate([ed, loop])
        s = a_s[es] + a_d[ed]
        e = _leaky(s, dtype(ATT_SLOPE))
        mx = np.full((N, HEADS), -np.inf, dtype=dtype)
        np.maximum.at(mx, ed, e)
        ex = np.exp(e - mx[ed])
        den = np.zeros((N, HEADS), dtype=dtype)
        np.add.at(den, ed, ex)
        alpha = ex / (den[ed] + dtype(1e-16))
        keep = np.ones(len(es), dtype=dtype)
        if omit == 'slot' and tedge is not None:
            keep[tedge] = 0
        if omit == 'self':
            keep[r['n_edges'] + tnode] = 0
        msg = (alpha * keep[:, None])[:, :, None] * xp[es]
        out = np.zeros((N, HEADS, FEAT), dtype=dtype)
        np.add.at(out, ed, msg)
        o = out.mean(1) + bias
        r.update(xp=xp, s=s, alpha=alpha, es=es, ed=ed, min_s=float(np.abs(s).min()))
    else:
        keep = np.ones(len(es), dtype=dtype)
        if omit == 'slot' and tedge is not None:
            keep[tedge] = 0
        agg = np.zeros_like(x)
        np.add.at(agg, ed, x[es] * keep[:, None])
        o = agg @ w0.T + bias + x @ w1.T
        r.update(agg=agg, es=es, ed=ed, s=None, min_s=None)
    r['pre_ln'] = o
    if ln_w is not None:
        mean = o.mean(-1, keepdims=True)
        var = ((o - mean) ** 2).mean(-1, keepdims=True)
        rstd = 1 / np.sqrt(var + dtype(LN_EPS))
        ohat = (o - mean) * rstd
        u = ohat * ln_w + ln_b
        r.update(ohat=ohat, rstd=rstd, u=u, y=_leaky(u, dtype(slope)) + x, min_u=float(np.abs(u).min()))
    else:
        r.update(u=None, y=o, min_u=None)
    return r


# ----------------------------------------------------------------------------- backward
def backward(dy, fwd, x, w0, w1, att_src, att_dst, ln_w=None, slope=0.2, omit=None):
    """dict(dx, dw0, dw1, datt_src, datt_dst, dbias, dln_w, dln_b) from dy and the (full) float64
    forward `fwd`; entries a layer does not have are None."""
    f64 = lambda a: None if a is None else np.asarray(a, dtype=np.float64)
    dy, x, w0, w1, ln_w = f64(dy), f64(x), f64(w0), f64(w1), f64(ln_w)
    N, J, F = x.shape[0], fwd['J'], fwd['F']
    es, ed, tnode, tedge, kind = fwd['es'], fwd['ed'], fwd['tnode'], fwd['tedge'], fwd['kind']
    rows = np.ones((N, 1))          # the rows that reach the weight / bias / LayerNorm sums
    if omit == 'frame':
        rows[(F - 1) * J:] = 0
    g = dict.fromkeys(('dx', 'dw0', 'dw1', 'datt_src', 'datt_dst', 'dbias', 'dln_w', 'dln_b'))
    if ln_w is not None:
        ohat, rstd, u = fwd['ohat'], fwd['rstd'], fwd['u']
        du = dy * np.where(u > 0, 1.0, slope)
        g['dln_w'] = (du * ohat * rows).sum(0)
        g['dln_b'] = (du * rows).sum(0)
        gg = du * ln_w
        do = rstd * (gg - gg.mean(-1, keepdims=True) - ohat * (gg * ohat).mean(-1, keepdims=True))
        dx = dy.copy()
    else:
        do = dy
        dx = np.zeros_like(x)
    g['dbias'] = (do * rows).sum(0)
    if kind == 1:
        g['dw0'] = (do * rows).T @ fwd['agg']
        g['dw1'] = (do * rows).T @ x
        dagg = do @ w0
        dx += do @ w1
        keep = np.ones(len(es))
        if omit == 'slot' and tedge is not None:
            keep[tedge] = 0
        np.add.at(dx, es, dagg[ed] * keep[:, None])
    else:
        a_s_p, a_d_p = f64(att_src).reshape(HEADS, FEAT), f64(att_dst).reshape(HEADS, FEAT)
        xp, alpha, s = fwd['xp'], fwd['alpha'], fwd['s']
        dout = np.repeat((do / HEADS)[:, None, :], HEADS, axis=1)        # [N][4][64]
        keep = np.ones(len(es))
        if omit == 'slot' and tedge is not None:
            keep[tedge] = 0
        if omit == 'self':
            keep[fwd['n_edges'] + tnode] = 0
        dxp = np.zeros_like(xp)
        np.add.at(dxp, es, (alpha * keep[:, None])[:, :, None] * dout[ed])
        dalpha = (dout[ed] * xp[es]).sum(-1)                              # [E][4]
        sdot = np.zeros((N, HEADS))
        np.add.at(sdot, ed, alpha * dalpha)
        ds = alpha * (dalpha - sdot[ed]) * np.where(s > 0, 1.0, ATT_SLOPE)
        da_dst = np.zeros((N, HEADS))
        np.add.at(da_dst, ed, ds)
        keep_r = np.ones(len(es))
        if omit == 'reverse' and tedge is not None:
            keep_r[tedge] = 0
        da_src = np.zeros((N, HEADS))
        np.add.at(da_src, es, ds * keep_r[:, None])
        dxp += da_src[:, :, None] * a_s_p[None] + da_dst[:, :, None] * a_d_p[None]
        datt_src = (da_src[:, :, None] * xp).sum(0)
        datt_dst = (da_dst[:, :, None] * xp).sum(0)
        dw0 = np.einsum('nhc,nk->hck', dxp * rows[:, :, None], x)
        if omit == 'head':
            datt_src[-1] = 0
            datt_dst[-1] = 0
            dw0[-1] = 0
        g['datt_src'], g['datt_dst'] = datt_src.reshape(np.shape(att_src)), datt_dst.reshape(np.shape(att_dst))
        g['dw0'] = dw0.reshape(HEADS * FEAT, FEAT)
        dx += dxp.reshape(N, HEADS * FEAT) @ w0
    g['dx'] = dx
    return g
