"""Float64 numpy restatements of the losses, small adjoints and the optimiser step of
csrc/losses.hip, csrc/train_loss.hip and csrc/evaluation.hip, by the formulas of include/a2m.h:

  bone    mean over (clip, bone) of (mean_t |gen[c] - gen[p]| - mean_t |real[c] - real[p]|)^2, 51 bones
  hand    mean over (clip, frame, 30 hand triples) of relu(-a) + relu(a - pi)
  body    mean over (clip, frame, 5 body triples) of relu(-pi/2 - a) + relu(a - pi)
          a = atan2(cross(u, v), dot(u, v)), u = p[j] - p[a], v = p[c] - p[j]
  motion  m = diff_t(pose): mean |m_fake - m_real|, mean_t ||diff m_fake||, mean_t ||diff diff m_fake||
          (a term over no frames is 0; the gradient through a zero norm or a zero difference is 0)
  mse     mean (pred - target)^2
  adam    torch.optim.Adam's update, weight decay added to the gradient
  interp  bilinear (T, 1) resize of [H, W], align_corners = False, and its adjoint
  moments per feature: mean and mean of squares over the frames, the neck subtracted in float32

No autograd and nothing from the package: the gradients are written out.  Every summing function
takes `omit`, the index of one term -- (clip, frame, bone), (clip, frame, triple), (clip, t,
feature), one flat element or one t -- that is left out of the sums with the divisor unchanged:
what a kernel computes that loses an element at an edge.  Negative indices count from the end.

Shared by the CPU and GPU tests; the tests treat its outputs as read-only.
"""
import numpy as np

PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 7, 6,
           10, 11, 12, 13, 10, 15, 16, 17, 10, 19, 20, 21, 10, 23, 24, 25, 10, 27, 28, 29,
           3, 31, 32, 33, 34, 31, 36, 37, 38, 31, 40, 41, 42, 31, 44, 45, 46, 31, 48, 49, 50]
# (parent, joint, first child) along every chain; the hand triples index joints from 10
HAND_TRIPLES = [(0, 1, 2), (1, 2, 3), (2, 3, 4), (0, 5, 6), (5, 6, 7), (6, 7, 8), (0, 9, 10),
                (9, 10, 11), (10, 11, 12), (0, 13, 14), (13, 14, 15), (14, 15, 16), (0, 17, 18),
                (17, 18, 19), (18, 19, 20), (21, 22, 23), (22, 23, 24), (23, 24, 25), (21, 26, 27),
                (26, 27, 28), (27, 28, 29), (21, 30, 31), (30, 31, 32), (31, 32, 33), (21, 34, 35),
                (34, 35, 36), (35, 36, 37), (21, 38, 39), (38, 39, 40), (39, 40, 41)]
BODY_TRIPLES = [(0, 1, 2), (1, 2, 3), (0, 4, 5), (4, 5, 6), (0, 7, 8)]
N_BONES = 51
CHILD = np.arange(1, 52)
PAR = np.array(PARENTS[1:])
PART = {'hand': (10, HAND_TRIPLES, 0.0), 'body': (0, BODY_TRIPLES, -np.pi / 2)}   # offset, triples, lower kink


def chain_pose(B, T, seed):
    """A pose built along the skeleton: joint 0 ~ N(0, 1), every other joint its parent plus
    len (cos th, sin th), len ~ U[0.5, 1.5), th ~ U(-pi, pi); float64, rounded to float32,
    interleaved [B][T][104].  Every bone is at least 0.5 long and the angles are well spread."""
    rng = np.random.default_rng(seed)
    p = np.zeros((B, T, 52, 2))
    p[:, :, 0] = rng.standard_normal((B, T, 2))
    ln = rng.uniform(0.5, 1.5, (B, T, 52))
    th = rng.uniform(-np.pi, np.pi, (B, T, 52))
    for j in range(1, 52):
        p[:, :, j, 0] = p[:, :, PARENTS[j], 0] + ln[:, :, j] * np.cos(th[:, :, j])
        p[:, :, j, 1] = p[:, :, PARENTS[j], 1] + ln[:, :, j] * np.sin(th[:, :, j])
    return p.reshape(B, T, 104).astype(np.float32)


def _joints(pose):
    p = np.asarray(pose, dtype=np.float64)
    return p.reshape(p.shape[0], p.shape[1], 52, 2)


def _weights(shape, omit):
    w = np.ones(shape)
    if omit is not None:
        w[tuple(omit)] = 0.0
    return w


# ------------------------------------------------------------------------------ bone
def bone_lengths(pose):
    """[B][T][51]: the length of bone k, joint k + 1 from its parent."""
    p = _joints(pose)
    d = p[:, :, CHILD] - p[:, :, PAR]
    return np.sqrt((d * d).sum(-1))


def bone_loss(gen, real, omit=None):
    """omit: one (clip, frame, bone) of the generated pose's lengths."""
    lg, lr = bone_lengths(gen), bone_lengths(real)
    T = lg.shape[1]
    d = (lg * _weights(lg.shape, omit)).sum(1) / T - lr.sum(1) / T
    return float((d * d).sum() / d.size)


def bone_grad(gen, real, omit=None):
    """d bone_loss / d gen, [B][T][104]."""
    p = _joints(gen)
    B, T = p.shape[:2]
    d = p[:, :, CHILD] - p[:, :, PAR]
    n = np.sqrt((d * d).sum(-1))
    w = _weights(n.shape, omit)
    coef = 2.0 * ((n * w).sum(1) / T - bone_lengths(real).sum(1) / T) / (B * N_BONES) / T      # [B][51]
    unit = np.where(n[..., None] > 0, d / np.where(n > 0, n, 1.0)[..., None], 0.0)
    g = (coef[:, None, :] * w)[..., None] * unit
    out = np.zeros_like(p)
    np.add.at(out, (slice(None), slice(None), CHILD), g)
    np.add.at(out, (slice(None), slice(None), PAR), -g)
    return out.reshape(B, T, 104)


# ------------------------------------------------------------------------------ angles
def _uv(pose, part):
    off, triples, _ = PART[part]
    t = np.array(triples) + off
    p = _joints(pose)
    return p[:, :, t[:, 1]] - p[:, :, t[:, 0]], p[:, :, t[:, 2]] - p[:, :, t[:, 1]], t


def angles(pose, part):
    """[B][T][30 or 5]: the signed angle of every triple."""
    u, v, _ = _uv(pose, part)
    return np.arctan2(u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0], (u * v).sum(-1))


def angle_terms(pose, part):
    a = angles(pose, part)
    return np.maximum(PART[part][2] - a, 0.0) + np.maximum(a - np.pi, 0.0)


def angle_loss(pose, part, omit=None):
    """omit: one (clip, frame, triple)."""
    t = angle_terms(pose, part)
    return float((t * _weights(t.shape, omit)).sum() / t.size)


def kink_distance(pose, part):
    """The smallest distance of an angle from a kink of the loss or from the wrap of atan2."""
    a = angles(pose, part)
    return float(np.minimum(np.abs(a - PART[part][2]), np.pi - np.abs(a)).min())


def angle_grad(pose, part, omit=None):
    """d angle_loss / d pose, [B][T][104]; 0 where u or v vanishes (atan2(0, 0))."""
    u, v, t = _uv(pose, part)
    B, T = u.shape[:2]
    cr = u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]
    dt = (u * v).sum(-1)
    a = np.arctan2(cr, dt)
    g = (np.where(a > np.pi, 1.0, 0.0) - np.where(a < PART[part][2], 1.0, 0.0)) * _weights(a.shape, omit) / a.size
    den = cr * cr + dt * dt
    ok = den > 0
    gcr = np.where(ok, g * dt / np.where(ok, den, 1.0), 0.0)
    gdt = np.where(ok, -g * cr / np.where(ok, den, 1.0), 0.0)
    gu = np.stack([gcr * v[..., 1] + gdt * v[..., 0], -gcr * v[..., 0] + gdt * v[..., 1]], -1)
    gv = np.stack([-gcr * u[..., 1] + gdt * u[..., 0], gcr * u[..., 0] + gdt * u[..., 1]], -1)
    out = np.zeros((B, T, 52, 2))
    np.add.at(out, (slice(None), slice(None), t[:, 1]), gu - gv)
    np.add.at(out, (slice(None), slice(None), t[:, 0]), -gu)
    np.add.at(out, (slice(None), slice(None), t[:, 2]), gv)
    return out.reshape(B, T, 104)


# ------------------------------------------------------------------------------ motion terms
def _motion_parts(fake, real, omit):
    f = np.asarray(fake, dtype=np.float64)
    fm = np.diff(f, axis=1)
    acc = fm[:, 1:] - fm[:, :-1]
    jerk = acc[:, 1:] - acc[:, :-1]
    d = fm - np.diff(np.asarray(real, dtype=np.float64), axis=1) if real is not None else None

    def w(a, key):
        o = omit.get(key) if isinstance(omit, dict) else omit
        return _weights(a.shape, o if a.shape[1] > 0 else None)
    return f, d, acc, jerk, (w(fm, 'l1'), w(acc, 'smooth'), w(jerk, 'jerk'))


def motion_terms(fake, real, omit=None):
    """(L1 on motion, smoothness, jerk).  omit (clip, t, feature): that element of the L1 sum and
    that feature's square in the norm at (clip, t) of each of the other two; or a dict with one
    such index for each of 'l1', 'smooth' and 'jerk' (a missing key omits nothing)."""
    f, d, acc, jerk, (w1, wa, wj) = _motion_parts(fake, real, omit)
    l1 = float((np.abs(d) * w1).sum() / d.size) if d is not None else 0.0
    sm = float(np.sqrt((acc * acc * wa).sum(-1)).sum() / (acc.shape[0] * acc.shape[1])) if acc.shape[1] else 0.0
    jk = float(np.sqrt((jerk * jerk * wj).sum(-1)).sum() / (jerk.shape[0] * jerk.shape[1])) if jerk.shape[1] else 0.0
    return l1, sm, jk


def _diff_adjoint(g):
    """The adjoint of diff along axis 1: out[t] = g[t - 1] - g[t] with zero edges."""
    out = np.zeros((g.shape[0], g.shape[1] + 1, g.shape[2]))
    out[:, 1:] += g
    out[:, :-1] -= g
    return out


def motion_grad(fake, real, gterms, omit=None):
    """d (sum_i gterms[i] terms[i]) / d fake, [B][T][Fd]."""
    f, d, acc, jerk, (w1, wa, wj) = _motion_parts(fake, real, omit)
    gm = np.zeros((f.shape[0], f.shape[1] - 1, f.shape[2]))
    if d is not None:
        gm += gterms[0] * np.sign(d) * w1 / d.size

    def unit(x, w):
        n = np.sqrt((x * x * w).sum(-1, keepdims=True))
        return np.where(n > 0, x * w / np.where(n > 0, n, 1.0), 0.0)
    if acc.shape[1]:
        gm += _diff_adjoint(gterms[1] * unit(acc, wa) / (acc.shape[0] * acc.shape[1]))
    if jerk.shape[1]:
        gm += _diff_adjoint(_diff_adjoint(gterms[2] * unit(jerk, wj) / (jerk.shape[0] * jerk.shape[1])))
    return _diff_adjoint(gm)


# ------------------------------------------------------------------------------ mse, adam
def mse_loss(pred, target, omit=None):
    """omit: one flat element."""
    d = (np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)).reshape(-1)
    return float((d * d * _weights(d.shape, None if omit is None else (omit,))).sum() / d.size)


def mse_grad(pred, target, grad_loss=1.0):
    d = np.asarray(pred, dtype=np.float64) - np.asarray(target, dtype=np.float64)
    return grad_loss * 2.0 * d / d.size


def adam(p, grads, m, v, lr, b1, b2, eps, wd, first_step=1, lrs=None):
    """len(grads) steps of torch.optim.Adam from step `first_step`; returns the (p, m, v) after every
    step.  lrs: a learning rate per step (default lr for all)."""
    p, m, v = (np.array(t, dtype=np.float64) for t in (p, m, v))
    out = []
    for k, g in enumerate(grads):
        step = first_step + k
        g = np.asarray(g, dtype=np.float64) + wd * p
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        denom = np.sqrt(v) / np.sqrt(1.0 - b2 ** step) + eps
        p = p - (lr if lrs is None else lrs[k]) / (1.0 - b1 ** step) * (m / denom)
        out.append((p, m, v))
    return out


# ------------------------------------------------------------------------------ interp, moments
def interp_weights(n_in, n_out):
    """[n_out][n_in]: the linear resize weights of one axis, align_corners = False."""
    A = np.zeros((n_out, n_in))
    for o in range(n_out):
        src = max(n_in / n_out * (o + 0.5) - 0.5, 0.0)
        i0 = min(int(src), n_in - 1)
        i1 = min(i0 + 1, n_in - 1)
        l1 = src - i0
        A[o, i0] += 1.0 - l1
        A[o, i1] += l1
    return A


def interp_time(x, T):
    """[B][C][H][W] -> [B][C][T]: the (T, 1) bilinear resize."""
    x = np.asarray(x, dtype=np.float64)
    return np.einsum('th,w,bchw->bct', interp_weights(x.shape[2], T), interp_weights(x.shape[3], 1)[0], x)


def interp_time_bwd(dy, H, W, omit=None):
    """The adjoint, [B][C][T] -> [B][C][H][W].  omit: one t left out of every sum over time."""
    dy = np.asarray(dy, dtype=np.float64)
    wt = _weights((dy.shape[2],), None if omit is None else (omit,))
    return np.einsum('th,w,bct->bchw', interp_weights(H, dy.shape[2]) * wt[:, None], interp_weights(W, 1)[0], dy)


def pose_moments(pose, necksub, omit=None):
    """pose float32 [n][104] planar (x of 52 joints, then y) -> (mean [104], mean of squares [104],
    mean of |terms| of each): the neck is subtracted in float32, the sums run in float64.
    omit: one frame."""
    x = np.asarray(pose, dtype=np.float32).reshape(-1, 104)
    if necksub:
        x = x - np.repeat(x[:, [0, 52]], 52, axis=1)          # a float32 subtraction
    x = x.astype(np.float64) * _weights((x.shape[0], 1), None if omit is None else (omit, 0))
    n = x.shape[0]
    return x.sum(0) / n, (x * x).sum(0) / n, np.abs(x).sum(0) / n, (x * x).sum(0) / n
