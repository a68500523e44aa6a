"""numpy restatement of the Toom-Cook F(2,2) down-sampling conv1d pieces of csrc
(conv1d_down_pack_kernel in ops.hip; the transforms and the wave / phase accumulation order of
gemm_f32_pipe_down.hip), in any float dtype.  Shared by the CPU and GPU tests.

The 4-tap stride-2 pad-1 conv is two 2-tap convs, over the odd input samples (taps w0, w2) and the
even ones (taps w1, w3); per phase d = three samples two apart, V = (d0 - d1, d1, d2 - d1),
U = (g0, g0 + g1, g1), and y[2i] = M0 + M1, y[2i + 1] = M1 + M2 with M_p summed over both phases."""
import numpy as np

# the six units of a 32-channel chunk in the packed row, as (plane, phase): the order in which the
# kernel's three k-steps read them (wn = 0 unit, then wn = 1 unit)
UNITS = [(0, 0), (2, 0), (0, 1), (2, 1), (1, 0), (1, 1)]


def u_planes(w):
    """[Co][Ci][4] -> U[plane][phase] ([Co][Ci] each; phase 0 = odd samples, taps (w0, w2))."""
    g = [(w[..., 0], w[..., 2]), (w[..., 1], w[..., 3])]
    return [[g[f][0] for f in range(2)], [g[f][0] + g[f][1] for f in range(2)], [g[f][1] for f in range(2)]]


def pack_u(w):
    """[Co][Ci][4] -> the packed layout [Co][Ci/32][6][32], flat: w0, w2, w1, w3, w0 + w2, w1 + w3."""
    Co, Ci, ks = w.shape
    assert ks == 4 and Ci % 32 == 0
    U = u_planes(w)
    u = np.stack([U[p][f] for p, f in UNITS], axis=1)   # [Co][6][Ci]
    return u.reshape(Co, 6, Ci // 32, 32).transpose(0, 2, 1, 3).reshape(-1)


def v_planes(x):
    """x [B][Ci][Tin] (Tin % 4 == 0; every clip padded with zeros on its own) -> V[plane][phase],
    [B][Ci][Tin / 4] each: pair i reads x[4i - 1 .. 4i + 4]."""
    B, Ci, T = x.shape
    xp = np.zeros((B, Ci, T + 2), x.dtype)
    xp[:, :, 1:T + 1] = x
    V = [[None, None] for _ in range(3)]
    for f in range(2):
        d = [xp[:, :, f + 2 * j:f + 2 * j + T:4] for j in range(3)]   # d_j[i] = x[4i - 1 + f + 2j]
        V[0][f], V[1][f], V[2][f] = d[0] - d[1], d[1], d[2] - d[1]
    return V


def down_conv(x, w):
    """y [B][Co][Tin / 2] through F(2,2) in x's dtype, accumulated as the kernel's waves do: per
    32-channel chunk M0 += odd then even, M2 likewise, M1 as two sums (one per phase), and
    y[2i] = M0 + (M1 odd + M1 even), y[2i + 1] = M2 + (M1 odd + M1 even)."""
    B, Ci, T = x.shape
    Co = w.shape[0]
    assert Ci % 32 == 0 and T % 4 == 0
    U, V = u_planes(w), v_planes(x)
    z = lambda: np.zeros((B, Co, T // 4), x.dtype)
    M0, M2, M1 = z(), z(), [z(), z()]
    mm = lambda u, v, c: np.einsum('oc,bci->boi', u[:, c:c + 32], v[:, c:c + 32])
    for c in range(0, Ci, 32):
        for f in range(2):
            M0 = M0 + mm(U[0][f], V[0][f], c)
            M2 = M2 + mm(U[2][f], V[2][f], c)
        for f in range(2):
            M1[f] = M1[f] + mm(U[1][f], V[1][f], c)
    y = np.empty((B, Co, T // 2), x.dtype)
    y[:, :, 0::2] = M0 + (M1[0] + M1[1])
    y[:, :, 1::2] = M2 + (M1[0] + M1[1])
    return y


def conv_ref64(x, w):
    """fp64 direct conv (cross-correlation, 4 taps, stride 2, pad 1)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, Ci, T = x.shape
    xp = np.zeros((B, Ci, T + 2))
    xp[:, :, 1:T + 1] = x
    return sum(np.einsum('oc,bct->bot', w[:, :, j], xp[:, :, j:j + T:2]) for j in range(4))
