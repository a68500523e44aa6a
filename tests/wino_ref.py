"""numpy restatement of the Winograd F(2,3) conv1d pieces of csrc (conv1d_wino_pack_kernel in
ops.hip, the transforms of gemm_f32_pipe_wino.hip), in any float dtype.  Shared by the CPU and
GPU tests."""
import numpy as np

G_MAT = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])   # U = G g
BT_MAT = np.array([[1.0, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]])          # V = B^T d
AT_MAT = np.array([[1.0, 1, 1, 0], [0, 1, -1, -1]])                                       # y = A^T M


def pack_u(w):
    """[Co][Ci][3] -> the packed layout [Co][Ci/32][4][32], flat, with the kernel's operations in
    w's dtype: U0 = g0, U1 = ((g0 + g2) + g1) / 2, U2 = ((g0 + g2) - g1) / 2, U3 = g2."""
    Co, Ci, ks = w.shape
    assert ks == 3 and Ci % 32 == 0
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]
    half = w.dtype.type(0.5)
    u = np.stack([g0, ((g0 + g2) + g1) * half, ((g0 + g2) - g1) * half, g2], axis=1)   # [Co][4][Ci]
    return u.reshape(Co, 4, Ci // 32, 32).transpose(0, 2, 1, 3).reshape(-1)


def unpack_u(packed, Co, Ci):
    """The packed layout back to [4][Co][Ci]."""
    return packed.reshape(Co, Ci // 32, 4, 32).transpose(2, 0, 1, 3).reshape(4, Co, Ci)


def wino_conv(x, w):
    """y[b][co][t] of the 3-tap pad-1 stride-1 conv of x [B][Ci][T] (T even; every clip padded with
    zeros on its own) through F(2,3): V from x, U from w, M_p = U_p V_p, y[2i] = M0 + M1 + M2,
    y[2i + 1] = M1 - M2 - M3, all in x's dtype."""
    B, Ci, T = x.shape
    Co = w.shape[0]
    xp = np.zeros((B, Ci, T + 2), x.dtype)
    xp[:, :, 1:T + 1] = x
    d = [xp[:, :, j:j + T:2] for j in range(4)]        # d_j[b][c][i] = x[2i - 1 + j]
    V = [d[0] - d[2], d[1] + d[2], d[2] - d[1], d[1] - d[3]]
    U = unpack_u(pack_u(w), Co, Ci)
    M = [np.einsum('oc,bci->boi', U[p], V[p]) for p in range(4)]
    y = np.empty((B, Co, T), x.dtype)
    y[:, :, 0::2] = (M[0] + M[1]) + M[2]
    y[:, :, 1::2] = (M[1] - M[2]) - M[3]
    return y


def conv_ref64(x, w):
    """fp64 direct conv (cross-correlation, pad 1)."""
    x, w = np.asarray(x, np.float64), np.asarray(w, np.float64)
    B, Ci, T = x.shape
    xp = np.zeros((B, Ci, T + 2))
    xp[:, :, 1:T + 1] = x
    return sum(np.einsum('oc,bct->bot', w[:, :, j], xp[:, :, j:j + T]) for j in range(3))
