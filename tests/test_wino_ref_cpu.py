"""Winograd F(2,3) conv1d, the parts that need no GPU: the packed weight layout of
a2m_conv1d_wino_pack_f32 (restated in tests/wino_ref.py) against G.g in fp64, and the F(2,3)
identity with per-clip zero padding in fp64."""
import numpy as np

import wino_ref as WR


def test_transform_matrices_are_f23():
    """A^T [(G g) * (B^T d)] is the two outputs of the 3-tap correlation, for every basis g, d."""
    for a in range(3):
        for b in range(4):
            g, d = np.eye(3)[a], np.eye(4)[b]
            y = WR.AT_MAT @ ((WR.G_MAT @ g) * (WR.BT_MAT @ d))
            ref = np.array([g @ d[0:3], g @ d[1:4]])
            assert np.array_equal(y, ref), (a, b, y, ref)


def test_packed_u_layout_matches_g_matrix():
    rng = np.random.default_rng(0)
    Co, Ci = 5, 96
    w = rng.standard_normal((Co, Ci, 3))
    packed = WR.pack_u(w)
    assert packed.shape == (Co * Ci * 4,)
    u = np.einsum('pk,ock->poc', WR.G_MAT, w)          # [4][Co][Ci] in fp64
    for co in (0, 3, 4):
        for ci in (0, 31, 32, 70, 95):
            for p in range(4):
                got = packed[((co * (Ci // 32) + ci // 32) * 4 + p) * 32 + ci % 32]
                assert abs(got - u[p, co, ci]) <= 1e-15 * max(1.0, abs(u[p, co, ci])), (co, ci, p)
    assert np.allclose(WR.unpack_u(packed, Co, Ci), u, rtol=0, atol=1e-15)
    # fp32: points 0 and 3 are the taps themselves, 1 and 2 within two roundings of G.g
    w32 = w.astype(np.float32)
    u32 = WR.unpack_u(WR.pack_u(w32), Co, Ci)
    assert u32.dtype == np.float32
    assert np.array_equal(u32[0], w32[..., 0]) and np.array_equal(u32[3], w32[..., 2])
    u64 = np.einsum('pk,ock->poc', WR.G_MAT, w32.astype(np.float64))
    assert np.abs(u32 - u64).max() <= 2 * 2.0 ** -24 * np.abs(w32).sum(-1).max()


def test_f23_identity_fp64_clip_padding():
    """T = 16 clips: every clip is padded on its own (no pair reads across a clip edge)."""
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 32, 16))
    w = rng.standard_normal((7, 32, 3))
    y, ref = WR.wino_conv(x, w), WR.conv_ref64(x, w)
    assert np.abs(y - ref).max() <= 1e-13 * np.abs(ref).max()
    # the edge probe of the GPU test: x only at t = 0 and T - 1, one tap -> the shifted input, exactly
    xe = np.zeros((2, 32, 16))
    xe[:, :, 0] = 1.0
    xe[:, :, 15] = 1.0
    for tap in range(3):
        we = np.zeros((32, 32, 3))
        we[np.arange(32), np.arange(32), tap] = 1.0
        ye = WR.wino_conv(xe, we)
        shifted = np.zeros_like(xe)
        s = tap - 1                                      # y[t] = x[t + s]
        for t in range(16):
            if 0 <= t + s < 16:
                shifted[:, :, t] = xe[:, :, t + s]
        assert np.array_equal(ye, shifted), tap


def test_f23_fp32_error_class():
    """fp32 transforms and sums stay in the direct conv's error class against fp64 (the bound the
    GPU test holds the kernel to is 1e-5 of max |ref|)."""
    rng = np.random.default_rng(2)
    x = rng.standard_normal((2, 256, 64)).astype(np.float32)
    w = (rng.standard_normal((64, 256, 3)) / np.sqrt(768)).astype(np.float32)
    ref = WR.conv_ref64(x, w)
    e = np.abs(WR.wino_conv(x, w).astype(np.float64) - ref).max() / np.abs(ref).max()
    assert e < 1e-5, e
