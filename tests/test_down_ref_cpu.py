"""Toom-Cook F(2,2) down-sampling conv1d, the parts that need no GPU: the packed weight layout of
a2m_conv1d_down_pack_f32 (restated in tests/down_ref.py) on a literal case, the F(2,2) identity
with per-clip zero padding in fp64, and the float32 emulation (transforms, wave and phase
accumulation order) against an fp64 conv1d(stride=2, padding=1) on the GPU test's shapes."""
import numpy as np
import pytest

import down_ref as DR

SHAPES = [(1, 32, 64, 16), (5, 64, 20, 16), (3, 96, 96, 32), (2, 128, 64, 64), (2, 64, 64, 128), (4, 512, 512, 64)]


def test_f22_identity_on_basis_vectors():
    """(M0 + M1, M1 + M2) of U = (g0, g0 + g1, g1), V = (d0 - d1, d1, d2 - d1) is the 2-tap
    correlation's two outputs, for every basis g, d."""
    for a in range(2):
        for b in range(3):
            g, d = np.eye(2)[a], np.eye(3)[b]
            M = np.array([g[0], g[0] + g[1], g[1]]) * np.array([d[0] - d[1], d[1], d[2] - d[1]])
            assert np.array_equal([M[0] + M[1], M[1] + M[2]], [g @ d[0:2], g @ d[1:3]]), (a, b)


def test_pack_u_literal_layout():
    """Co = 2, Ci = 64: w[co][ci][j] = 1000 co + 10 ci + j, so every packed float names its source."""
    Co, Ci = 2, 64
    co, ci, j = np.meshgrid(np.arange(Co), np.arange(Ci), np.arange(4), indexing='ij')
    w = (1000.0 * co + 10.0 * ci + j).astype(np.float32)
    p = DR.pack_u(w)
    assert p.shape == (Co * Ci * 6,) and p.dtype == np.float32
    row = p.reshape(Co, Ci // 32, 6, 32)
    # row 0, chunk 0: w0, w2, w1, w3, w0 + w2, w1 + w3 of channels 0..31
    c = 10.0 * np.arange(32)
    assert np.array_equal(row[0, 0], [c, c + 2, c + 1, c + 3, 2 * c + 2, 2 * c + 4])
    # row 1, chunk 1: channels 32..63
    c = 1000.0 + 10.0 * np.arange(32, 64)
    assert np.array_equal(row[1, 1], [c, c + 2, c + 1, c + 3, 2 * c + 2, 2 * c + 4])
    # flat offsets: row stride 6 Ci, chunk stride 192, unit stride 32
    assert p[6 * Ci + 192 + 4 * 32 + 5] == 2 * (1000.0 + 10.0 * 37) + 2


def test_f22_identity_fp64_clip_padding_and_edges():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((3, 32, 16))
    w = rng.standard_normal((7, 32, 4))
    y, ref = DR.down_conv(x, w), DR.conv_ref64(x, w)
    assert np.abs(y - ref).max() <= 1e-13 * np.abs(ref).max()
    # the edge probe of the GPU test: x only at t = 0 and T - 1, one tap -> y[t] = x[2t - 1 + tap], exactly
    xe = np.zeros((2, 32, 16))
    xe[:, :, 0] = 1.0
    xe[:, :, 15] = 1.0
    for tap in range(4):
        we = np.zeros((32, 32, 4))
        we[np.arange(32), np.arange(32), tap] = 1.0
        ye = DR.down_conv(xe, we)
        shifted = np.zeros((2, 32, 8))
        for t in range(8):
            if 0 <= 2 * t - 1 + tap < 16:
                shifted[:, :, t] = xe[:, :, 2 * t - 1 + tap]
        assert np.array_equal(ye, shifted), tap


@pytest.mark.parametrize('B,Ci,Co,Tin', SHAPES)
def test_f22_fp32_emulation_against_fp64(B, Ci, Co, Tin):
    rng = np.random.default_rng(B + Ci + Tin)
    x = rng.standard_normal((B, Ci, Tin)).astype(np.float32)
    w = (rng.standard_normal((Co, Ci, 4)) / np.sqrt(4 * Ci)).astype(np.float32)
    y = DR.down_conv(x, w)
    assert y.dtype == np.float32
    ref = DR.conv_ref64(x, w)
    e = np.abs(y.astype(np.float64) - ref).max() / np.abs(ref).max()
    print(f'B={B} Ci={Ci} Co={Co} Tin={Tin}: emulation {e:.2e}')
    assert e < 1e-5, e
