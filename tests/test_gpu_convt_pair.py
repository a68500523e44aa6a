"""The paired launch of a stride-2 ConvTranspose1d's two output phases (gemm_pipe_kernel_pair,
a2m_convt_pair_override) against the sequential path -- one gemm() per phase, held to one split --
and against torch.

Each phase runs the same tile body on the same operands in the same k order in both paths, so the
outputs are bitwise equal.  The shapes are the smallest at which the tail and bound handling can
go wrong: a partial n-tile (N = 32), M not a multiple of 64 with an odd number of channel chunks
(the chunk-parity tail), 2 + 2 and 3 + 2 taps, a strided output view, the fused BN + ReLU epilogue.
"""
import functools

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4   # tests/test_gpu_parity.py::test_convt1d_tap_path
DEV = 'cuda'


@pytest.fixture
def eng():
    import a2m
    from a2m import _native as N
    yield a2m, N
    N.check(N.lib.a2m_convt_pair_override(-1))
    N.check(N.lib.a2m_gemm_plan_override(0, 0))
    a2m.set_gemm_precision('fp32')


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


# name -> (B, Ci, Co, Tin), (ks, stride, pad, out_pad), out= view with a padded batch stride, BN + ReLU
CASES = {
    'n32_partial_tile': ((2, 64, 64, 16), (3, 2, 1, 1), False, False),
    'm40_three_chunks': ((3, 96, 40, 8), (3, 2, 1, 1), False, False),
    'm72_t32': ((2, 128, 72, 32), (3, 2, 1, 1), False, False),
    'b1_t64': ((1, 64, 64, 64), (3, 2, 1, 1), False, False),
    'k4_taps_2_2': ((2, 64, 48, 16), (4, 2, 1, 0), False, False),
    'k5_taps_3_2': ((2, 96, 40, 16), (5, 2, 2, 1), False, False),
    'strided_out': ((3, 64, 40, 16), (3, 2, 1, 1), True, False),
    'bn_relu': ((2, 64, 64, 16), (3, 2, 1, 1), False, True),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """CPU tensors of the case and its torch reference (computed once, shared, never modified)."""
    (B, Ci, Co, Tin), (ks, stride, pad, op), _, bn = CASES[name]
    x, w, b = _rand(B, Ci, Tin, seed=41), _rand(Ci, Co, ks, seed=42, scale=0.1), _rand(Co, seed=43)
    ref = torch.nn.functional.conv_transpose1d(x, w, b, stride=stride, padding=pad, output_padding=op)
    bnp = None
    if bn:
        bnp = (_rand(Co, seed=44).abs() + .5, _rand(Co, seed=45), _rand(Co, seed=46), _rand(Co, seed=47).abs() + .5)
        ref = torch.relu(torch.nn.functional.batch_norm(ref, bnp[2], bnp[3], bnp[0], bnp[1], False, 0.0, 1e-5))
    return x, w, b, bnp, ref


def _runner(name):
    """run() -> the case's output (a fresh tensor, or the view of a NaN-filled padded buffer)."""
    from a2m import functional as F
    (B, Ci, Co, Tin), (ks, stride, pad, op), strided, _ = CASES[name]
    x, w, b, bnp, ref = _case(name)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    bn = None if bnp is None else tuple(t.to(DEV) for t in bnp) + (1e-5,)
    cache = {}
    Tout = ref.shape[2]

    def run():
        out, big = None, None
        if strided:
            big = torch.full((B, Co + 3, Tout), float('nan'), device=DEV)
            out = big[:, :Co]
            assert out.stride(0) > Co * Tout
        y = F.convt1d(xd, wd, bd, stride, pad, op, bn=bn, act=F.ACT_RELU if bn else F.ACT_NONE, out=out,
                      cache=cache)
        if strided:
            assert torch.isnan(big[:, Co:]).all()   # nothing written outside the view
        return y
    return run, ref


def _both(N, run, off_split=1):
    """The same call with the pair forced on, then forced off (held to one split)."""
    N.check(N.lib.a2m_convt_pair_override(1))
    pair = run().clone()
    N.check(N.lib.a2m_convt_pair_override(0))
    N.check(N.lib.a2m_gemm_plan_override(64 if off_split else 0, off_split))
    try:
        seq = run().clone()
    finally:
        N.check(N.lib.a2m_gemm_plan_override(0, 0))
        N.check(N.lib.a2m_convt_pair_override(-1))
    torch.cuda.synchronize()
    return pair, seq


@pytest.mark.parametrize('name', sorted(CASES))
def test_pair_bitwise_equals_sequential_and_matches_torch(eng, name):
    from a2m import functional as F
    _, N = eng
    run, ref = _runner(name)
    N.check(N.lib.a2m_convt_pair_override(1))
    F.gemm_kernel_counts(reset=True)
    with F.gemm_timing() as t:
        run()
    assert t.launches == 1, f'{name}: the pair was not taken ({t.launches} launches)'
    assert F.gemm_kernel_counts() == [0, 0, 0, 1]   # one GEMM_KIND_PIPE_PAIR launch, nothing else
    pair, seq = _both(N, run)
    assert pair.shape == ref.shape
    e_pair, e_seq = rel_err(pair.cpu(), ref), rel_err(seq.cpu(), ref)
    print(f'{name}: rel err vs torch pair {e_pair:.2e} sequential {e_seq:.2e}')
    assert torch.equal(pair, seq), f'{name}: max diff {(pair - seq).abs().max().item()}'
    assert e_pair < TOL and e_seq < TOL


def test_stride4_keeps_sequential_path(eng):
    """k6 s4 p1: four phases, never paired -- the override changes nothing."""
    from a2m import functional as F
    _, N = eng
    B, Ci, Co, T = 3, 96, 40, 4
    x, w, b = _rand(B, Ci, T, seed=51), _rand(Ci, Co, 6, seed=52, scale=0.1), _rand(Co, seed=53)
    ref = torch.nn.functional.conv_transpose1d(x, w, b, stride=4, padding=1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    cache = {}
    N.check(N.lib.a2m_convt_pair_override(1))
    F.gemm_kernel_counts(reset=True)
    with F.gemm_timing() as t:
        F.convt1d(xd, wd, bd, 4, 1, 0, cache=cache)
    assert t.launches == 4
    counts = F.gemm_kernel_counts()
    assert counts[F.GEMM_KIND_PIPE_PAIR] == 0 and sum(counts) == 4
    on, off = _both(N, lambda: F.convt1d(xd, wd, bd, 4, 1, 0, cache=cache), off_split=0)
    assert torch.equal(on, off) and rel_err(on.cpu(), ref) < TOL


def test_bf16_keeps_sequential_path(eng):
    from a2m import functional as F
    a2m, N = eng
    B, Ci, Co, T = 2, 128, 64, 16
    x, w, b = _rand(B, Ci, T, seed=54), _rand(Ci, Co, 3, seed=55, scale=0.1), _rand(Co, seed=56)
    ref = torch.nn.functional.conv_transpose1d(x, w, b, stride=2, padding=1, output_padding=1)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    a2m.set_gemm_precision('bf16')
    cache = {}
    N.check(N.lib.a2m_convt_pair_override(1))
    F.gemm_kernel_counts(reset=True)
    with F.gemm_timing() as t:
        F.convt1d(xd, wd, bd, cache=cache)
    assert t.launches == 2
    counts = F.gemm_kernel_counts()
    assert counts[F.GEMM_KIND_PIPE_PAIR] == 0 and sum(counts) == 2
    on, off = _both(N, lambda: F.convt1d(xd, wd, bd, cache=cache), off_split=0)
    assert torch.equal(on, off) and rel_err(on.cpu(), ref) < 2e-2   # bf16 operands (tests/test_gpu_pipe.py)


def test_default_rule_pairs_only_launches_that_fill_the_chip(eng):
    """Override -1: paired from one 64x64 tile per CU (2 tiles(M, N) >= 256), sequential below."""
    from a2m import functional as F
    _, N = eng
    N.check(N.lib.a2m_convt_pair_override(-1))
    for (B, Ci, Co, T), paired in (((64, 64, 512, 16), True), ((64, 64, 448, 16), False)):   # 2 x 128 / 2 x 112 tiles
        xd, wd = _rand(B, Ci, T, seed=57).to(DEV), _rand(Ci, Co, 3, seed=58, scale=0.1).to(DEV)
        cache = {}
        F.gemm_kernel_counts(reset=True)
        with F.gemm_timing() as t:
            y = F.convt1d(xd, wd, None, cache=cache)
        assert (t.launches == 1) == paired, (Co, t.launches)
        assert F.gemm_kernel_counts()[F.GEMM_KIND_PIPE_PAIR] == (1 if paired else 0)
        N.check(N.lib.a2m_convt_pair_override(0))
        N.check(N.lib.a2m_gemm_plan_override(64, 1))
        try:
            seq = F.convt1d(xd, wd, None, cache=cache)
        finally:
            N.check(N.lib.a2m_gemm_plan_override(0, 0))
            N.check(N.lib.a2m_convt_pair_override(-1))
        if paired:
            assert torch.equal(y, seq)


def test_pair_deterministic_and_graph_capturable(eng):
    from a2m import functional as F
    _, N = eng
    (B, Ci, Co, Tin), (ks, stride, pad, op), _, _ = CASES['m72_t32']
    x, w, b, _, ref = _case('m72_t32')
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    cache = {}
    N.check(N.lib.a2m_convt_pair_override(1))
    eager = F.convt1d(xd, wd, bd, stride, pad, op, cache=cache)
    again = F.convt1d(xd, wd, bd, stride, pad, op, cache=cache)
    assert torch.equal(eager, again)
    out = torch.zeros_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.convt1d(xd, wd, bd, stride, pad, op, out=out, cache=cache)
    for _ in range(2):
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_pair_timing_is_one_record_with_both_phases_flops(eng):
    from a2m import functional as F
    _, N = eng
    for name in ('m72_t32', 'k5_taps_3_2'):
        (B, Ci, Co, Tin), (ks, stride, pad, op), _, _ = CASES[name]
        run, _ = _runner(name)
        N.check(N.lib.a2m_convt_pair_override(1))
        run()   # packs the weights outside the window
        F.gemm_kernel_counts(reset=True)
        with F.gemm_timing() as t:
            run()
        assert t.launches == 1 and t.reduces == 0 and t.ms_reduce == 0
        assert F.gemm_kernel_counts() == [0, 0, 0, 1]
        assert t.flops == 2.0 * Co * B * Tin * ks * Ci
        assert t.ms_tile > 0
