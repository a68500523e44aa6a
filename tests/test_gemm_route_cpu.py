"""The GEMM engine's launch decision (gemm_route, csrc/gemm_route.cpp) through a2m_gemm_f32_route:
no GPU, the pointers are fake addresses that are only inspected for alignment.

The table check holds the route to the launches the parent commit of the route refactor issued:
tests/golden/gemm_route_parent_log.txt are that commit's A2M_GEMM_LOG=1 lines for the gemm_*,
gemm_kr_* and gemm_at_* cases of tests/test_gpu_pipe.py at fp32 / bf16, plan override (64, 0 | 3)
and pipe override 1 | 0, each run under a '# case=... prec=... split=... pipe=...' marker line.
The sweep checks structural properties of every route.
"""
import ctypes
import itertools
import os
import re

import pytest

from conftest import GOLDEN

KIND_TILE, KIND_TILE_KS2, KIND_PIPE, KIND_PIPE_PAIR = range(4)
VEC4, MCONTIG, HALO, REDUCE = 1, 2, 4, 8
BASE_A, BASE_B, BASE_C = 0x10000000, 0x20000000, 0x30000000   # 4096-aligned, never dereferenced


@pytest.fixture
def lib():
    from a2m import _native as N
    yield N.lib
    N.check(N.lib.a2m_gemm_pipe_override(-1))
    N.check(N.lib.a2m_gemm_plan_override(0, 0))
    N.check(N.lib.a2m_set_gemm_precision(0))


def route(lib, M, N, K, a_m, a_k, b_n, b_k, batch=1, pa=BASE_A, pb=BASE_B, pc=BASE_C):
    """The route of C[M][N] (row-major) = A . B^T with the given row / k strides."""
    out = (ctypes.c_int32 * 8)()
    bs = (lambda n: n) if batch > 1 else (lambda n: 0)   # batch strides as functional.gemm passes them
    rc = lib.a2m_gemm_f32_route(M, N, 1, K, 1, batch, pa, bs(M * max(K, 1)), a_m, a_k, 0, pb, bs(N * max(K, 1)),
                                b_n, 0, b_k, 0, pc, bs(M * N), N, 1, 0, None, 1.0, 0, out)
    assert rc == 0, lib.a2m_last_error()
    keys = ('kind', 'tile', 'bk', 'splits', 'kchunk', 'ma', 'mb', 'flags')
    return dict(zip(keys, out))


def case_strides(case):
    """(M, N, K, a_m, a_k, b_n, b_k) of a gemm_* case of tests/test_gpu_pipe.py."""
    m = re.fullmatch(r'gemm_(kr_|at_)?(\d+)x(\d+)x(\d+)(_rows|_kr)?', case)
    kind, (M, N, K), tail = m.group(1), map(int, m.group(2, 3, 4)), m.group(5)
    if kind is None:
        return M, N, K, K, 1, K, 1            # A [M][K], B [N][K]
    if kind == 'kr_':
        return M, N, K, K, 1, 1, N            # A [M][K], B [K][N]
    if tail == '_rows':
        return M, N, K, 1, M, K, 1            # A [K][M], B [N][K]
    return M, N, K, 1, M, 1, N                # A [K][M], B [K][N]


def parent_rows():
    rows, cfg = [], None
    with open(os.path.join(GOLDEN, 'gemm_route_parent_log.txt')) as f:
        for line in f:
            if line.startswith('# '):
                cfg = dict(kv.split('=') for kv in line[2:].split())
            elif line.startswith('a2m gemm '):
                rows.append((cfg, line.strip()))
    return rows


PARENT_ROWS = parent_rows()


def test_parent_log_covers_the_parametrisation():
    seen = {(c['case'], c['prec'], c['split'], c['pipe']) for c, _ in PARENT_ROWS}
    cases = {c['case'] for c, _ in PARENT_ROWS}
    assert len(cases) == 7 and all(c.startswith('gemm_') for c in cases)
    assert seen == set(itertools.product(cases, ('fp32', 'bf16'), ('0', '3'), ('1', '0')))
    assert len(PARENT_ROWS) == len(seen)   # one launch per run


@pytest.mark.parametrize('cfg,line', PARENT_ROWS,
                         ids=['{case}-{prec}-split{split}-pipe{pipe}'.format(**c) for c, _ in PARENT_ROWS])
def test_route_matches_parent_launch(lib, cfg, line):
    f = dict(re.findall(r'(\w+)=([\d,]+)', line))
    M, N, K, a_m, a_k, b_n, b_k = case_strides(cfg['case'])
    assert (int(f['M']), int(f['N']), int(f['K'])) == (M, N, K)
    assert lib.a2m_set_gemm_precision({'fp32': 0, 'bf16': 1}[cfg['prec']]) == 0
    assert lib.a2m_gemm_plan_override(64, int(cfg['split'])) == 0
    assert lib.a2m_gemm_pipe_override(int(cfg['pipe'])) == 0
    r = route(lib, M, N, K, a_m, a_k, b_n, b_k)
    assert (r['tile'], r['bk'], r['splits']) == (int(f['tile']), int(f['bk']), int(f['splits']))
    assert [r['ma'], r['mb']] == [int(v) for v in f['modes'].split(',')]
    assert (r['kind'] == KIND_PIPE) == ('(pipe)' in line)


SIZES_MN = (1, 63, 64, 65, 130, 1000)
SIZES_K = (0, 4, 31, 32, 33, 300, 20000)


def layouts(M, N, K):
    """(a_m, a_k, b_n, b_k): row-major and k-major operands."""
    return [(max(K, 1), 1, max(K, 1), 1), (max(K, 1), 1, 1, N), (1, M, max(K, 1), 1), (1, M, 1, N)]


@pytest.mark.parametrize('prec', [0, 1])
def test_route_properties(lib, prec):
    assert lib.a2m_set_gemm_precision(prec) == 0
    for pipe in (-1, 0):
        assert lib.a2m_gemm_pipe_override(pipe) == 0
        for M, N, K, batch in itertools.product(SIZES_MN, SIZES_MN, SIZES_K, (1, 3)):
            for lay in layouts(M, N, K):
                r = route(lib, M, N, K, *lay, batch=batch)
                where = (prec, pipe, M, N, K, batch, lay, r)
                assert r['splits'] >= 1 and r['splits'] * r['kchunk'] >= K, where
                assert r['bk'] == (64 if prec else 32) and r['kchunk'] % r['bk'] == 0 and r['kchunk'] > 0, where
                assert r['tile'] in (64, 128), where
                if K == 0:
                    assert r['splits'] == 1, where
                assert bool(r['flags'] & REDUCE) == (r['splits'] > 1), where
                if N % 4 != 0 and r['splits'] == 1:
                    assert not r['flags'] & VEC4, where
                assert not r['flags'] & HALO, where          # no tap conv among these operands
                assert r['kind'] in (KIND_TILE, KIND_TILE_KS2, KIND_PIPE), where
                if pipe == 0:
                    assert r['kind'] != KIND_PIPE, where
                if r['kind'] == KIND_PIPE:
                    assert r['tile'] == 64, where
                if r['kind'] == KIND_TILE_KS2:
                    assert prec == 0 and r['tile'] == 64 and (r['ma'], r['mb']) == (0, 0), where
                assert route(lib, M, N, K, *lay, batch=batch) == r, where   # deterministic


def test_misaligned_base_leaves_mode_0_and_vec4(lib):
    for M, N, K in ((64, 64, 64), (130, 1000, 300), (65, 64, 32)):
        lay = (K, 1, K, 1)
        r = route(lib, M, N, K, *lay)
        assert (r['ma'], r['mb']) == (0, 0)
        assert r['flags'] & VEC4
        ra = route(lib, M, N, K, *lay, pa=BASE_A + 4)
        assert ra['ma'] in (1, 4) and ra['mb'] == 0
        rb = route(lib, M, N, K, *lay, pb=BASE_B + 4)
        assert rb['ma'] == 0 and rb['mb'] in (1, 4)
        # one split, output base off the 16-byte grid: scalar stores
        assert lib.a2m_gemm_plan_override(0, 1) == 0
        assert route(lib, M, N, K, *lay)['flags'] & VEC4
        rc = route(lib, M, N, K, *lay, pc=BASE_C + 4)
        assert rc['splits'] == 1 and not rc['flags'] & VEC4
        assert lib.a2m_gemm_plan_override(0, 0) == 0


def test_kernel_counts_without_launches(lib):
    c = (ctypes.c_int64 * 4)()
    assert lib.a2m_gemm_kernel_counts(c, 1) == 0
    route(lib, 64, 64, 64, 64, 1, 64, 1)   # a route query is no launch
    assert lib.a2m_gemm_kernel_counts(c, 0) == 0
    assert list(c) == [0, 0, 0, 0]
