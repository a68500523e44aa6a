"""Checks of tests/graph_ref.py, the float64 restatement the GPU comparison of the skeleton-graph
layer kernels (tests/test_gpu_graph_fp64.py) rests on; no GPU needed.

  * it agrees with oracle.model (_gat_fn / graph_conv + layer_norm + leaky_relu) in float64 under torch
    autograd, forward and every gradient, on every case of the GPU file, to 1e-12 of the maximum -- the
    only use of the oracle: the GPU tests do not depend on it
  * every omission of graph_ref.OMITS moves the outputs it belongs to by more than the bound the GPU
    test applies to them, on every case that has the term
  * every LayerNorm output u and attention logit s lies at least 10 x the case's float32 evaluation
    error (float32 run of the restatement against the float64 run) from its LeakyReLU kink
  * the E32 table of the GPU file is reproduced (python tests/test_graph_ref_cpu.py --write-table
    rewrites it, choosing each case's draw k as the first that meets the two conditions above)
  * skeleton.in_neighbour_csr(symmetric=True) refuses a topology the layer backward is wrong on
"""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import graph_ref as GR
import test_gpu_graph_fp64 as G
from conftest import rel_err

ALL_CASES = G.CASES + G.FWD_CASES
GRADS = ('dx', 'dw0', 'dw1', 'datt_src', 'datt_dst', 'dbias', 'dln_w', 'dln_b')
# omission -> the outputs it must show in (where the case has them and they are not identically zero)
SHOWS_IN = {'slot': ('y', 'pre_ln', 'dx'), 'self': ('y', 'pre_ln', 'dx'), 'reverse': ('datt_src', 'dx'),
            'frame': ('dw0', 'dw1', 'dbias', 'dln_w', 'dln_b'), 'head': ('dw0', 'datt_src', 'datt_dst')}
MARGIN = 10.0


def oracle_outputs(c, p, dtype):
    """name -> numpy array: the oracle's forward and autograd gradients in `dtype`."""
    from oracle import model as OM
    topo, F, kind, norm_res, slope = c
    J, src, dst = G.topology(topo)
    ei = torch.tensor([list(src), list(dst)], dtype=torch.long).reshape(2, -1)
    edges = OM.expand_edges(ei, J, F)
    t = {k: None if v is None else v.detach().clone().to(dtype).requires_grad_(k != 'dy') for k, v in p.items()}
    if kind == 0:
        o = OM._gat_fn(t['x'], edges, t['w0'], t['att_src'], t['att_dst'], t['bias'], 4)
    else:
        o = OM.graph_conv(OM.Ctx({'g.lin_rel.weight': t['w0'], 'g.lin_rel.bias': t['bias'],
                                  'g.lin_root.weight': t['w1']}), 'g', t['x'], edges)
    y = TF.leaky_relu(TF.layer_norm(o, (64,), t['ln_w'], t['ln_b']), slope) + t['x'] if norm_res else o
    out = {'y': y.detach().numpy()}
    if norm_res:
        out['pre_ln'] = o.detach().numpy()
    if topo != 'directed':
        y.backward(t['dy'])
        for name in GRADS:
            leaf = t['x' if name == 'dx' else name[1:]]
            if leaf is not None:
                out[name] = leaf.grad.numpy()
    return out


def _shows(c, omit, fwd):
    """The outputs an omission must show in on this case ((): the case does not have the term)."""
    kind = c[2]
    if omit in ('slot', 'reverse') and fwd['tedge'] is None:
        return ()
    if omit in ('self', 'reverse', 'head') and kind != 0:
        return ()
    if c[0] == 'directed':   # forward only
        return tuple(n for n in SHOWS_IN[omit] if n in ('y', 'pre_ln'))
    return SHOWS_IN[omit]


@functools.lru_cache(maxsize=None)
def analyse(c, k):
    """Everything the checks need of draw k of a case: reference outputs, E32 per output, the kink
    margins with their float32 evaluation errors, and per omission the shift of each output."""
    back = c[0] != 'directed'
    p, fwd, g = G.reference_for(c, k, backward=back)
    ref = G.outputs(c, fwd, g)
    n_threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        o32 = oracle_outputs(c, p, torch.float32)
    finally:
        torch.set_num_threads(n_threads)
    e32 = {name: (rel_err(o32[name].reshape(r.shape), r) if r.any() else 0.0) for name, r in ref.items()}
    _, f32, _ = G.reference_for(c, k, dtype=np.float32, backward=False)
    margins = {}
    for key in ('u', 's'):
        if fwd[key] is not None:
            margins[key] = (float(np.abs(fwd[key]).min()), float(np.abs(f32[key].astype(np.float64) - fwd[key]).max()))
    shifts = {}
    for omit in GR.OMITS:
        names = _shows(c, omit, fwd)
        if not names:
            continue
        _, fo, go = G.reference_for(c, k, omit=omit, backward=back)
        om = G.outputs(c, fo, go)
        shifts[omit] = {n: rel_err(om[n], ref[n]) for n in names if n in ref and ref[n].any()}
    return dict(p=p, ref=ref, e32=e32, margins=margins, shifts=shifts)


def _bound(name, e32):
    return min(G.FACTOR * e32, G.TOL if name in ('y', 'pre_ln') else G.GTOL)


def _problems(a):
    """What keeps a draw from serving as a test case (empty: nothing)."""
    bad = []
    for key, (mn, ev) in a['margins'].items():
        if not mn >= MARGIN * ev:
            bad.append(f'min |{key}| {mn:.3e} < {MARGIN:g} x fp32 error {ev:.3e}')
    for omit, sh in a['shifts'].items():
        for name, d in sh.items():
            if not d > _bound(name, a['e32'][name]):
                bad.append(f"omit '{omit}' moves {name} by {d:.3e} <= bound {_bound(name, a['e32'][name]):.3e}")
    return bad


def _k(c):
    return G.E32[G.case_id(c)][0]


@pytest.mark.parametrize('c', ALL_CASES, ids=G.case_id)
def test_reference_matches_float64_oracle(c):
    a = analyse(c, _k(c))
    o64 = oracle_outputs(c, a['p'], torch.float64)
    assert set(o64) == set(a['ref'])
    for name, r in a['ref'].items():
        if not r.any():
            assert np.abs(o64[name]).max() < 1e-14, name
            continue
        err = rel_err(r, o64[name].reshape(r.shape))
        assert err < 1e-12, (name, err)


@pytest.mark.parametrize('c', ALL_CASES, ids=G.case_id)
def test_omissions_show_above_the_gpu_bounds(c):
    a = analyse(c, _k(c))
    cid = G.case_id(c)
    for omit, sh in a['shifts'].items():
        assert sh, (cid, omit)
        for name, d in sh.items():
            b = min(G.bound(cid, name))
            print(f"{cid} omit '{omit}' {name}: shift {d:.3e} bound {b:.3e}")
            assert d > b, (omit, name, d, b)


def test_every_omission_is_exercised():
    """Each name has cases that exercise it; the edge names on every topology with an edge."""
    for omit in GR.OMITS:
        n = sum(1 for c in ALL_CASES if analyse(c, _k(c))['shifts'].get(omit))
        assert n >= 4, (omit, n)
    for c in G.CASES:
        if c[0] != 'single':
            assert 'slot' in analyse(c, _k(c))['shifts']
    single = [c for c in G.CASES if c[0] == 'single' and c[2] == 0]
    assert single and all('self' in analyse(c, _k(c))['shifts'] for c in single)


@pytest.mark.parametrize('c', ALL_CASES, ids=G.case_id)
def test_inputs_stay_clear_of_the_kinks(c):
    a = analyse(c, _k(c))
    assert ('u' in a['margins']) == c[3] and ('s' in a['margins']) == (c[2] == 0)
    for key, (mn, ev) in a['margins'].items():
        print(f'{G.case_id(c)} min |{key}| {mn:.3e} fp32 error {ev:.3e} ratio {mn / ev:.1f}')
        assert mn >= MARGIN * ev, (key, mn, ev)


@pytest.mark.parametrize('c', ALL_CASES, ids=G.case_id)
def test_e32_table_is_reproduced(c):
    """The table's entries against a fresh float32 run of the oracle.  On the CPU the table was
    written on the run is the same; another CPU's float32 BLAS blocks its sums differently, that is
    another summation order of the same formulas, for which the GPU bound allows FACTOR: the same
    allowance holds here, both ways."""
    row = G.E32[G.case_id(c)]
    a = analyse(c, row[0])
    for name, val in zip(G.OUTS, row[1:]):
        assert (val is None) == (name not in a['ref']), name
        if val is None:
            continue
        e = a['e32'][name]
        print(f'{G.case_id(c)} {name}: table {val:.3e} now {e:.3e}')
        assert (e == 0.0 and val == 0.0) or e / G.FACTOR <= val <= G.FACTOR * e, (name, val, e)


def test_topologies_are_what_the_gpu_file_says():
    S = _skeleton()
    t = {name: G.topology(name) for name in list(G.FRAMES) + ['directed']}
    deg = {name: GR.in_degree_stats(*v) for name, v in t.items()}
    assert deg['star7'] == (7, 0) and deg['single'] == (0, 0) and deg['directed'] == (7, 0)
    J, src, dst = t['path128']
    assert J == 128 and len(src) == 126 and J + 1 + len(src) == 255 and max(src) == 63
    J, src, dst = t['tree85']
    assert J == 85 and len(src) == 168 and J + 1 + len(src) == 254 and deg['tree85'][0] == 7
    full = [n for n in range(J) if dst.count(n) == 7]   # all 8 GAT slots on nodes other than node 0
    assert len(full) >= 2 and 0 not in full
    assert t['tree43'][0] == 43 and len(t['tree43'][1]) == 84 and deg['tree43'][0] == 7
    assert sorted(zip(*t['hand'][1:])) == sorted(zip(*t['hand-shuffled'][1:])) and t['hand'] != t['hand-shuffled']
    assert list(zip(*t['multi'][1:])).count((0, 1)) == 2
    for name, (J, src, dst) in t.items():   # every one within the kernels' limits
        S.in_neighbour_csr(torch.tensor([list(src), list(dst)], dtype=torch.long).reshape(2, -1), J)
    assert sorted({F * G.topology(n)[0] for n, fs in G.FRAMES.items() for F in fs} & {129, 170}) == [129, 170]


# ----------------------------------------------------------------------------- symmetric check
def _skeleton():
    from a2m import skeleton as S
    return S


def _ei(name):
    J, src, dst = G.topology(name)
    return torch.tensor([list(src), list(dst)], dtype=torch.long).reshape(2, -1), J


def test_symmetric_check_accepts_the_skeletons_and_a_repeated_edge():
    S = _skeleton()
    for lo, J in ((0, S.NUM_BODY), (10, S.NUM_HAND)):
        ei = S.edge_index(lo, J)
        a, b = S.in_neighbour_csr(ei, J, symmetric=True), S.in_neighbour_csr(ei, J)
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    for name in G.FRAMES:
        S.in_neighbour_csr(*_ei(name), symmetric=True)
    ptr, idx = S.in_neighbour_csr(*_ei('multi'), symmetric=True)
    assert idx[ptr[1]:ptr[2]].tolist() == [0, 0, 2]


def test_symmetric_check_refuses_a_directed_topology_and_names_the_edge():
    S = _skeleton()
    ei, J = _ei('directed')
    with pytest.raises(ValueError, match=r'edge 1->0 .* reverse 0->1'):
        S.in_neighbour_csr(ei, J, symmetric=True)
    ptr, idx = S.in_neighbour_csr(ei, J)          # still builds: the forward takes it
    assert ptr.tolist() == [0] + [7] * 9 and idx.tolist() == list(range(1, 8))
    # multiplicity counts: 0->1 twice, 1->0 once
    with pytest.raises(ValueError, match=r'edge 0->1 occurs 2 time\(s\) but its reverse 1->0 1'):
        S.in_neighbour_csr(torch.tensor([[0, 0, 1], [1, 1, 0]]), 2, symmetric=True)


# ----------------------------------------------------------------------------- table
def _row(c):
    """(k, row text) of the first draw that serves."""
    for k in range(64):
        a = analyse(c, k)
        bad = _problems(a)
        if not bad:
            vals = ', '.join('None' if n not in a['ref'] else f"{a['e32'][n]:.3e}" for n in G.OUTS)
            return k, f"    '{G.case_id(c)}': ({k}, {vals}),"
        print(f'# {G.case_id(c)} k={k}: {"; ".join(bad)}', file=sys.stderr)
    raise SystemExit(f'{G.case_id(c)}: no draw serves')


def write_table():
    rows = [_row(c)[1] for c in ALL_CASES]
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_graph_fp64.py')
    with open(path) as f:
        text = f.read()
    block = '# E32-BEGIN\nE32 = {\n' + '\n'.join(rows) + '\n}\n# E32-END'
    text = re.sub(r'# E32-BEGIN\n.*?# E32-END', lambda m: block, text, flags=re.S)
    with open(path, 'w') as f:
        f.write(text)
    print(f'{len(rows)} rows written to {path}')


if __name__ == '__main__':
    if '--write-table' in sys.argv:
        write_table()
    else:
        print(__doc__)
