"""The fused eval graph stack with its topology plan (a2m_graph_stack_fwd_ex2_f32): against the
oracle's layer-by-layer PyG restatement, built as test_gpu_parity.py::test_graph_stack_vs_oracle
builds it, against the plan = None path, in bf16 operand mode and replayed from a captured graph.

Frame counts: hand (J = 42, 3 frames a tile) 1 / 3 / 4 / 7 frames = a partial-only tile, exactly
one tile, a full + a partial tile (two wave rotations), all four rotations with a partial tail;
body (J = 10, 12 a tile) 12 / 13; a J = 9 star (14 a tile; one node with 7 in-edges, the only way
to the kernels' 8-slot instantiation, and leaves of in-degree 0) 14 / 15.

Error of the fp32 kernel against the float64 restatement (the edge softmax runs on the hardware
exp2 and reciprocal; printed by test_fp32_error_against_float64), measured on MI355X:
    body 13 fr: parent 4.036e-07, this kernel 6.306e-07      (PARENT_ERR below holds the parent's)
    hand 7 fr:  parent 6.791e-07, this kernel 6.475e-07
    star 15 fr: parent 3.544e-07, this kernel 3.544e-07
The restatement's own fp32 evaluation is at 2.4e-07 ... 3.1e-07 of the float64 one.
"""
import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = 'cuda'
# the parent commit's fp32 kernel (precise expf, IEEE division) against the float64 restatement on
# the largest case of each skeleton: the rule is new < 1e-4 and new < 2 x parent
PARENT_ERR = {'body': 4.036e-07, 'hand': 6.791e-07, 'star': 3.544e-07}
CASES = [('hand', 1), ('hand', 3), ('hand', 4), ('hand', 7), ('body', 12), ('body', 13), ('star', 14), ('star', 15)]
LARGEST = {'hand': 7, 'body': 13, 'star': 15}


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).float()


def _skeleton(name):
    from a2m import skeleton as S
    if name == 'star':   # leaves 1..7 -> hub 0; node 8 isolated
        return 9, torch.tensor([list(range(1, 8)), [0] * 7], dtype=torch.long)
    J, lo = (10, 0) if name == 'body' else (42, 10)
    return J, S.edge_index(lo, J)


_cache = {}


def _case(name, Fr):
    """Inputs, parameters and the oracle's fp32 / float64 results of one case, built once."""
    if (name, Fr) in _cache:
        return _cache[name, Fr]
    from a2m import skeleton as S
    from oracle import model as OM
    J, ei = _skeleton(name)
    x = _rand(Fr * J, 64, seed=80)
    edges = OM.expand_edges(ei, J, Fr)
    ptr, idx = S.in_neighbour_csr(ei, J)
    params = []
    for L in range(5):
        lnw, lnb = _rand(64, seed=90 + L).abs() + .5, _rand(64, seed=95 + L, scale=0.1)
        if L % 2 == 0:
            params.append((0, _rand(256, 64, seed=100 + L, scale=0.15), _rand(1, 4, 64, seed=110 + L, scale=0.3),
                           _rand(1, 4, 64, seed=120 + L, scale=0.3), _rand(64, seed=130 + L, scale=0.1), lnw, lnb))
        else:
            params.append((1, _rand(64, 64, seed=140 + L, scale=0.12), _rand(64, seed=150 + L, scale=0.1),
                           _rand(64, 64, seed=160 + L, scale=0.12), None, lnw, lnb))

    def oracle(dt):
        ref = x.to(dt)
        for P in params:
            t = [None if v is None else v.to(dt) for v in P[1:]]
            if P[0] == 0:
                g = OM._gat_fn(ref, edges, t[0], t[1], t[2], t[3], 4)
            else:
                g = OM.graph_conv(OM.Ctx({'g.lin_rel.weight': t[0], 'g.lin_rel.bias': t[1],
                                          'g.lin_root.weight': t[2]}), 'g', ref, edges)
            ref = torch.nn.functional.leaky_relu(torch.nn.functional.layer_norm(g, (64,), t[4], t[5]), 0.2) + ref
        return ref

    c = dict(J=J, x=x, ptr=ptr, idx=idx, params=params, ref=oracle(torch.float32), ref64=oracle(torch.float64))
    _cache[name, Fr] = c
    return c


def _device_side(c):
    """The case's device tensors: x, CSR, the stack's layer tuples and (where the library has the
    plan entry points) the plan."""
    from a2m import functional as F
    if 'dev' not in c:
        dv = lambda t: t.to(DEV)  # noqa: E731
        layers = []
        for P in c['params']:
            if P[0] == 0:
                lw = dv(P[1])
                layers.append((0, lw, None, F.graph_att_proj(lw, dv(P[2]), dv(P[3])), dv(P[4]), dv(P[5]), dv(P[6])))
            else:
                layers.append((1, dv(P[1]), dv(P[3]), None, dv(P[2]), dv(P[5]), dv(P[6])))
        plan = dv(F.graph_stack_plan(c['J'], c['ptr'], c['idx'])) \
            if hasattr(F.N.lib, 'a2m_graph_stack_fwd_ex2_f32') else None
        c['dev'] = (dv(c['x']), dv(c['ptr']), dv(c['idx']), layers, plan)
    return c['dev']


@pytest.mark.parametrize('name,Fr', CASES)
def test_plan_stack_vs_oracle_and_no_plan(name, Fr):
    from a2m import functional as F
    c = _case(name, Fr)
    x, ptr, idx, layers, plan = _device_side(c)
    J = c['J']
    out = F.graph_stack(x, J, ptr, idx, layers, plan=plan).cpu()
    base = F.graph_stack(x, J, ptr, idx, layers).cpu()
    e, e0 = rel_err(out, c['ref']), rel_err(base, c['ref'])
    print(f'{name} {Fr} frames: plan {e:.2e}, no plan {e0:.2e} vs oracle; '
          f'plan vs no plan {rel_err(out, base):.2e}, bitwise {torch.equal(out, base)}')
    assert e < TOL and e0 < TOL, (e, e0)
    if Fr % (128 // J) == 0:
        assert torch.equal(out, base)
    else:   # a partial last tile: its live rows sit in other MFMA rows than the in-kernel build's
        assert torch.equal(out, base) or rel_err(out, base) < 2e-6, rel_err(out, base)


@pytest.mark.parametrize('name', ['body', 'hand', 'star'])
def test_fp32_error_against_float64(name):
    """The fp32 kernel against the restatement evaluated in float64.  Also runs on an older library
    selected with A2M_LIB (no plan there), which is how PARENT_ERR was measured."""
    from a2m import functional as F
    c = _case(name, LARGEST[name])
    x, ptr, idx, layers, plan = _device_side(c)
    kw = {} if plan is None else {'plan': plan}
    out = F.graph_stack(x, c['J'], ptr, idx, layers, **kw).cpu()
    e = rel_err(out.double(), c['ref64'])
    print(f'graph_stack fp32 rel_err vs float64 oracle: {name} {LARGEST[name]} frames {e:.3e} '
          f'(oracle fp32 vs float64 {rel_err(c["ref"].double(), c["ref64"]):.3e})')
    assert e < TOL and e < 2 * PARENT_ERR[name], e


@pytest.mark.parametrize('name', ['body', 'hand', 'star'])
def test_plan_stack_bf16_mode(name):
    import a2m
    from a2m import functional as F
    c = _case(name, LARGEST[name])
    x, ptr, idx, layers, plan = _device_side(c)
    J = c['J']
    wh = [F.graph_weights_bf16(Lr[1], Lr[2], {}) for Lr in layers]
    prev = a2m.set_gemm_precision('bf16')
    try:
        out16 = F.graph_stack(x, J, ptr, idx, layers, plan=plan).cpu()
        out16h = F.graph_stack(x, J, ptr, idx, layers, wh=wh, plan=plan).cpu()
    finally:
        a2m.set_gemm_precision(prev)
    assert torch.equal(out16, out16h)
    e16 = rel_err(out16, c['ref'])
    print(f'{name}: bf16 stack with plan vs oracle {e16:.2e}')
    assert 1e-6 < e16 < 3e-2, e16


def test_plan_stack_replays_from_a_captured_graph():
    from a2m import functional as F
    c = _case('hand', 7)
    x, ptr, idx, layers, plan = _device_side(c)
    eager = F.graph_stack(x, 42, ptr, idx, layers, plan=plan)
    xin, out = x.clone(), torch.empty_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.graph_stack(xin, 42, ptr, idx, layers, out=out, plan=plan)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        F.graph_stack(xin, 42, ptr, idx, layers, out=out, plan=plan)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    xin.mul_(0.5)   # new input through the same captured launch
    g.replay()
    assert torch.equal(out, F.graph_stack(xin, 42, ptr, idx, layers, plan=plan))
