"""Times the fused eval graph stack (a2m_graph_stack_fwd_f32: GAT, GraphConv, GAT, GraphConv,
GAT) at the bench shapes: hand (J=42) and body (J=10) over B*T = 4096 frames, each alone on the
chip.
    python tools/stack_bench.py [hand|body|both] [iters] [bf16 [nowh]] [noplan]
The topology plan (a2m_graph_stack_plan_build) is passed as the model passes it, unless `noplan`
is given or the library (an older one selected with A2M_LIB) has no plan entry points."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'audio-to-motion-generation_amd'))
import torch  # noqa: E402

from a2m import functional as F  # noqa: E402
from a2m import skeleton as S  # noqa: E402

dev = torch.device('cuda')
FR = 4096
argv = [a for a in sys.argv[1:] if a not in ('bf16', 'nowh', 'noplan')]
if 'bf16' in sys.argv[1:]:   # the bf16 operand mode's stack (layer products on the bf16 MFMA)
    import a2m
    a2m.set_gemm_precision('bf16')
which = argv[0] if len(argv) > 0 else 'both'
iters = int(argv[1]) if len(argv) > 1 else 20
g = torch.Generator(device='cpu').manual_seed(0)


def rnd(*s, scale=1.0):
    return (torch.randn(*s, generator=g) * scale).to(dev)


for name, J, lo in (('hand', 42, 10), ('body', 10, 0)):
    if which not in ('both', name):
        continue
    hptr, hidx = S.in_neighbour_csr(S.edge_index(lo, J), J)
    ptr, idx = hptr.to(dev), hidx.to(dev)
    plan = None
    if 'noplan' not in sys.argv[1:] and hasattr(F.N.lib, 'a2m_graph_stack_fwd_ex2_f32'):
        plan = F.graph_stack_plan(J, hptr, hidx).to(dev)
    x = rnd(FR * J, 64)
    layers = []
    for L in range(5):
        lnw, lnb = rnd(64).abs() + .5, rnd(64, scale=0.1)
        if L % 2 == 0:
            lw = rnd(256, 64, scale=0.15)
            U = F.graph_att_proj(lw, rnd(1, 4, 64, scale=0.3), rnd(1, 4, 64, scale=0.3))
            layers.append((0, lw, None, U, rnd(64, scale=0.1), lnw, lnb, {}))
        else:
            layers.append((1, rnd(64, 64, scale=0.12), rnd(64, 64, scale=0.12), None, rnd(64, scale=0.1), lnw, lnb, {}))
    out = torch.empty_like(x)
    # bf16 mode: the layer weights' cached bf16 copies, as the model passes them (nowh: without)
    wh = [F.graph_weights_bf16(Lr[1], Lr[2], {}) for Lr in layers] \
        if 'bf16' in sys.argv[1:] and 'nowh' not in sys.argv[1:] else None
    kw = {} if plan is None else {'plan': plan}
    for _ in range(3):
        F.graph_stack(x, J, ptr, idx, layers, out=out, wh=wh, **kw)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        F.graph_stack(x, J, ptr, idx, layers, out=out, wh=wh, **kw)
    e1.record()
    e1.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    gf = FR * J * 64 * 64 * 2 * (3 * 4 + 2 * 2) / 1e9
    print(f'{name} stack{"" if plan is None else " (plan)"}: {us:.1f} us/launch, {gf:.2f} GFLOP of MFMA work, {gf / us * 1e3:.1f} TF', flush=True)
