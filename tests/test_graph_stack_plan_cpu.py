"""The fused graph stack's topology plan (a2m_graph_stack_plan_build): pure host code, checked
against a restatement of the tables graph_stack_kernel builds in LDS without a plan -- the
degree-sorted stable row order, the in-degrees and the tile-local gather slots -- for the body
and hand skeletons and a J = 9 star (one node with 7 in-edges, the kernels' limit; its leaves
have in-degree 0)."""
import numpy as np
import pytest
import torch

from conftest import REPO  # noqa: F401  (puts the package on sys.path)

ROW, ROWS, SLOTS = 12, 128, 8


def star_edges(J):
    """Leaves 1..7 -> hub 0 (in-degree 7); any further node is isolated."""
    return torch.tensor([[i for i in range(1, 8)], [0] * 7], dtype=torch.long)


def skeletons():
    from a2m import skeleton as S
    return [('body', 10, S.edge_index(0, 10)), ('hand', 42, S.edge_index(10, 42)), ('star', 9, star_edges(9))]


@pytest.mark.parametrize('name,J,ei', skeletons(), ids=lambda v: v if isinstance(v, str) else None)
def test_plan_tables(name, J, ei):
    from a2m import functional as F
    from a2m import skeleton as S
    ptr, idx = S.in_neighbour_csr(ei, J)
    plan = F.graph_stack_plan(J, ptr, idx)
    assert plan.dtype == torch.uint8 and plan.numel() == ROWS * ROW
    rows = plan.numpy().reshape(ROWS, ROW)
    ptr, idx = ptr.tolist(), idx.tolist()
    nb = (128 // J) * J
    node, deg = rows[:, 0].astype(int), rows[:, 1].astype(int)
    # the row order is a permutation of the tile's nodes; padding rows carry 0xff and nothing else
    assert sorted(node[:nb].tolist()) == list(range(nb))
    assert (node[nb:] == 0xff).all() and not rows[nb:, 1:].any()
    assert not rows[:, 10:].any()
    # degree non-increasing along the order, stable by node index within one degree
    want_deg = [ptr[n % J + 1] - ptr[n % J] for n in node[:nb]]
    assert deg[:nb].tolist() == want_deg
    assert all(deg[p] > deg[p + 1] or (deg[p] == deg[p + 1] and node[p] < node[p + 1]) for p in range(nb - 1))
    # slots: the CSR in-neighbours in edge order as tile-local indices, the node at slot d, 0 after
    for p in range(nb):
        n, d = node[p], deg[p]
        f0, ln = n - n % J, n % J
        want = [f0 + s for s in idx[ptr[ln]:ptr[ln + 1]]] + [n]
        want += [0] * (SLOTS - len(want))
        assert rows[p, 2:10].tolist() == want, (p, n)
    if name == 'star':
        assert deg[:nb // J].tolist() == [7] * (nb // J) and set(deg[nb // J:nb]) == {0}


def test_plan_refuses_topologies_over_the_limits():
    from a2m import functional as F
    # in-degree 8: one past the kernels' 7 (+ the GAT self loop)
    ptr = torch.tensor([0, 8] + [8] * 8, dtype=torch.int32)
    idx = torch.arange(1, 9, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'graph_stack: node 0 has in-degree 8: the graph kernels support at most 7'):
        F.graph_stack_plan(9, ptr, idx)
    # J = 129: the launch's own text
    with pytest.raises(ValueError, match=r'graph_stack: bad J=129'):
        F.graph_stack_plan(129, torch.zeros(130, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    # more CSR entries than the kernels stage: 100 nodes x 2 in-edges
    ptr = torch.arange(0, 201, 2, dtype=torch.int32)
    with pytest.raises(ValueError, match=r'graph_stack: 200 edges over 100 nodes'):
        F.graph_stack_plan(100, ptr, torch.zeros(200, dtype=torch.int32))
    # an edge from outside the graph
    with pytest.raises(ValueError, match=r'outside \[0, 3\)'):
        F.graph_stack_plan(3, torch.tensor([0, 1, 1, 1], dtype=torch.int32), torch.tensor([3], dtype=torch.int32))


def test_plan_bytes_and_short_buffer():
    import ctypes
    from a2m import _native as N
    from a2m import skeleton as S
    ptr, idx = S.in_neighbour_csr(S.edge_index(0, 10), 10)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    assert N.lib.a2m_graph_stack_plan_bytes(10, p(ptr), p(idx)) == ROWS * ROW
    assert N.lib.a2m_graph_stack_plan_bytes(129, p(ptr), p(idx)) == 0
    buf = np.zeros(ROWS * ROW - 1, np.uint8)
    assert N.lib.a2m_graph_stack_plan_build(10, p(ptr), p(idx), buf.ctypes.data_as(ctypes.c_void_p), buf.size) == N.A2M_EINVAL
    assert 'plan buffer' in N.last_error()


def test_model_keeps_the_plans_as_non_persistent_buffers():
    from a2m import functional as F
    from a2m.real_motion_model import SelfAttention_G
    g = SelfAttention_G(p=0.0)
    for part, J in (('body', 10), ('hand', 42)):
        ptr, idx = g.topology(part)
        assert torch.equal(g.stack_plan(part), F.graph_stack_plan(J, ptr, idx))
    assert not any('stack_plan' in k for k in g.state_dict())
