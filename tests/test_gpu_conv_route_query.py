"""The route query names the kernel that runs: for each branch of the conv1d front the route taken
from the matching query (a2m_conv1d_down_route / a2m_conv1d_wino_route, no launch) is held against
one F.conv1d launch's engine counts (a2m_gemm_kernel_counts: exactly one launch, of the kind the
route names) and against the packed-weight cache slot that the route's flags imply (the Winograd
bit: 'wino_w'; the down-sampling bit: 'down_w'; the tap-chunked operand, mode 5: 'w'; otherwise
the plain weights, no slot).

Cases (B, Ci, Co, Tin, k, s, p), the smallest at which each branch is reached: the gathered tile
(Co < 128), the explicit im2col with the dense route (Co >= 128), the down-sampling tile on the
same shape, the tap path and the Winograd tile on one shape, and the down-sampling tile over
partial M and N tiles.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

CASES = [
    ((2, 128, 64, 64, 4, 2, 1), False, None),      # the gathered tile: Co < 128
    ((2, 64, 128, 64, 4, 2, 1), False, None),      # im2col and the dense route
    ((2, 64, 128, 64, 4, 2, 1), True, 'down_w'),   # the down-sampling tile
    ((2, 64, 64, 32, 3, 1, 1), False, 'w'),        # the tap path
    ((2, 64, 64, 32, 3, 1, 1), True, 'wino_w'),    # the Winograd tile
    ((5, 64, 20, 16, 4, 2, 1), True, 'down_w'),    # partial tiles
]


@pytest.mark.parametrize('shape,request_tile,slot', CASES)
def test_route_query_names_the_kernel_that_runs(shape, request_tile, slot):
    from a2m import _native as N
    from a2m import functional as F
    B, Ci, Co, Tin, k, s, p = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Ci, Tin, generator=g).to(DEV)
    w = (torch.randn(Co, Ci, k, generator=g) / (Ci * k) ** 0.5).to(DEV)
    out = torch.empty(B, Co, (Tin + 2 * p - k) // s + 1, device=DEV)
    if k == 3:
        r = F.conv1d_wino_route(x, Co, out, wino=request_tile)
    else:
        r = F.conv1d_down_route(x, Co, out, down=request_tile, ks=k, stride=s, pad=p)
    assert r is not None
    implied = {'wino_w'} if r['flags'] & F.ROUTE_WINO else {'down_w'} if r['flags'] & F.ROUTE_DOWN else \
        {'w'} if r['mb'] == 5 else set()
    assert implied == ({slot} if slot else set()), (r, slot)
    cache = {}
    c = (ctypes.c_int64 * 4)()
    N.check(N.lib.a2m_gemm_kernel_counts(c, 1))
    F.conv1d(x, w, None, s, p, out=out, cache=cache, wino=request_tile)
    N.check(N.lib.a2m_gemm_kernel_counts(c, 1))
    print(f'{shape} requested={request_tile}: route {r} counts {list(c)} cache {sorted(cache)}')
    assert list(c) == [int(i == r['kind']) for i in range(4)], (list(c), r)
    assert {n for n in ('w', 'wino_w', 'down_w') if n in cache} == implied, (sorted(cache), r)
