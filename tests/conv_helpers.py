"""Helpers shared by the conv1d GPU tests (test_gpu_wino_conv.py, test_gpu_down_conv.py,
test_gpu_tapconv.py): seeded BatchNorm-eval parameters on the device, the planner-override fixture
and the fp64 BN-eval + LeakyReLU reference."""
import pytest
import torch

DEV = 'cuda'


def bn_params(Co, g):
    """(weight, bias, running mean, running var, eps) of a BatchNorm in eval mode, drawn from g."""
    return tuple(t.to(DEV) for t in (torch.rand(Co, generator=g) + 0.5, torch.randn(Co, generator=g),
                                     torch.randn(Co, generator=g) * 0.1, torch.rand(Co, generator=g) + 0.5)) + (1e-5,)


def bn_lrelu_ref(z, bn, slope=0.2):
    """fp64 BN-eval affine + LeakyReLU of z [B, C, T] (fp64) with the parameters of bn_params."""
    wq, bq, rm, rv, eps = (t.cpu().double() if torch.is_tensor(t) else t for t in bn)
    z = (z - rm.view(1, -1, 1)) / torch.sqrt(rv.view(1, -1, 1) + eps) * wq.view(1, -1, 1) + bq.view(1, -1, 1)
    return torch.where(z > 0, z, slope * z)


@pytest.fixture
def plan_override():
    from a2m import _native as N

    def set_plan(tile, splits):
        N.check(N.lib.a2m_gemm_plan_override(tile, splits))
    yield set_plan
    N.check(N.lib.a2m_gemm_plan_override(0, 0))
