"""k_at_step_tail against the kernel sequence it replaces (prox, axpby,
fused_scalars, reg_value): torch.equal on z, x and all six scalars."""

import pytest
import torch

from sparkagd_amd import ops

pytestmark = pytest.mark.gpu

# 16-B body / scalar tail boundaries (f32: 4 per vector, f64: 2), more than
# one block, and one size past the 8192-block grid cap (grid-stride loop)
SIZES = [1, 3, 4, 5, 1023, 4099]
PAST_GRID_CAP = 8192 * 256 * 4 + 7
KINDS = [ops.PROX_SIMPLE, ops.PROX_SQUARED_L2]


def _inputs(d, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    v = [torch.randn(d, generator=g, dtype=torch.float64).to(dtype).cuda()
         for _ in range(4)]
    return v  # x_old, z_old, y, g_y


def _sequence(kind, x_old, z_old, y, g_y, theta, step, lam):
    z, _ = ops.prox(kind, z_old, g_y, step, lam)
    x = ops.axpby(1.0 - theta, x_old, theta, z)
    scal = ops.fused_scalars(x, y, g_y, x_old)
    _, reg = ops.prox(kind, x, torch.zeros_like(x), 0.0, lam)
    return z, x, torch.cat([scal, reg.reshape(1)])


def _check(kind, vecs, theta, step, lam):
    x_old, z_old, y, g_y = vecs
    z0, x0, s0 = _sequence(kind, x_old, z_old, y, g_y, theta, step, lam)
    # a slice of a larger block, as run() passes it; NaN where the kernel
    # must overwrite, a sentinel where it must not write
    block = torch.full((11,), float("nan"), dtype=torch.float64, device="cuda")
    block[6:] = 7.0
    z1, x1 = ops.at_step_tail(kind, x_old, z_old, y, g_y, theta, step, lam,
                              block[0:6])
    assert torch.equal(z1, z0)
    assert torch.equal(x1, x0)
    assert torch.equal(block[0:6], s0), (block[0:6].tolist(), s0.tolist())
    assert torch.equal(block[6:], torch.full_like(block[6:], 7.0))
    # a second call into the same block overwrites, it does not accumulate
    ops.at_step_tail(kind, x_old, z_old, y, g_y, theta, step, lam, block[0:6])
    assert torch.equal(block[0:6], s0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("theta", [1.0, 0.37])
@pytest.mark.parametrize("d", SIZES)
def test_matches_kernel_sequence(d, theta, kind, dtype):
    _check(kind, _inputs(d, dtype, seed=d), theta, 0.73, 1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_past_the_grid_cap(kind, dtype):
    _check(kind, _inputs(PAST_GRID_CAP, dtype, seed=1), 0.37, 0.73, 1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind", KINDS)
def test_zeros_and_negative_shrink(kind, dtype):
    """Exact zeros in every input, and lam large enough that 1 - step*lam
    is negative."""
    vecs = _inputs(4099, dtype, seed=2)
    for i, v in enumerate(vecs):
        v[i::3] = 0.0
    vecs[1][:7] = 0.0
    vecs[3][:7] = 0.0
    _check(kind, vecs, 0.37, 0.73, 5.0)  # 1 - 0.73*5 < 0
