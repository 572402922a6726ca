"""fp8 multi-column MFMA kernels (k_margins_multi_f8, k_grad_multi_f8): the
decode and lane maps bit for bit, both passes against f64, and the softmax /
CV-sweep routes that an fp8 shard with more than 32 columns could not take."""

import pytest
import torch

from sparkagd_amd import (
    AGDConfig, DenseShard, SoftmaxRegressionWithAGD, assign_folds,
    cross_validate, generate_dense_problem, ops,
)
from sparkagd_amd.data import generate_multiclass_problem
from sparkagd_amd.ops import reference
from sparkagd_amd.ops.multiclass import margins_multi, padded_k

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F8 = torch.float8_e4m3fn
# n: a row tail below one 32-row block, one row past a block, a ragged third
# block; d: one 16-byte load unit, one unit past a 128/256-column step, enough
# steps that the margins slab split engages; K: KC 4 and 16 in one 32-class
# tile, 2 and 4 tiles, a second class group
GRID = [(n, d, k) for n in (1, 33, 80) for d in (16, 272, 4112)
        for k in (3, 16, 33, 100, 150)]


def _fp8_shard(n, d):
    """(fp8 features on the GPU, the same values as f64 on the CPU)."""
    g = torch.Generator().manual_seed(7919 * n + d)
    x = torch.randn(n, d, generator=g).to(F8)
    return x.to(DEV), x.float().double()


def test_decode_and_lane_maps_are_exact():
    """Every e4m3 code (NaN codes replaced by 0) in every lane position, in a
    different rotation per row, through products by 1 and 0."""
    codes = (torch.arange(256)[None, :] + 37 * torch.arange(32)[:, None]) % 256
    codes[(codes & 0x7F) == 0x7F] = 0
    a = codes.to(torch.uint8).view(F8)
    want = a.float()
    grad = ops.grad_multi_fp8(a.to(DEV), torch.eye(32).reshape(-1).to(DEV), 32)
    assert torch.equal(grad.reshape(256, 32).cpu(), want.T)
    z = ops.margins_multi_fp8(a.to(DEV), torch.eye(256).reshape(-1).to(DEV), 256)
    assert torch.equal(z.reshape(32, 256).cpu(), want)


@pytest.mark.parametrize("n,d,k", GRID)
def test_margins_against_f64(n, d, k):
    feats, a = _fp8_shard(n, d)
    w = torch.randn(d, k, generator=torch.Generator().manual_seed(k))
    kc = padded_k(k)
    wflat = w.reshape(-1).to(DEV)
    # routing is opt-in up to 32 padded columns: call the op there
    z = (margins_multi(feats, wflat, k) if kc > 32
         else ops.margins_multi_fp8(feats, wflat, k))
    z = z.reshape(n, kc).cpu()
    # residue of the bf16 hi + lo split of W, then f32 accumulation over d
    bound = (2.0 ** -16 + d * 2.0 ** -24) * (a.abs() @ w.double().abs())
    err = (z[:, :k].double() - a @ w.double()).abs()
    print(f"max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((z[:, k:] == 0).all())


@pytest.mark.parametrize("split", [False, True], ids=["bf16_m", "split_m"])
@pytest.mark.parametrize("n,d,k", GRID)
def test_gradient_against_f64(n, d, k, split):
    """split=False: against Aᵀ·bf16(M), f32 accumulation over n alone;
    split=True (what the solver routes run): against Aᵀ·M, plus 2^-16 for the
    residue of the hi + lo split."""
    feats, a = _fp8_shard(n, d)
    kc = padded_k(k)
    m = torch.zeros(n, kc)
    m[:, :k] = torch.randn(n, k, generator=torch.Generator().manual_seed(k + 1))
    m0 = m.clone()
    m0[n // 2] = 0.0  # a zero row changes nothing else
    for mm in (m, m0):
        mflat = mm.reshape(-1).to(DEV)
        grad = ops.grad_multi_fp8(feats, mflat, k, split_m=split)
        assert torch.equal(grad, ops.grad_multi_fp8(feats, mflat, k, split_m=split))
        mref = mm[:, :k] if split else mm[:, :k].bfloat16()
        want = a.T @ mref.double()
        rel = 2.0 * n * 2.0 ** -24 + (2.0 ** -16 if split else 0.0)
        bound = rel * (a.abs().T @ mm[:, :k].double().abs())
        err = (grad.reshape(d, k).double().cpu() - want).abs()
        print(f"max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())


def test_softmax_40_classes_on_fp8_matches_cpu():
    src, _ = generate_multiclass_problem(2048, 256, 40, seed=0)
    f8 = src.features.to(F8)
    kw = dict(num_classes=40, num_iterations=10, reg_param=1e-3,
              convergence_tol=0.0)
    got = SoftmaxRegressionWithAGD.train(
        DenseShard(f8.to(DEV), src.labels.to(DEV)), **kw)
    want = SoftmaxRegressionWithAGD.train(
        DenseShard(f8.float().double(), src.labels), **kw)
    assert len(got.loss_history) == len(want.loss_history) == 10
    for i, (a, b) in enumerate(zip(want.loss_history, got.loss_history)):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (i, a, b)


def test_cross_validate_36_tasks_on_fp8():
    """3 lambdas x 12 folds = 36 columns. Seed 3 / fold seed 5: the f64 run's
    mean held-out losses of the two best lambdas differ by far more than the
    1e-4 scoring tolerance (checked on the CPU), so best_lambda is decided."""
    src, _ = generate_dense_problem(n=4096, d=512, seed=3, label_noise=1.0)
    f8 = src.features.to(F8)
    feats = f8.float().double()
    lams = [1e-4, 3e-3, 1e-1]
    cfg = AGDConfig(loss_history_mode="backtrack")
    res = cross_validate(DenseShard(f8.to(DEV), src.labels.to(DEV)), lams,
                         n_folds=12, num_iterations=20, config=cfg, seed=5)
    folds = assign_folds(src.n, 12, seed=5)
    for li in range(3):
        for f in range(12):
            rows = folds == f
            _, loss = reference._multiplier_and_loss(
                feats[rows] @ res.fold_weights[li, f].double().cpu(),
                src.labels[rows].double(), ops.LOSS_LOGISTIC)
            want = float(loss.mean())
            got = float(res.heldout_loss[li, f])
            assert abs(got - want) <= 1e-4 * want, (lams[li], f, got, want)
    ref = cross_validate(DenseShard(feats, src.labels), lams, n_folds=12,
                         num_iterations=20, config=cfg, seed=5, refit=False)
    assert res.best_lambda == ref.best_lambda
