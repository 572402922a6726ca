"""Packed multi-column MFMA kernels (k_margins_multi_pk, k_grad_multi_pk and
their escape corrections) against f64, their routing from the multinomial
and multi-task gradients, and the packed CV sweep / softmax run end to end."""

import pytest
import torch

from sparkagd_amd import (
    AGDConfig, DenseShard, LogisticGradient, MultinomialLogisticGradient,
    MultiTaskGradient, SoftmaxRegressionWithAGD, assign_folds, cross_validate,
    generate_dense_problem, ops, packing,
)
from sparkagd_amd.data import generate_multiclass_problem
from sparkagd_amd.ops import hiplib, reference
from sparkagd_amd.ops.multiclass import padded_k

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# n: a row tail below one 32-row block, one row past a block, a ragged third
# block; d: one group, one group past a 256-column tile, enough 256-column
# steps that the margins slab split engages; K: KC 4 and 16 in one 32-class
# tile, then 2 and 4 tiles
GRID = [(n, d, k, esc) for n in (1, 33, 80) for d in (8, 264, 4104)
        for k in (3, 16, 33, 100) for esc in (False, True)]


def _packed_shard(n, d, esc, monkeypatch):
    """(packed GPU shard, its bf16 values as f64 on the CPU)."""
    monkeypatch.setattr(packing, "PACK_ESCAPE_CAP", 1.0)
    g = torch.Generator().manual_seed(7919 * n + d)
    x = torch.randn(n, d, generator=g)
    if esc:  # five planted escapes: binades far outside randn's table
        at = torch.randperm(n * d, generator=g)[:5]
        x.view(-1)[at] = 1e4 * (1.0 + torch.rand(at.numel(), generator=g))
    x = x.to(torch.bfloat16)
    shard = DenseShard(x.to(DEV), torch.zeros(n, device=DEV))
    assert shard.pack(), shard.pack_refused
    return shard, x.double()


@pytest.mark.parametrize("n,d,k,esc", GRID)
def test_margins_against_f64(n, d, k, esc, monkeypatch):
    shard, a = _packed_shard(n, d, esc, monkeypatch)
    g = torch.Generator().manual_seed(k)
    w = torch.randn(d, k, generator=g)
    kc = padded_k(k)
    z = ops.margins_multi_packed(shard._packed_gpu(), w.reshape(-1).to(DEV), k)
    z = z.reshape(n, kc).cpu()
    # residue of the bf16 hi + lo split of W, then f32 accumulation over d
    bound = (2.0 ** -16 + d * 2.0 ** -24) * (a.abs() @ w.double().abs())
    err = (z[:, :k].double() - a @ w.double()).abs()
    print(f"max err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert bool((z[:, k:] == 0).all())


@pytest.mark.parametrize("split", [False, True], ids=["bf16_m", "split_m"])
@pytest.mark.parametrize("n,d,k,esc", GRID)
def test_gradient_against_f64(n, d, k, esc, split, monkeypatch):
    """split=False: M rounded to bf16 once, against Aᵀ·bf16(M), f32
    accumulation over n alone. split=True (what the solver routes run): M as
    a bf16 hi + lo pair, against Aᵀ·M, with the margins test's 2^-16 for the
    residue of the split on top of the same accumulation term."""
    shard, a = _packed_shard(n, d, esc, monkeypatch)
    pk = shard._packed_gpu()
    kc = padded_k(k)
    g = torch.Generator().manual_seed(k + 1)
    m = torch.zeros(n, kc)
    m[:, :k] = torch.randn(n, k, generator=g)
    m0 = m.clone()
    m0[n // 2] = 0.0  # a zero row changes nothing else
    for mm in (m, m0):
        mflat = mm.reshape(-1).to(DEV)
        grad = ops.grad_multi_packed(pk, mflat, k, split_m=split)
        assert torch.equal(grad, ops.grad_multi_packed(pk, mflat, k, split_m=split))
        mref = mm[:, :k] if split else mm[:, :k].bfloat16()
        want = a.T @ mref.double()
        rel = 2.0 * n * 2.0 ** -24 + (2.0 ** -16 if split else 0.0)
        bound = rel * (a.abs().T @ mm[:, :k].double().abs())
        err = (grad.reshape(d, k).double().cpu() - want).abs()
        print(f"max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all())


@pytest.mark.parametrize("make", [
    lambda: MultinomialLogisticGradient(5),
    lambda: MultiTaskGradient(LogisticGradient(), 6),
], ids=["multinomial", "multitask"])
def test_packed_shard_leaves_the_gemm_route(make, monkeypatch):
    def gemm(*args, **kwargs):
        raise RuntimeError("hipBLASLt route taken")

    monkeypatch.setattr(hiplib, "gemm_bf16f32_nt", gemm)
    monkeypatch.setattr(hiplib, "gemm_bf16f32_tn", gemm)
    grad = make()
    k = grad.num_classes
    src, _ = generate_multiclass_problem(256, 64, 2, seed=1, dtype=torch.bfloat16)
    shard = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    w = 0.1 * torch.randn(64 * k, generator=torch.Generator().manual_seed(2))
    with pytest.raises(RuntimeError, match="hipBLASLt route taken"):
        grad.eval(shard, w.to(DEV))
    assert shard.pack(), shard.pack_refused
    g, lc = grad.eval(shard, w.to(DEV))
    assert g.shape == (64 * k,) and bool(torch.isfinite(g).all())
    assert float(lc[1]) == 256.0


def test_cross_validate_packed_bf16_on_gpu():
    """test_gpu_multitask.py::test_cross_validate_bf16_on_gpu with pack=True."""
    src, _ = generate_dense_problem(n=4096, d=512, seed=3, dtype=torch.bfloat16,
                                    label_noise=1.0)
    lams = [1e-4, 3e-3, 1e-1]
    cfg = AGDConfig(loss_history_mode="backtrack")
    gpu = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    res = cross_validate(gpu, lams, n_folds=3, num_iterations=20, config=cfg,
                         seed=5, pack=True)
    assert gpu.is_packed, gpu.pack_refused
    folds = assign_folds(src.n, 3, seed=5)
    feats = src.features.double()
    for li in range(3):
        for f in range(3):
            rows = folds == f
            _, loss = reference._multiplier_and_loss(
                feats[rows] @ res.fold_weights[li, f].double().cpu(),
                src.labels[rows].double(), ops.LOSS_LOGISTIC)
            want = float(loss.mean())
            got = float(res.heldout_loss[li, f])
            print(f"lambda {lams[li]} fold {f}: {got:.8f} vs torch {want:.8f}")
            assert abs(got - want) <= 1e-4 * want
    ref = cross_validate(DenseShard(feats, src.labels), lams, n_folds=3,
                         num_iterations=20, config=cfg, seed=5, refit=False)
    assert res.best_lambda == ref.best_lambda
    assert res.model.weights.shape == (512,) and res.model.weights.is_cuda


def test_softmax_on_packed_shard_matches_cpu():
    src, _ = generate_multiclass_problem(2048, 256, 5, seed=0,
                                         dtype=torch.bfloat16)
    gpu = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    kw = dict(num_classes=5, num_iterations=10, reg_param=1e-3,
              convergence_tol=0.0)
    got = SoftmaxRegressionWithAGD.train(gpu, pack=True, **kw)
    assert gpu.is_packed, gpu.pack_refused
    want = SoftmaxRegressionWithAGD.train(
        DenseShard(src.features.double(), src.labels), **kw)
    assert len(got.loss_history) == len(want.loss_history) == 10
    for i, (a, b) in enumerate(zip(want.loss_history, got.loss_history)):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (i, a, b)
