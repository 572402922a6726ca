"""Multi-task kernels (k_multiplier_tasks, k_prox_tasks) against the f64
oracle, and the batched GPU runs against the CPU f64 batched run."""

import math

import pytest
import torch

from sparkagd_amd import (
    AGDConfig, CSRShard, DenseShard, LogisticGradient, MultiTaskGradient,
    PerTaskUpdater, SquaredL2Updater, assign_folds, cross_validate,
    generate_dense_problem, ops, run,
)
from sparkagd_amd.data import generate_csr_problem
from sparkagd_amd.ops import multitask as mt
from sparkagd_amd.ops import reference
from sparkagd_amd.ops.multiclass import padded_k

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOSSES = [ops.LOSS_LOGISTIC, ops.LOSS_LEAST_SQUARES, ops.LOSS_HINGE,
          ops.LOSS_SMOOTH_HINGE]
N_FOLDS = 3


def _multiplier_inputs(n, r, loss_type):
    g = torch.Generator().manual_seed(1000 * n + 10 * r + loss_type)
    kc = padded_k(r)
    z = torch.zeros(n, kc)
    z[:, :r] = 2.0 * torch.randn(n, r, generator=g)
    # junk in the pad columns must not leak into M or the losses
    z[:, r:] = 7.0
    if loss_type == ops.LOSS_LEAST_SQUARES:
        labels = torch.randn(n, generator=g)
    else:
        labels = (torch.rand(n, generator=g) < 0.5).to(torch.float32)
    mask = (torch.rand(n, generator=g) < 0.7).to(torch.uint8)
    sw = 0.5 + torch.rand(n, generator=g)
    fold = torch.randint(0, N_FOLDS, (n,), generator=g, dtype=torch.int32)
    holdout = torch.tensor([(t % (N_FOLDS + 1)) - 1 for t in range(r)],
                           dtype=torch.int32)  # -1, 0, 1, 2, -1, ...
    scale = (1.0 + torch.rand(r, generator=g)).to(torch.float32)
    return z, labels, mask, sw, fold, holdout, scale


def _check_multiplier(n, r, loss_type, use_extras, invert):
    z, labels, mask, sw, fold, holdout, scale = _multiplier_inputs(n, r, loss_type)
    kc = padded_k(r)
    extras = (mask, sw, fold, holdout) if use_extras else (None,) * 4
    dev = [None if t is None else t.to(DEV) for t in extras]
    zf = z.reshape(-1).to(DEV)
    M, tl, lc = mt.multiplier_tasks(zf, labels.to(DEV), loss_type, r,
                                    scale.to(DEV), *dev, invert=invert)
    M_ref, tl_ref, lc_ref = mt.ref_multiplier_tasks(
        z[:, :r].double(), labels.double(), loss_type, scale.double(),
        *extras, invert=invert)
    tag = (n, r, loss_type, use_extras, invert)
    M2 = M.reshape(n, kc)
    torch.testing.assert_close(M2[:, :r].double().cpu(), M_ref,
                               rtol=3e-4, atol=3e-4, msg=lambda s: f"{tag} {s}")
    assert torch.equal(M2[:, r:], torch.zeros_like(M2[:, r:])), tag
    torch.testing.assert_close(tl.cpu(), tl_ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lc.cpu(), lc_ref, rtol=1e-5, atol=1e-5)
    # loss_count[0] is the scaled sum of task_loss, in f64
    want = float((scale.double() * tl.cpu()).sum())
    assert abs(float(lc[0]) - want) <= 1e-12 * max(abs(want), 1e-300), tag
    # run-to-run bitwise reproducibility
    M_b, tl_b, lc_b = mt.multiplier_tasks(zf, labels.to(DEV), loss_type, r,
                                          scale.to(DEV), *dev, invert=invert)
    assert torch.equal(M, M_b) and torch.equal(tl, tl_b) and torch.equal(lc, lc_b), tag
    # loss-only call: M is neither allocated nor stored, the sums are the same
    M_n, tl_n, lc_n = mt.multiplier_tasks(zf, labels.to(DEV), loss_type, r,
                                          scale.to(DEV), *dev, invert=invert,
                                          need_mult=False)
    assert M_n is None
    assert torch.equal(tl, tl_n) and torch.equal(lc, lc_n), tag


@pytest.mark.parametrize("r", [1, 3, 4, 5, 8, 13, 16, 17, 32, 33, 40])
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_multiplier_tasks_matches_oracle(n, r):
    for loss_type in LOSSES:
        _check_multiplier(n, r, loss_type, use_extras=False, invert=False)
        _check_multiplier(n, r, loss_type, use_extras=True, invert=False)
        _check_multiplier(n, r, loss_type, use_extras=True, invert=True)


def test_multiplier_tasks_many_blocks_and_wide():
    """More rows than one grid-stride trip covers at the grid cap, and a
    column count past one 256-column chunk of the generic kernel."""
    _check_multiplier(300_000, 16, ops.LOSS_LOGISTIC, True, False)
    _check_multiplier(5000, 300, ops.LOSS_SMOOTH_HINGE, True, False)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("d,r", [(1, 7), (1000, 5), (4096, 16)])
@pytest.mark.parametrize("kind", [ops.PROX_SIMPLE, ops.PROX_L1,
                                  ops.PROX_SQUARED_L2, ops.PROX_ELASTIC_NET])
def test_prox_tasks_matches_oracle(kind, d, r, dtype):
    g = torch.Generator().manual_seed(17 * d + r)
    w = torch.randn(d * r, generator=g, dtype=dtype)
    gr = torch.randn(d * r, generator=g, dtype=dtype)
    lam = torch.rand(r, generator=g, dtype=torch.float64)
    lam2 = (torch.rand(r, generator=g, dtype=torch.float64)
            if kind == ops.PROX_ELASTIC_NET else torch.zeros(r, dtype=torch.float64))
    out_h, reg_h = mt.prox_tasks(kind, w.to(DEV), gr.to(DEV), 0.37, lam, lam2)
    out_r, reg_r = mt.ref_prox_tasks(kind, w, gr, 0.37, lam, lam2)
    # atol = rtol as tests/test_gpu_kernels.py::test_prox: the operands are
    # O(1), so an absolute error of a few ulp(1) is the format's precision
    # where the soft-threshold cancels
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    torch.testing.assert_close(out_h.cpu(), out_r, rtol=tol, atol=tol)
    torch.testing.assert_close(reg_h.cpu(), reg_r, rtol=tol, atol=0.0)
    out_b, reg_b = mt.prox_tasks(kind, w.to(DEV), gr.to(DEV), 0.37, lam, lam2)
    assert torch.equal(out_h, out_b) and torch.equal(reg_h, reg_b)


# --- end to end: the separable-trajectory configuration ---

LAMBDAS = (0.01, 0.1, 1.0)


def _tasks():
    holdout = [f for _ in LAMBDAS for f in range(N_FOLDS)] + [-1]
    lams = [lam for lam in LAMBDAS for _ in range(N_FOLDS)] + [0.1]
    return holdout, lams


def _batched_run(shard, folds, frob_sq, wdtype):
    holdout, lams = _tasks()
    r = len(holdout)
    # the CPU suite's L0 = 2|A|_F^2/140 + 1 at n = 240, scaled to this n
    L0 = 2.0 * frob_sq / (shard.n * 140.0 / 240.0) + 1.0
    grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
    return run(shard, grad, PerTaskUpdater(SquaredL2Updater(), lams), 0.0, 25,
               1.0, torch.zeros(shard.d * r, dtype=wdtype, device=shard.device),
               L0, math.inf, 1.0, 1.0, False)


def test_batched_run_f32_dense_matches_cpu():
    src, _ = generate_dense_problem(n=2048, d=256, seed=0)
    folds = assign_folds(src.n, N_FOLDS, seed=1)
    frob = float(src.features.double().norm() ** 2)
    cpu = DenseShard(src.features.double(), src.labels)
    gpu = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    wc, hc = _batched_run(cpu, folds, frob, torch.float64)
    wg, hg = _batched_run(gpu, folds, frob, torch.float32)
    assert len(hc) == len(hg) == 25
    assert abs(hc[-1] - hg[-1]) <= 1e-3 * abs(hc[-1])
    torch.testing.assert_close(wg.double().cpu(), wc, rtol=5e-3, atol=5e-3)


def test_batched_run_csr_matches_cpu():
    src, _ = generate_csr_problem(n=2048, d=256, nnz_per_row=8, seed=0)
    folds = assign_folds(src.n, N_FOLDS, seed=1)
    frob = float(src.val.double().norm() ** 2)
    cpu = CSRShard(src.rowptr, src.col, src.val.double(), src.labels, src.d)
    gpu = CSRShard(src.rowptr.to(DEV), src.col.to(DEV), src.val.to(DEV),
                   src.labels.to(DEV), src.d)
    wc, hc = _batched_run(cpu, folds, frob, torch.float64)
    wg, hg = _batched_run(gpu, folds, frob, torch.float32)
    assert len(hc) == len(hg) == 25
    assert abs(hc[-1] - hg[-1]) <= 1e-3 * abs(hc[-1])
    torch.testing.assert_close(wg.double().cpu(), wc, rtol=5e-3, atol=5e-3)


def test_batched_run_bf16_gemm_route_matches_cpu():
    """bf16 shard through the hipBLASLt margins/grad GEMMs against the CPU
    f64 run on the same bf16-valued data."""
    src, _ = generate_dense_problem(n=2048, d=256, seed=0, dtype=torch.bfloat16)
    folds = assign_folds(src.n, N_FOLDS, seed=1)
    frob = float(src.features.double().norm() ** 2)
    cpu = DenseShard(src.features.double(), src.labels)
    gpu = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    wc, hc = _batched_run(cpu, folds, frob, torch.float64)
    wg, hg = _batched_run(gpu, folds, frob, torch.float32)
    assert len(hc) == len(hg) == 25
    for i, (a, b) in enumerate(zip(hc, hg)):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (i, a, b)
    num = float(torch.norm(wg.double().cpu() - wc))
    den = float(torch.norm(wc)) + 1e-30
    assert num / den < 1e-2, (num, den)


def test_cross_validate_bf16_on_gpu():
    src, _ = generate_dense_problem(n=4096, d=512, seed=3, dtype=torch.bfloat16,
                                    label_noise=1.0)
    lams = [1e-4, 3e-3, 1e-1]
    cfg = AGDConfig(loss_history_mode="backtrack")
    gpu = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    res = cross_validate(gpu, lams, n_folds=3, num_iterations=20, config=cfg,
                         seed=5)
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
    cpu = DenseShard(feats, src.labels)
    ref = cross_validate(cpu, lams, n_folds=3, num_iterations=20, config=cfg,
                         seed=5, refit=False)
    assert res.best_lambda == ref.best_lambda
    assert res.model.link == "logistic"
    assert res.model.weights.shape == (512,) and res.model.weights.is_cuda
