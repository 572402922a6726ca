"""Multi-task training (R binary problems in one shard stream) and k-fold
cross-validation — CPU tier, f64.

The stacked problem is separable, so every check here compares one column of
the batched computation with the single-task code on that task's rows."""

import math
import os
import subprocess
import sys

import pytest
import torch

from sparkagd_amd import (
    CSRShard, CVResult, DenseShard, ElasticNetUpdater, HingeGradient,
    InterceptShard, L1Updater, LeastSquaresGradient, LogisticGradient,
    MixedShard, MultiTaskGradient, PerTaskUpdater, SimpleUpdater,
    SmoothedHingeGradient, SquaredL2Updater, assign_folds, cross_validate,
    generate_dense_problem, ops, run,
)
from sparkagd_amd.config import AGDConfig
from sparkagd_amd.data import generate_csr_problem, shard_range
from sparkagd_amd.ops import reference

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GRADIENTS = [LogisticGradient, LeastSquaresGradient, HingeGradient,
             SmoothedHingeGradient]
LAMBDAS = (0.01, 0.1, 1.0)
N_FOLDS = 3


def _problem(loss_type=ops.LOSS_LOGISTIC, sample_weight=False):
    shard, _ = generate_dense_problem(n=240, d=12, seed=0, loss_type=loss_type,
                                      dtype=torch.float64)
    if sample_weight:
        g = torch.Generator().manual_seed(3)
        shard = DenseShard(shard.features, shard.labels,
                           0.5 + torch.rand(shard.n, generator=g))
    return shard


def _tasks():
    """{0.01, 0.1, 1.0} x 3 folds plus one task that trains on every row."""
    holdout = [f for _ in LAMBDAS for f in range(N_FOLDS)] + [-1]
    lams = [lam for lam in LAMBDAS for _ in range(N_FOLDS)] + [0.1]
    return holdout, lams


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def _check_eval_parity(shard, dense_features, grad_cls, mask):
    folds = assign_folds(shard.n, N_FOLDS, seed=1)
    holdout, _ = _tasks()
    r = len(holdout)
    sw = shard.sample_weight
    mt = MultiTaskGradient(grad_cls(), r, folds, holdout, sample_weight=sw)
    g = torch.Generator().manual_seed(5)
    w = 0.3 * torch.randn(shard.d * r, generator=g, dtype=torch.float64)
    grad, lc = mt.eval(shard, w, mask)
    grad = grad.reshape(shard.d, r)
    wts = sw.to(torch.float64) if sw is not None else torch.ones(shard.n, dtype=torch.float64)
    n_total = float(wts.sum())
    expect_loss = 0.0
    for t, h in enumerate(holdout):
        rows = folds != h
        n_r = float(wts[rows].sum())
        sub_mask = None if mask is None else mask[rows]
        g_ref, lc_ref = reference.dense_eval(
            dense_features[rows], shard.labels[rows],
            w.reshape(shard.d, r)[:, t].contiguous(), grad_cls.LOSS_TYPE,
            sub_mask, True, None if sw is None else sw[rows])
        scale = n_total / n_r
        assert _rel(grad[:, t], scale * g_ref) <= 1e-12, (grad_cls.__name__, t)
        assert abs(float(mt.last_task_loss[t]) - float(lc_ref[0])) \
            <= 1e-12 * abs(float(lc_ref[0]))
        expect_loss += scale * float(lc_ref[0])
    assert abs(float(lc[0]) - expect_loss) <= 1e-12 * abs(expect_loss)
    count = float((wts * mask.to(torch.float64)).sum()) if mask is not None else n_total
    assert abs(float(lc[1]) - count) <= 1e-12 * count


@pytest.mark.parametrize("grad_cls", GRADIENTS)
@pytest.mark.parametrize("masked_weighted", [False, True])
def test_eval_matches_single_task_dense(grad_cls, masked_weighted):
    shard = _problem(grad_cls.LOSS_TYPE, sample_weight=masked_weighted)
    mask = None
    if masked_weighted:
        g = torch.Generator().manual_seed(9)
        mask = (torch.rand(shard.n, generator=g) < 0.7).to(torch.uint8)
    _check_eval_parity(shard, shard.features, grad_cls, mask)


@pytest.mark.parametrize("grad_cls", GRADIENTS)
def test_eval_matches_single_task_csr(grad_cls):
    src, _ = generate_csr_problem(n=200, d=40, nnz_per_row=5, seed=2,
                                  loss_type=grad_cls.LOSS_TYPE)
    g = torch.Generator().manual_seed(4)
    shard = CSRShard(src.rowptr, src.col, src.val.to(torch.float64),
                     src.labels, src.d,
                     sample_weight=0.5 + torch.rand(src.n, generator=g))
    dense = torch.sparse_csr_tensor(
        shard.rowptr.to(torch.int64), shard.col.to(torch.int64), shard.val,
        size=(shard.n, shard.d)).to_dense()
    mask = (torch.rand(shard.n, generator=g) < 0.8).to(torch.uint8)
    _check_eval_parity(shard, dense, grad_cls, mask)


@pytest.mark.parametrize("grad_cls", [LogisticGradient, SmoothedHingeGradient,
                                      LeastSquaresGradient])
def test_separable_trajectory(grad_cls):
    """With backtracking off (beta = alpha = 1, no restart) θ and L are
    data-independent, so each column of the batched run is the single-task
    run() on that fold's rows with that lambda."""
    shard = _problem(grad_cls.LOSS_TYPE)
    folds = assign_folds(shard.n, N_FOLDS, seed=1)
    holdout, lams = _tasks()
    r = len(holdout)
    L0 = 2.0 * float(shard.features.norm() ** 2) / 140 + 1.0
    args = (L0, math.inf, 1.0, 1.0, False)
    mt = MultiTaskGradient(grad_cls(), r, folds, holdout)
    w, hist = run(shard, mt, PerTaskUpdater(SquaredL2Updater(), lams), 0.0, 25,
                  1.0, torch.zeros(shard.d * r, dtype=torch.float64), *args)
    assert len(hist) == 25
    w = w.reshape(shard.d, r)
    worst = 0.0
    for t, (h, lam) in enumerate(zip(holdout, lams)):
        rows = folds != h
        sub = DenseShard(shard.features[rows], shard.labels[rows])
        w_t, hist_t = run(sub, grad_cls(), SquaredL2Updater(), 0.0, 25, lam,
                          torch.zeros(shard.d, dtype=torch.float64), *args)
        assert len(hist_t) == 25
        worst = max(worst, _rel(w[:, t], w_t))
    print(f"{grad_cls.__name__}: worst column relative error {worst:.3g}")
    assert worst <= 1e-12


@pytest.mark.parametrize("updater", [SimpleUpdater(), L1Updater(),
                                     SquaredL2Updater(),
                                     ElasticNetUpdater(0.3)],
                         ids=["simple", "l1", "l2", "elastic"])
def test_per_task_updater_is_base_per_column(updater):
    d, r = 37, 5
    g = torch.Generator().manual_seed(11)
    w = torch.randn(d * r, generator=g, dtype=torch.float64)
    gr = torch.randn(d * r, generator=g, dtype=torch.float64)
    lams = [0.0, 0.05, 0.3, 1.0, 2.5]
    up = PerTaskUpdater(updater, lams)
    assert up.AFFINE_PROX is False
    out, reg = up.compute(w, gr, 0.37, 1, 0.8)
    reg_sum = 0.0
    for t, lam in enumerate(lams):
        o_t, r_t = updater.compute(w.reshape(d, r)[:, t].contiguous(),
                                   gr.reshape(d, r)[:, t].contiguous(),
                                   0.37, 1, 0.8 * lam)
        torch.testing.assert_close(out.reshape(d, r)[:, t], o_t,
                                   rtol=1e-12, atol=1e-14)
        reg_sum += float(r_t)
    assert abs(float(reg) - reg_sum) <= 1e-12 * max(reg_sum, 1e-300)
    assert abs(float(up.reg_value(out, 0.8)) - reg_sum) <= 1e-12 * max(reg_sum, 1e-300)


def test_single_task_equals_base_run():
    shard = _problem()
    w0 = torch.zeros(shard.d, dtype=torch.float64)
    w_b, h_b = run(shard, LogisticGradient(), SquaredL2Updater(), 1e-9, 30,
                   0.05, w0)
    w_m, h_m = run(shard, MultiTaskGradient(LogisticGradient(), 1),
                   SquaredL2Updater(), 1e-9, 30, 0.05, w0)
    assert len(h_b) == len(h_m)
    assert _rel(w_m, w_b) <= 1e-12
    torch.testing.assert_close(torch.tensor(h_m), torch.tensor(h_b),
                               rtol=1e-12, atol=0.0)


def _torch_mean_loss(features, labels, w, loss_type, weights=None):
    _, loss = reference._multiplier_and_loss(
        features.to(torch.float64) @ w.to(torch.float64), labels, loss_type)
    if weights is None:
        return float(loss.mean())
    wt = weights.to(torch.float64)
    return float((loss * wt).sum() / wt.sum())


def _cv_config():
    # a Lipschitz bound of the logistic smooth part plus the largest lambda:
    # the L2 step is explicit, so L must cover it
    return AGDConfig(L0=50.0)


def test_cross_validate_scores_and_model():
    shard = _problem(sample_weight=True)
    lams = [1e-3, 1e-2, 0.3]
    res = cross_validate(shard, lams, n_folds=3, num_iterations=40, seed=2,
                         config=_cv_config())
    assert isinstance(res, CVResult)
    folds = assign_folds(shard.n, 3, seed=2)
    assert res.heldout_loss.shape == (3, 3)
    assert res.fold_weights.shape == (3, 3, shard.d)
    for li in range(3):
        for f in range(3):
            rows = folds == f
            want = _torch_mean_loss(shard.features[rows], shard.labels[rows],
                                    res.fold_weights[li, f], ops.LOSS_LOGISTIC,
                                    shard.sample_weight[rows])
            assert abs(float(res.heldout_loss[li, f]) - want) <= 1e-12 * want
    torch.testing.assert_close(res.mean_loss, res.heldout_loss.mean(dim=1))
    assert res.best_lambda == lams[int(res.mean_loss.argmin())]
    assert res.model.link == "logistic"
    assert res.model.weights.shape == (shard.d,)
    assert len(res.loss_history) > 0
    # the three lambdas differ, so the held-out scores must as well
    assert float(res.heldout_loss.std()) > 0


def test_cross_validate_equal_lambdas_is_tracked_and_ties_go_up():
    shard = _problem()
    res = cross_validate(shard, [0.01, 0.01], n_folds=2, num_iterations=10,
                         config=_cv_config(), refit=False)
    assert res.model is None
    torch.testing.assert_close(res.heldout_loss[0], res.heldout_loss[1],
                               rtol=1e-12, atol=0.0)
    assert res.best_lambda == 0.01


def test_cross_validate_error_cases():
    shard = _problem()
    with pytest.raises(ValueError, match="no training rows"):
        cross_validate(shard, [0.1], n_folds=1, num_iterations=2)
    with pytest.raises(ValueError, match="dense and CSR"):
        cross_validate(InterceptShard(shard), [0.1], n_folds=2)
    with pytest.raises(ValueError, match="dense and CSR"):
        cross_validate(MixedShard([shard, shard]), [0.1], n_folds=2)
    with pytest.raises(ValueError, match="direct solver"):
        cross_validate(shard, [0.1], n_folds=2, config=AGDConfig(solver="gram"))


def test_multitask_gradient_error_cases():
    shard = _problem()
    folds = assign_folds(shard.n, 2, seed=0)
    mt = MultiTaskGradient(LogisticGradient(), 2, folds, [0, 1])
    w = torch.zeros(shard.d * 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="dense and CSR"):
        mt.eval(InterceptShard(shard), torch.zeros(shard.d * 2 + 1, dtype=torch.float64))
    with pytest.raises(ValueError, match="direct solver"):
        run(shard, mt, SquaredL2Updater(), 1e-6, 2, 0.1, w, solver="gram")
    with pytest.raises(ValueError, match="no training rows"):
        MultiTaskGradient(LogisticGradient(), 1, torch.zeros(5, dtype=torch.int32), [0])
    weighted = _problem(sample_weight=True)
    with pytest.raises(ValueError, match="sample_weight"):
        mt.eval(weighted, w)


# --- two ranks (gloo) ---

def _global_cv_problem():
    shard = _problem(sample_weight=True)
    return shard, assign_folds(shard.n, 3, seed=4)


def _dist_cv(rank, world):
    from sparkagd_amd import Communicator

    full, folds = _global_cv_problem()
    lo, hi = shard_range(full.n, rank, world)
    part = DenseShard(full.features[lo:hi], full.labels[lo:hi],
                      full.sample_weight[lo:hi])
    res = cross_validate(part, [1e-3, 0.2], n_folds=3, num_iterations=15,
                         comm=Communicator(), config=_cv_config(),
                         fold_id=folds[lo:hi])
    return (res.heldout_loss.tolist(), res.fold_weights.tolist(),
            res.model.weights.tolist(), res.best_lambda)


def test_two_rank_cross_validate_matches_one_rank():
    import test_distributed as td

    try:
        results = td._run_dist(_dist_cv, world=2)
    finally:
        td.teardown_module(None)
    full, folds = _global_cv_problem()
    ref = cross_validate(full, [1e-3, 0.2], n_folds=3, num_iterations=15,
                         config=_cv_config(), fold_id=folds)
    for rank in (0, 1):
        held, fw, mw, best = results[rank]
        torch.testing.assert_close(torch.tensor(held, dtype=torch.float64),
                                   ref.heldout_loss, rtol=1e-10, atol=0.0)
        assert _rel(torch.tensor(fw, dtype=torch.float64), ref.fold_weights) <= 1e-10
        assert _rel(torch.tensor(mw, dtype=torch.float64), ref.model.weights) <= 1e-10
        assert best == ref.best_lambda
    assert results[0][1] == results[1][1]  # replicated update


def test_cross_validate_example_runs():
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "examples", "cross_validate.py"),
         "--n", "600", "--d", "16", "--iters", "15"],
        capture_output=True, text=True, timeout=300, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "best lambda" in out.stdout
    assert out.stdout.count("lambda=") >= 3
