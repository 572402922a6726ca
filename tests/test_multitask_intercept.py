"""Per-task intercepts on the CPU tier (f64): a stacked run with
``intercept=True`` on A against the same run on the ones-appended shard
[A, 1] with the same free-row updater. The two differ only in the bias
plumbing, so they agree to rounding."""

import pytest
import torch

from sparkagd_amd import (
    AGDConfig, CSRShard, DenseShard, LogisticGradient, MultiTaskGradient,
    OneVsRestWithAGD, PerTaskUpdater, SquaredL2Updater, assign_folds,
    cross_validate, run,
)

N, D, K, ITERS = 240, 7, 3, 20


def _shards(kind):
    """(shard on A, shard on [A, 1]) with unbalanced class labels."""
    g = torch.Generator().manual_seed(5)
    A = torch.randn(N, D, generator=g, dtype=torch.float64)
    A[torch.rand(N, D, generator=g) < 0.5] = 0.0
    u = torch.rand(N, generator=g)
    y = (u > 0.7).float() + (u > 0.9).float()  # 70 / 20 / 10 %
    A1 = torch.cat([A, torch.ones(N, 1, dtype=torch.float64)], dim=1)
    if kind == "dense":
        return DenseShard(A, y), DenseShard(A1, y)
    out = []
    for m in (A, A1):
        s = m.to_sparse_csr()
        out.append(CSRShard(s.crow_indices().to(torch.int32),
                            s.col_indices().to(torch.int32), s.values(), y,
                            m.shape[1]))
    return tuple(out)


def _appended_run(shard1, grad, lams, cfg):
    r = len(lams)
    return run(shard1, grad, PerTaskUpdater(SquaredL2Updater(), lams, free_rows=1),
               0.0, ITERS, 1.0, torch.zeros(shard1.d * r, dtype=torch.float64),
               cfg.L0, cfg.Lexact, cfg.beta, cfg.alpha, cfg.may_restart,
               loss_history_mode=cfg.loss_history_mode,
               track_margins=cfg.track_margins)


def _close(a, b):
    torch.testing.assert_close(torch.as_tensor(a, dtype=torch.float64),
                               torch.as_tensor(b, dtype=torch.float64),
                               rtol=1e-10, atol=1e-10)


@pytest.mark.parametrize("track", ["auto", False])
@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_one_vs_rest_intercept_is_the_ones_appended_run(kind, track):
    shard, shard1 = _shards(kind)
    cfg = AGDConfig(track_margins=track)
    model = OneVsRestWithAGD.train(shard, K, num_iterations=ITERS, reg_param=0.05,
                                   convergence_tol=0.0, intercept=True, config=cfg)
    grad = MultiTaskGradient(LogisticGradient(), K, target_class=range(K))
    w, hist = _appended_run(shard1, grad, [0.05] * K, cfg)
    _close(model.loss_history, hist)
    _close(torch.cat([model.weights.reshape(-1), model.intercepts]), w)
    assert bool((model.intercepts != 0).all())
    z = shard1.features @ w.reshape(D + 1, K) if kind == "dense" else None
    if z is not None:  # score() carries the intercepts
        _close(model.score(shard), z)


@pytest.mark.parametrize("track", ["auto", False])
@pytest.mark.parametrize("kind", ["dense", "csr"])
def test_cv_sweep_intercept_is_the_ones_appended_run(kind, track):
    shard, shard1 = _shards(kind)
    shard.labels = shard1.labels = (shard.labels > 0).float()
    lams, n_f = [0.01, 0.1], 2
    folds = assign_folds(N, n_f, seed=1)
    cfg = AGDConfig(track_margins=track)
    res = cross_validate(shard, lams, n_folds=n_f, num_iterations=ITERS,
                         convergence_tol=0.0, fold_id=folds, config=cfg,
                         intercept=True)
    holdout = [f for _ in lams for f in range(n_f)]
    task_lams = [lam for lam in lams for _ in range(n_f)]
    grad = MultiTaskGradient(LogisticGradient(), 4, folds, holdout)
    w, hist = _appended_run(shard1, grad, task_lams, cfg)
    _close(res.loss_history, hist)
    W = w.reshape(D + 1, 4)
    _close(res.fold_weights, W[:D].T.reshape(2, n_f, D))
    _close(res.fold_intercepts, W[D].reshape(2, n_f))
    # held-out scoring saw the biased margins: the appended run's own score
    num, _ = grad.task_losses(shard1, grad.margins(shard1, w), invert=True)
    per_fold = torch.bincount(folds.long(), minlength=n_f).double()
    _close(res.heldout_loss, num.reshape(2, n_f) / per_fold)
    assert res.model.intercept != 0.0


def test_default_path_is_unchanged():
    shard, _ = _shards("dense")
    a = OneVsRestWithAGD.train(shard, K, num_iterations=8, reg_param=0.05)
    b = OneVsRestWithAGD.train(shard, K, num_iterations=8, reg_param=0.05,
                               intercept=False)
    assert a.loss_history == b.loss_history
    assert torch.equal(a.weights, b.weights)
    assert torch.equal(b.intercepts, torch.zeros(K, dtype=torch.float64))
