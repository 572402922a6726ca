"""Margin tracking of a mixed-lambda multi-task run (PerTaskUpdater over an
affine base: one shrink per column of the [n, KC] margins) — CPU tier, f64.

The tracked run must stream the shard twice per iteration (one margins pass
over g_y, one Aᵀ·m pass) and compute what the untracked run computes."""

import math

import pytest
import torch

from sparkagd_amd import (
    CSRShard, DenseShard, ElasticNetUpdater, L1Updater, LogisticGradient,
    MultiTaskGradient, PerTaskUpdater, SimpleUpdater, SquaredL2Updater,
    assign_folds, cross_validate, generate_dense_problem, run,
)
from sparkagd_amd.config import AGDConfig
from sparkagd_amd.data import generate_csr_problem
from sparkagd_amd.ops import multitask as mt
from sparkagd_amd.ops.multiclass import padded_k

LAMBDAS = (0.01, 0.1, 1.0)
N_FOLDS = 3


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


class _Record:
    def __init__(self):
        self.rows = []

    def log(self, **kw):
        self.rows.append(kw)


# --- 1. the oracle and its pad-column contract ---

@pytest.mark.parametrize("r", [1, 5, 33])
def test_oracle_is_the_column_formula_and_zeroes_the_pads(r):
    n, kc = 19, padded_k(r)
    g = torch.Generator().manual_seed(r)
    zm, xm, gm = (torch.randn(n, kc, generator=g, dtype=torch.float64)
                  for _ in range(3))
    for t in (zm, xm, gm):
        t[:, r:] = float("nan")
    lam = torch.rand(r, generator=g, dtype=torch.float64)
    step, theta = 0.37, 0.61
    zn, xn = mt.ref_at_margin_update_tasks(
        zm.reshape(-1), xm.reshape(-1), gm.reshape(-1), step, lam, theta, r)
    zn, xn = zn.reshape(n, kc), xn.reshape(n, kc)
    for c in range(r):
        want_z = (1.0 - step * float(lam[c])) * zm[:, c] - step * gm[:, c]
        want_x = (1.0 - theta) * xm[:, c] + theta * want_z
        torch.testing.assert_close(zn[:, c], want_z, rtol=1e-15, atol=1e-15)
        torch.testing.assert_close(xn[:, c], want_x, rtol=1e-15, atol=1e-15)
    assert torch.equal(zn[:, r:], torch.zeros(n, kc - r, dtype=torch.float64))
    assert torch.equal(xn[:, r:], torch.zeros(n, kc - r, dtype=torch.float64))
    # the dispatching op is the oracle on CPU
    zd, xd = mt.at_margin_update_tasks(
        zm.reshape(-1), xm.reshape(-1), gm.reshape(-1), step, lam, theta, r)
    assert torch.equal(zd.reshape(n, kc), zn) and torch.equal(xd.reshape(n, kc), xn)


# --- 2. stream count ---

def count_streams(shard, updater, num_tasks, folds, holdout, iters, wdtype,
                  **run_kw):
    """(margins calls, eval_from_margins(need_grad=True) calls, history) of a
    default-settings run() from zero weights."""
    grad = MultiTaskGradient(LogisticGradient(), num_tasks, folds, holdout)
    calls = {"margins": 0, "grad": 0}
    margins, efm = grad.margins, grad.eval_from_margins

    def counted_margins(*a, **kw):
        calls["margins"] += 1
        return margins(*a, **kw)

    def counted_efm(shard_, m, mask=None, need_grad=True):
        calls["grad"] += bool(need_grad)
        return efm(shard_, m, mask, need_grad)

    grad.margins, grad.eval_from_margins = counted_margins, counted_efm
    w0 = torch.zeros(shard.d * num_tasks, dtype=wdtype, device=shard.device)
    _w, hist = run(shard, grad, updater, 1e-300, iters, 1.0, w0, **run_kw)
    return calls["margins"], calls["grad"], hist


STREAM_LAMBDAS = [1e-4, 1e-2, 1e-4, 1e-2]
STREAM_HOLDOUT = [0, 0, 1, 1]


def test_mixed_lambda_run_streams_the_shard_twice_per_iteration():
    T = 12
    shard, _ = generate_dense_problem(n=240, d=20, seed=0, dtype=torch.float64)
    folds = assign_folds(shard.n, 2, seed=1)
    args = (shard, PerTaskUpdater(SquaredL2Updater(), STREAM_LAMBDAS), 4,
            folds, STREAM_HOLDOUT, T, torch.float64)
    n_margins, n_grad, hist = count_streams(*args)
    assert len(hist) == T
    assert n_margins == 1 + T
    assert n_grad == T
    # the untracked path: margins for y, the backtracking x and the
    # loss-history x of every iteration
    n_margins_u, _, hist_u = count_streams(*args, track_margins=False)
    assert len(hist_u) == T
    assert n_margins_u == 3 * T


def test_l1_base_is_not_tracked():
    T = 12
    shard, _ = generate_dense_problem(n=240, d=20, seed=0, dtype=torch.float64)
    folds = assign_folds(shard.n, 2, seed=1)
    n_margins, _, hist = count_streams(
        shard, PerTaskUpdater(L1Updater(), STREAM_LAMBDAS), 4, folds,
        STREAM_HOLDOUT, T, torch.float64)
    assert len(hist) == T
    assert n_margins > 1 + T


def test_task_count_mismatch_is_not_tracked():
    """An updater over fewer columns than the gradient has (weights still a
    whole number of blocks) must not take the per-column margin update."""
    shard, _ = generate_dense_problem(n=240, d=20, seed=0, dtype=torch.float64)
    folds = assign_folds(shard.n, 2, seed=1)
    n_margins, _, _ = count_streams(
        shard, PerTaskUpdater(SquaredL2Updater(), [1e-3, 1e-2]), 4, folds,
        STREAM_HOLDOUT, 4, torch.float64)
    assert n_margins > 1 + 4


# --- 3. tracked = untracked ---

def _tasks():
    """{0.01, 0.1, 1.0} x 3 folds plus one task that trains on every row."""
    holdout = [f for _ in LAMBDAS for f in range(N_FOLDS)] + [-1]
    lams = [lam for lam in LAMBDAS for _ in range(N_FOLDS)] + [0.1]
    return holdout, lams


def _shards():
    dense, _ = generate_dense_problem(n=240, d=12, seed=0, dtype=torch.float64)
    src, _ = generate_csr_problem(n=200, d=40, nnz_per_row=5, seed=2)
    csr = CSRShard(src.rowptr, src.col, src.val.to(torch.float64), src.labels,
                   src.d)
    frob = {"dense": float(dense.features.norm() ** 2),
            "csr": float(csr.val.norm() ** 2)}
    return {"dense": dense, "csr": csr}, frob


def _mixed_run(shard, args, base=None, metrics=None, **kw):
    holdout, lams = _tasks()
    r = len(holdout)
    folds = assign_folds(shard.n, N_FOLDS, seed=1)
    grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
    upd = PerTaskUpdater(base or SquaredL2Updater(), lams)
    return run(shard, grad, upd, 0.0, 25, 1.0,
               torch.zeros(shard.d * r, dtype=torch.float64), *args,
               metrics=metrics, **kw)


def _assert_same(run_a, run_b):
    (wa, ha), (wb, hb) = run_a, run_b
    assert len(ha) == len(hb) == 25
    assert _rel(wa, wb) <= 1e-12
    torch.testing.assert_close(torch.tensor(ha, dtype=torch.float64),
                               torch.tensor(hb, dtype=torch.float64),
                               rtol=1e-12, atol=0.0)


@pytest.mark.parametrize("kind", ["dense", "csr"])
@pytest.mark.parametrize("config", ["separable", "default"])
def test_tracked_equals_untracked(kind, config):
    shards, frob = _shards()
    shard = shards[kind]
    if config == "separable":
        # backtracking off: the configuration of test_separable_trajectory
        args = (2.0 * frob[kind] / 140 + 1.0, math.inf, 1.0, 1.0, False)
    else:
        args = (1.0, math.inf, 0.5, 0.9, True)
    rec = _Record()
    tracked = _mixed_run(shard, args, metrics=rec)
    untracked = _mixed_run(shard, args, track_margins=False)
    _assert_same(tracked, untracked)
    if config == "default":
        # the restart branch (zm = xm.clone()) ran on the tracked path
        assert any(row["restarted"] for row in rec.rows)
    refreshed = _mixed_run(shard, args, margin_refresh_every=5)
    _assert_same(refreshed, tracked)


def test_simple_base_is_tracked_with_zero_shrink():
    """A SimpleUpdater base ignores its lambdas: the margin update must too."""
    shards, _ = _shards()
    args = (1.0, math.inf, 0.5, 0.9, True)
    tracked = _mixed_run(shards["dense"], args, base=SimpleUpdater())
    untracked = _mixed_run(shards["dense"], args, base=SimpleUpdater(),
                           track_margins=False)
    _assert_same(tracked, untracked)


def test_resume_recomputes_the_tracked_margins(tmp_path):
    shards, _ = _shards()
    shard = shards["dense"]
    holdout, lams = _tasks()
    r = len(holdout)
    folds = assign_folds(shard.n, N_FOLDS, seed=1)
    w0 = torch.zeros(shard.d * r, dtype=torch.float64)

    def go(iters, **kw):
        grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
        return run(shard, grad, PerTaskUpdater(SquaredL2Updater(), lams), 0.0,
                   iters, 1.0, w0, **kw)

    ckpt = str(tmp_path / "mixed.ckpt")
    go(6, checkpoint_path=ckpt, checkpoint_every=6)
    w_resumed, h_resumed = go(12, resume_from=ckpt)
    w_straight, h_straight = go(12)
    assert len(h_resumed) == len(h_straight) == 12
    assert _rel(w_resumed, w_straight) <= 1e-12
    torch.testing.assert_close(torch.tensor(h_resumed, dtype=torch.float64),
                               torch.tensor(h_straight, dtype=torch.float64),
                               rtol=1e-12, atol=0.0)


# --- 4. cross_validate ---

def test_cross_validate_mixed_sweep_tracked_selects_the_same_lambda():
    shard, _ = generate_dense_problem(n=240, d=12, seed=0, dtype=torch.float64)
    lams = [1e-3, 1e-2, 0.3]
    kw = dict(n_folds=3, num_iterations=40, seed=2, refit=False)
    tracked = cross_validate(shard, lams, config=AGDConfig(L0=50.0), **kw)
    untracked = cross_validate(
        shard, lams, config=AGDConfig(L0=50.0, track_margins=False), **kw)
    assert tracked.best_lambda == untracked.best_lambda
    torch.testing.assert_close(tracked.heldout_loss, untracked.heldout_loss,
                               rtol=1e-10, atol=0.0)
    assert float(tracked.heldout_loss.std()) > 0


# --- 5. attributes ---

def test_column_affine_attribute():
    lams = [0.1, 0.2]
    for base in (SquaredL2Updater(), SimpleUpdater()):
        up = PerTaskUpdater(base, lams)
        assert up.COLUMN_AFFINE_PROX is True
        assert up.AFFINE_PROX is False
    for base in (ElasticNetUpdater(0.3), L1Updater()):
        up = PerTaskUpdater(base, lams)
        assert up.COLUMN_AFFINE_PROX is False
        assert up.AFFINE_PROX is False
        with pytest.raises(NotImplementedError):
            z = torch.zeros(4, dtype=torch.float64)
            up.prox_margins_tasks(z, z, z, 0.1, 1.0, 0.5)


def test_rounding_margins_pass_tracks_only_on_request(monkeypatch):
    """Where the margins pass rounds its weights (a bf16 GPU shard; forced
    here), "auto" leaves a mixed sweep untracked and True tracks it."""
    T = 4
    shard, _ = generate_dense_problem(n=240, d=20, seed=0, dtype=torch.float64)
    folds = assign_folds(shard.n, 2, seed=1)
    args = (shard, PerTaskUpdater(SquaredL2Updater(), STREAM_LAMBDAS), 4,
            folds, STREAM_HOLDOUT, T, torch.float64)
    assert MultiTaskGradient(LogisticGradient(), 1).rounds_margin_weights(shard) is False
    monkeypatch.setattr(MultiTaskGradient, "rounds_margin_weights",
                        lambda self, shard: True)
    assert count_streams(*args)[0] == 3 * T
    assert count_streams(*args, track_margins=True)[0] == 1 + T
