"""k_at_margin_update_tasks against the f64 oracle and the scalar kernel, and
tracked mixed-lambda GPU runs against the CPU f64 run and the untracked GPU
run."""

import math

import pytest
import torch

from sparkagd_amd import (
    CSRShard, DenseShard, LogisticGradient, MultiTaskGradient, PerTaskUpdater,
    SquaredL2Updater, assign_folds, generate_dense_problem, ops, run,
)
from sparkagd_amd.data import generate_csr_problem
from sparkagd_amd.ops import multitask as mt
from sparkagd_amd.ops.multiclass import padded_k

from test_gpu_multitask import N_FOLDS, _batched_run, _tasks
from test_multitask_tracked import (
    STREAM_HOLDOUT, STREAM_LAMBDAS, _Record, count_streams,
)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STEP, THETA = 0.37, 0.61

# the shapes of test_multiplier_tasks_matches_oracle (every padded_k template,
# the ceil-4 regime, KC above 256, more than one grid-stride trip), plus one
# whose second trip lands on ANOTHER column (KC = 36 does not divide the grid
# stride), the only case where the carried column index moves
SHAPES = ([(n, r) for n in (1, 257, 1000)
           for r in (1, 3, 4, 5, 8, 13, 16, 17, 32, 33, 40)]
          + [(5000, 300), (300_000, 16), (240_000, 33)])


def _inputs(n, r, dtype, pad_fill):
    g = torch.Generator().manual_seed(100 * n + r)
    kc = padded_k(r)
    out = []
    for _ in range(3):
        t = torch.randn(n, kc, generator=g, dtype=dtype)
        t[:, r:] = pad_fill
        out.append(t.reshape(-1))
    lam = torch.rand(r, generator=g, dtype=torch.float64)
    return out, lam


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("n,r", SHAPES)
def test_at_margin_update_tasks_matches_oracle(n, r, dtype):
    kc = padded_k(r)
    tol = 1e-6 if dtype == torch.float32 else 1e-12
    zeros = torch.zeros(n, kc - r, dtype=dtype)
    ref = None
    for pad_fill in (7.0, float("nan")):
        (zm, xm, gm), lam = _inputs(n, r, dtype, pad_fill)
        if ref is None:  # the oracle never reads the pads: one reference
            ref = mt.ref_at_margin_update_tasks(
                zm.double(), xm.double(), gm.double(), STEP, lam, THETA, r)
        dev = [t.to(DEV) for t in (zm, xm, gm)]
        lam_d = lam.to(DEV)
        zn, xn = mt.at_margin_update_tasks(*dev, STEP, lam_d, THETA, r)
        assert zn.dtype == dtype and xn.dtype == dtype
        for got, want in ((zn, ref[0]), (xn, ref[1])):
            got2 = got.cpu().reshape(n, kc)
            torch.testing.assert_close(got2[:, :r].double(),
                                       want.reshape(n, kc)[:, :r],
                                       rtol=tol, atol=tol)
            assert torch.equal(got2[:, r:], zeros), (n, r, pad_fill)
        zb, xb = mt.at_margin_update_tasks(*dev, STEP, lam_d, THETA, r)
        # NaN != NaN, but the outputs hold none: bitwise run-to-run equality
        assert torch.equal(zn, zb) and torch.equal(xn, xb)


# 1 - 0.37*0.967 is 0x1.48cfbfc6540ccp-1 with the product and the difference
# rounded separately (what the host computes) and 0x1.48cfbfc6540cdp-1 fused
FMA_STEP, FMA_LAMBDA = 0.37, 0.967


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64],
                         ids=["f32", "f64"])
@pytest.mark.parametrize("n,r", [(1000, 16), (777, 36), (240_000, 36)])
def test_equal_lambda_is_bitwise_the_scalar_kernel(n, r, dtype):
    assert (1.0 - FMA_STEP * FMA_LAMBDA).hex() == "0x1.48cfbfc6540ccp-1"
    assert padded_k(r) == r  # no pads
    (zm, xm, gm), _ = _inputs(n, r, dtype, 0.0)
    dev = [t.to(DEV) for t in (zm, xm, gm)]
    lam = torch.full((r,), FMA_LAMBDA, dtype=torch.float64, device=DEV)
    zn, xn = mt.at_margin_update_tasks(*dev, FMA_STEP, lam, THETA, r)
    zs, xs = ops.at_margin_update(*dev, 1.0 - FMA_STEP * FMA_LAMBDA,
                                  -FMA_STEP, THETA)
    assert torch.equal(zn, zs)
    assert torch.equal(xn, xs)


def test_stream_count_on_device():
    T = 12
    src, _ = generate_dense_problem(n=2048, d=256, seed=0)
    shard = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    folds = assign_folds(shard.n, 2, seed=1)
    args = (shard, PerTaskUpdater(SquaredL2Updater(), STREAM_LAMBDAS), 4,
            folds, STREAM_HOLDOUT, T, torch.float32)
    n_margins, n_grad, hist = count_streams(*args)
    assert len(hist) == T
    assert n_margins == 1 + T
    assert n_grad == T
    n_margins_u, _, _ = count_streams(*args, track_margins=False)
    assert n_margins_u == 3 * T


# --- end to end: the _batched_run configuration, tracked by default ---

def _dense_pair(dtype):
    src, _ = generate_dense_problem(n=2048, d=256, seed=0, dtype=dtype)
    frob = float(src.features.double().norm() ** 2)
    cpu = DenseShard(src.features.double(), src.labels)
    gpu = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    return cpu, gpu, frob


def _tracked_vs_cpu(cpu, gpu, frob, track_margins="auto"):
    folds = assign_folds(cpu.n, N_FOLDS, seed=1)
    wc, hc = _batched_run(cpu, folds, frob, torch.float64)
    holdout, lams = _tasks()
    r = len(holdout)
    # the same run as _batched_run's, counted: it must be the tracked one
    L0 = 2.0 * frob / (gpu.n * 140.0 / 240.0) + 1.0
    grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
    calls = {"margins": 0}
    margins = grad.margins

    def counted(*a, **kw):
        calls["margins"] += 1
        return margins(*a, **kw)

    grad.margins = counted
    wg, hg = run(gpu, grad, PerTaskUpdater(SquaredL2Updater(), lams), 0.0, 25,
                 1.0, torch.zeros(gpu.d * r, dtype=torch.float32, device=DEV),
                 L0, math.inf, 1.0, 1.0, False, track_margins=track_margins)
    assert calls["margins"] == 1 + 25
    assert len(hc) == len(hg) == 25
    return wc, hc, wg, hg


def test_tracked_run_f32_dense_matches_cpu():
    wc, hc, wg, hg = _tracked_vs_cpu(*_dense_pair(torch.float32))
    print(f"last loss cpu {hc[-1]:.10f} gpu {hg[-1]:.10f}")
    assert abs(hc[-1] - hg[-1]) <= 1e-3 * abs(hc[-1])
    torch.testing.assert_close(wg.double().cpu(), wc, rtol=5e-3, atol=5e-3)


def test_tracked_run_csr_matches_cpu():
    src, _ = generate_csr_problem(n=2048, d=256, nnz_per_row=8, seed=0)
    frob = float(src.val.double().norm() ** 2)
    cpu = CSRShard(src.rowptr, src.col, src.val.double(), src.labels, src.d)
    gpu = CSRShard(src.rowptr.to(DEV), src.col.to(DEV), src.val.to(DEV),
                   src.labels.to(DEV), src.d)
    wc, hc, wg, hg = _tracked_vs_cpu(cpu, gpu, frob)
    print(f"last loss cpu {hc[-1]:.10f} gpu {hg[-1]:.10f}")
    assert abs(hc[-1] - hg[-1]) <= 1e-3 * abs(hc[-1])
    torch.testing.assert_close(wg.double().cpu(), wc, rtol=5e-3, atol=5e-3)


def test_tracked_run_bf16_matches_cpu():
    # a bf16 GPU shard tracks a mixed sweep only when asked to
    wc, hc, wg, hg = _tracked_vs_cpu(*_dense_pair(torch.bfloat16),
                                     track_margins=True)
    worst = max(abs(a - b) / max(1.0, abs(a)) for a, b in zip(hc, hg))
    num = float(torch.norm(wg.double().cpu() - wc))
    den = float(torch.norm(wc)) + 1e-30
    print(f"worst loss gap {worst:.3g}, weights relative norm {num / den:.3g}")
    for i, (a, b) in enumerate(zip(hc, hg)):
        assert abs(a - b) < 2e-3 * max(1.0, abs(a)), (i, a, b)
    assert num / den < 1e-2, (num, den)


# --- a restart on the tracked path ---

RESTART_ITERS = 30
# the L2 step is explicit, so the lambdas stay well under the default L0 = 1
# that the backtracking starts from (at lambda = 0.1 this run diverges with
# the plain updater too); with these the shared gradient test first restarts
# the run a few iterations before the end
RESTART_LAMBDAS = (5e-3, 1e-2, 2e-2)


def restart_task_lambdas():
    return [lam for lam in RESTART_LAMBDAS for _ in range(N_FOLDS)] + [1e-2]


def restart_run(shard, folds, updater, reg_param, track):
    """Default backtracking (L0 = 1, beta = 0.5, alpha = 0.9) with
    may_restart=True on the ten (fold, all-rows) tasks of ``_tasks()``;
    returns (weights, history, iterations that restarted)."""
    holdout, _ = _tasks()
    r = len(holdout)
    rec = _Record()
    grad = MultiTaskGradient(LogisticGradient(), r, folds, holdout)
    w, hist = run(shard, grad, updater, 0.0, RESTART_ITERS, reg_param,
                  torch.zeros(shard.d * r, dtype=torch.float32, device=DEV),
                  1.0, math.inf, 0.5, 0.9, True, metrics=rec,
                  track_margins="auto" if track else False)
    return w, hist, [row["iter"] for row in rec.rows if row["restarted"]]


def run_gap(a, b):
    """(weights relative norm, worst relative loss-history gap) of two runs."""
    (wa, ha, _), (wb, hb, _) = a, b
    assert len(ha) == len(hb)
    wgap = float((wa.double() - wb.double()).norm() / wb.double().norm())
    hgap = max(abs(x - y) / abs(y) for x, y in zip(ha, hb))
    return wgap, hgap


# The tolerance is the parent's own behaviour, not the new path's: the gap
# between the EXISTING equal-lambda tracked and untracked f32 runs (plain
# SquaredL2Updater) of this configuration on this shard, measured on an
# MI355X at each lambda of RESTART_LAMBDAS (runs are bitwise repeatable):
#   lambda   weights rel. norm   worst rel. loss gap
#   0.005    2.786e-05           4.108e-08
#   0.01     1.909e-05           3.512e-08
#   0.02     5.274e-05           1.361e-07
# The worst of the three, times 4 for the extra columns. The mixed run
# measured 2.600e-05 and 2.174e-07 and restarted first at iteration 23,
# tracked and untracked alike.
EQUAL_LAMBDA_W_SPREAD = 5.274e-05
EQUAL_LAMBDA_LOSS_SPREAD = 1.361e-07


def test_restart_on_the_tracked_path_matches_untracked():
    src, _ = generate_dense_problem(n=2048, d=256, seed=0)
    shard = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    folds = assign_folds(shard.n, N_FOLDS, seed=1)
    lams = restart_task_lambdas()
    tracked = restart_run(shard, folds, PerTaskUpdater(SquaredL2Updater(), lams),
                          1.0, True)
    untracked = restart_run(shard, folds,
                            PerTaskUpdater(SquaredL2Updater(), lams), 1.0, False)
    assert len(tracked[1]) == RESTART_ITERS
    assert tracked[2], "no restart on the tracked path"
    assert tracked[2][0] < RESTART_ITERS  # iterations ran after a restart
    wgap, hgap = run_gap(tracked, untracked)
    print(f"restarts {tracked[2]}; weights gap {wgap:.3e}, loss gap {hgap:.3e}")
    assert wgap <= 4.0 * EQUAL_LAMBDA_W_SPREAD
    assert hgap <= 4.0 * EQUAL_LAMBDA_LOSS_SPREAD


def test_bf16_shard_tracks_a_mixed_sweep_only_on_request():
    """The margins GEMM of a bf16 shard rounds the weights: "auto" keeps a
    mixed sweep untracked there, track_margins=True tracks it."""
    T = 4
    src, _ = generate_dense_problem(n=2048, d=256, seed=0, dtype=torch.bfloat16)
    shard = DenseShard(src.features.to(DEV), src.labels.to(DEV))
    folds = assign_folds(shard.n, 2, seed=1)
    args = (shard, PerTaskUpdater(SquaredL2Updater(), STREAM_LAMBDAS), 4,
            folds, STREAM_HOLDOUT, T, torch.float32)
    assert count_streams(*args)[0] > 1 + T
    assert count_streams(*args, track_margins=True)[0] == 1 + T
