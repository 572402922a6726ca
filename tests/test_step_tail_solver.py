"""run() with one host round trip per trial (fused step tail + deferred
fetch) against the kernel-by-kernel sequence (SPARKAGD_STEP_TAIL=0): same
weights, same loss history, bit for bit, on a trajectory that backtracks and
restarts. GPU tier: bf16 shard, the native kernels. CPU tier: the same
bf16-valued data in float64 through the reference ops."""

import math

import pytest
import torch

from sparkagd_amd import (
    LogisticGradient, SimpleUpdater, SquaredL2Updater, run,
)
from sparkagd_amd.data import DenseShard

TIERS = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]
SHAPES = [(256, 512), (255, 520)]
# chosen on the CPU reference trajectory (see test_trajectory_has_both_branches):
# both shapes backtrack and restart within ITERS iterations from this seed
# and L0
SEED = 3
ITERS = 40
REG = 1e-3
L0 = 0.02  # far below the Lipschitz constant: the first iterations backtrack


class _Records:
    def __init__(self):
        self.rows = []

    def log(self, **kw):
        self.rows.append(kw)


def _shard(n, d, tier, sample_weight=None):
    g = torch.Generator().manual_seed(SEED)
    a = torch.randn(n, d, generator=g).to(torch.bfloat16)
    w_true = torch.randn(d, generator=g) / math.sqrt(d)
    noise = torch.randn(n, generator=g)
    labels = ((a.float() @ w_true + 0.5 * noise) > 0).float()
    if tier == "cuda":
        return (DenseShard(a.cuda(), labels.cuda(), sample_weight),
                torch.zeros(d, device="cuda", dtype=torch.float32))
    return (DenseShard(a.double(), labels.double(), sample_weight),
            torch.zeros(d, dtype=torch.float64))


def _solve(monkeypatch, tier, n, d, updater, *, fused, hook=None, iters=ITERS,
           shard=None):
    if fused:
        monkeypatch.delenv("SPARKAGD_STEP_TAIL", raising=False)
    else:
        monkeypatch.setenv("SPARKAGD_STEP_TAIL", "0")
    made, w0 = _shard(n, d, tier)
    rec = _Records()
    w, hist = run(shard or made, LogisticGradient(), updater, 0.0, iters, REG,
                  w0, L0, math.inf, 0.5, 0.9, True,
                  loss_history_mode="backtrack", metrics=rec,
                  iteration_hook=hook, pack_dense=False)
    return w, hist, rec.rows


@pytest.mark.parametrize("tier", TIERS)
@pytest.mark.parametrize("n,d", SHAPES)
def test_same_weights_and_history(monkeypatch, tier, n, d):
    w1, h1, rows1 = _solve(monkeypatch, tier, n, d, SquaredL2Updater(), fused=True)
    w0, h0, rows0 = _solve(monkeypatch, tier, n, d, SquaredL2Updater(), fused=False)
    assert torch.equal(w1, w0)
    assert h1 == h0
    assert len(h1) == ITERS
    for key in ("n_backtracks", "restarted", "L", "theta", "f_y", "norm_dx"):
        assert [r[key] for r in rows1] == [r[key] for r in rows0], key
    # the trajectory takes both branches, or the comparison proves little
    assert sum(r["n_backtracks"] for r in rows1) >= 1
    assert any(r["restarted"] for r in rows1)
    # one fetch per trial; the first iteration also fetches the example
    # count, once for the run
    for i, r in enumerate(rows1):
        assert r["host_fetches"] == 1 + r["n_backtracks"] + (1 if i == 0 else 0), r
    # the kernel-by-kernel sequence drains four times per trial
    assert all(r["host_fetches"] >= 4 for r in rows0)


@pytest.mark.parametrize("tier", TIERS)
def test_same_weights_and_history_simple_updater(monkeypatch, tier):
    n, d = SHAPES[1]
    w1, h1, rows1 = _solve(monkeypatch, tier, n, d, SimpleUpdater(), fused=True)
    w0, h0, _ = _solve(monkeypatch, tier, n, d, SimpleUpdater(), fused=False)
    assert torch.equal(w1, w0)
    assert h1 == h0
    assert all(r["host_fetches"] == 1 + r["n_backtracks"] + (1 if i == 0 else 0)
               for i, r in enumerate(rows1))


def test_trajectory_has_both_branches(monkeypatch):
    """The reference trajectory alone (CPU, kernel-by-kernel sequence)
    backtracks and restarts for both shapes: SEED and ITERS were chosen so."""
    for n, d in SHAPES:
        _, _, rows = _solve(monkeypatch, "cpu", n, d, SquaredL2Updater(), fused=False)
        assert sum(r["n_backtracks"] for r in rows) >= 1
        assert any(r["restarted"] for r in rows)


@pytest.mark.parametrize("tier", TIERS)
def test_changed_count_raises_at_the_fetch(monkeypatch, tier):
    """The example count is fetched once; a shard whose count changes mid-run
    (sample weights swapped between iterations) must stop the run at the next
    fetch, not go on averaging with the stale count."""
    n, d = SHAPES[0]
    shard, _ = _shard(n, d, tier, sample_weight=torch.ones(n))
    seen = []

    def hook(n_iter):
        seen.append(n_iter)
        if n_iter == 3:
            shard.sample_weight = torch.full_like(shard.sample_weight, 2.0)

    with pytest.raises(RuntimeError, match="evaluation count changed"):
        _solve(monkeypatch, tier, n, d, SquaredL2Updater(), fused=True,
               hook=hook, iters=8, shard=shard)
    assert seen == [1, 2, 3]  # raised inside iteration 4, at its first fetch
