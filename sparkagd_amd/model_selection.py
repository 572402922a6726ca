"""Model selection: k-fold cross-validation of a regularisation sweep in ONE
training run.

A sweep of L regularisation strengths scored by F-fold cross-validation is
R = L·F binary GLMs over the same rows. ``cross_validate`` stacks them as the
columns of one [d, R] weight block (``MultiTaskGradient`` /
``PerTaskUpdater``), so every stream of the shard serves all R models instead
of one, then scores every model on its held-out fold with one more margins
pass.
"""

from __future__ import annotations

import dataclasses
import math
from typing import List, Optional, Sequence

import torch

from .config import AGDConfig
from .models.gradient import Gradient, LogisticGradient
from .models.multitask import MultiTaskGradient, PerTaskUpdater
from .models.updater import SquaredL2Updater, Updater
from .parallel.comm import Communicator

_LINKS = {0: "logistic", 1: "identity", 2: "hinge", 3: "hinge"}


def assign_folds(n_local: int, n_folds: int, seed: int, rank: int = 0) -> torch.Tensor:
    """Uniform random fold ids in [0, n_folds) for ``n_local`` rows (i32,
    CPU), seeded per rank so that the ranks of a sharded run draw independent
    streams and a rerun draws the same ones."""
    if n_folds < 1:
        raise ValueError("n_folds must be >= 1")
    gen = torch.Generator(device="cpu")
    gen.manual_seed((int(seed) * 1000003 + int(rank) * 7919) % (2**63 - 1))
    return torch.randint(0, n_folds, (int(n_local),), generator=gen,
                         dtype=torch.int32)


@dataclasses.dataclass
class CVResult:
    """Outcome of :func:`cross_validate`.

    ``heldout_loss[l, f]`` is the ``sample_weight``-weighted mean loss of the
    model trained at ``lambdas[l]`` without fold f, on fold f;
    ``mean_loss`` / ``std_loss`` [L] are its mean and (population) standard
    deviation over the folds; ``best_lambda`` minimises the mean (ties go to
    the larger lambda); ``fold_weights[l, f]`` are that model's weights [d];
    ``loss_history`` is the stacked run's (sum over the R tasks of mean
    training loss + regulariser); ``model`` is the refit on all rows at
    ``best_lambda`` (None with ``refit=False``)."""

    lambdas: List[float]
    heldout_loss: torch.Tensor
    mean_loss: torch.Tensor
    std_loss: torch.Tensor
    best_lambda: float
    fold_weights: torch.Tensor
    loss_history: List[float]
    model: Optional[object] = None


def cross_validate(
    data,
    lambdas: Sequence[float],
    n_folds: int = 5,
    gradient: Optional[Gradient] = None,
    updater: Optional[Updater] = None,
    num_iterations: int = 100,
    convergence_tol: float = 1e-6,
    seed: int = 0,
    comm: Optional[Communicator] = None,
    config: Optional[AGDConfig] = None,
    refit: bool = True,
    fold_id: Optional[torch.Tensor] = None,
) -> CVResult:
    """k-fold cross-validation of ``lambdas`` for a binary GLM: all
    ``len(lambdas) * n_folds`` models train in one ``run()`` over the shard,
    then one margins pass plus one loss-only multiplier call score each on
    its held-out fold.

    ``gradient`` is one of the binary gradients (default logistic),
    ``updater`` one of the plain updaters (default squared L2); the
    regularisation strength of a model is its entry of ``lambdas``
    (``config.reg_param`` is not used). Rows are assigned to folds by
    ``assign_folds(data.n, n_folds, seed, comm.rank)`` unless ``fold_id``
    [n_local] is given. Dense and CSR shards, direct solver.

    The R tasks share one step size, θ sequence and restart test, so they
    converge together, paced by the slowest. With a simple or squared-L2
    updater the run tracks its margins (two shard streams per step), whether
    the lambdas are equal or mixed: a mixed sweep updates them with one shrink
    per column. ``config.track_margins=False`` keeps the untracked path
    (three streams with ``loss_history_mode="backtrack"``, four at the
    defaults), which is also what an L1 or elastic-net sweep runs. One
    exception: a MIXED sweep on a bf16 dense shard on the GPU is tracked only
    with ``config.track_margins=True``. Its margins GEMM rounds the weights
    to bf16, tracked margins then carry that rounding of every increment,
    and a column whose ``step * lambda`` passes 1 does not damp it: with
    lambdas spread over decades under one shared step, a tracked run was
    seen to pick another ``best_lambda`` than the f64 run.
    """
    from .optimizer import run

    comm = comm or Communicator()
    cfg = dataclasses.replace(config) if config is not None else AGDConfig()
    cfg.num_iterations = num_iterations
    cfg.convergence_tol = convergence_tol
    cfg.validate()
    if cfg.solver == "gram":
        raise ValueError("cross_validate runs on the direct solver only "
                         "(config.solver='gram' is not supported)")
    lams = [float(v) for v in lambdas]
    if not lams or any(v < 0 or not math.isfinite(v) for v in lams):
        raise ValueError("lambdas must be a non-empty list of finite values >= 0")
    if getattr(data, "kind", None) not in ("dense", "csr"):
        raise ValueError(
            "cross_validate supports dense and CSR shards only; got "
            f"{type(data).__name__}")
    gradient = gradient or LogisticGradient()
    updater = updater or SquaredL2Updater()
    n_l, n_f = len(lams), int(n_folds)
    if fold_id is None:
        fold_id = assign_folds(data.n, n_f, seed, comm.rank)
    holdout = [f for _ in range(n_l) for f in range(n_f)]
    task_lams = [lam for lam in lams for _ in range(n_f)]
    n_tasks = n_l * n_f
    mt_grad = MultiTaskGradient(gradient, n_tasks, fold_id, holdout, comm,
                                sample_weight=data.sample_weight)

    # held-out weight per fold (denominators), all-reduced like the N_r
    sw = data.sample_weight
    per_fold = torch.bincount(
        fold_id.to(device="cpu", dtype=torch.int64),
        weights=(sw.to(device="cpu", dtype=torch.float64) if sw is not None
                 else torch.ones(data.n, dtype=torch.float64)),
        minlength=n_f)[:n_f].clone()
    comm.allreduce_(per_fold)
    if bool((per_fold <= 0).any()):
        raise ValueError(
            f"folds {torch.nonzero(per_fold <= 0).flatten().tolist()} hold "
            "no rows: nothing to score them on")

    if len(set(task_lams)) == 1:
        # one lambda: the plain updater keeps margin tracking on
        run_updater, reg_param = updater, task_lams[0]
    else:
        run_updater, reg_param = PerTaskUpdater(updater, task_lams), 1.0
    wdtype = torch.float64 if data.device.type == "cpu" else torch.float32
    w0 = torch.zeros(data.d * n_tasks, device=data.device, dtype=wdtype)
    w, hist = run(
        data, mt_grad, run_updater, cfg.convergence_tol, cfg.num_iterations,
        reg_param, w0, cfg.L0, cfg.Lexact, cfg.beta, cfg.alpha,
        cfg.may_restart, loss_history_mode=cfg.loss_history_mode, comm=comm,
        track_margins=cfg.track_margins,
        margin_refresh_every=cfg.margin_refresh_every,
        backtrack_tol=cfg.backtrack_tol)

    # held-out scoring: one margins pass + one loss-only multiplier call
    zf = mt_grad.margins(data, w, scoring=True)
    num, _ = mt_grad.task_losses(data, zf, invert=True)
    num = num.clone()
    comm.allreduce_(num)
    heldout = (num.cpu().reshape(n_l, n_f) / per_fold.reshape(1, n_f))
    mean = heldout.mean(dim=1)
    std = heldout.std(dim=1, unbiased=False)
    best_val = float(mean.min())
    best = max(lam for lam, m in zip(lams, mean.tolist()) if m == best_val)
    fold_w = w.reshape(data.d, n_tasks).T.reshape(n_l, n_f, data.d).contiguous()

    model = None
    if refit:
        from .models.trainers import _GLMTrainer

        trainer = type("_RefitTrainer", (_GLMTrainer,), {
            "GRADIENT_CLS": type(gradient),
            "LINK": _LINKS.get(gradient.LOSS_TYPE, "logistic")})
        model = trainer.train(
            data, num_iterations=num_iterations, reg_param=best,
            convergence_tol=convergence_tol, updater=updater, comm=comm,
            config=dataclasses.replace(cfg))
    return CVResult(lams, heldout, mean, std, best, fold_w, hist, model)
