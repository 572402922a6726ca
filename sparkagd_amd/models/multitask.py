"""Multi-task plug-ins: R independent binary problems trained in one run.

``MultiTaskGradient`` stacks R copies of one binary loss — each with its own
training rows (all rows but one held-out fold) — as the columns of a [d, R]
weight block, so every stream of the shard serves all R tasks;
``PerTaskUpdater`` gives each column its own regularisation strength. The
optimizer is generic over Gradient/Updater and runs the stacked problem
unchanged.

Known property: the tasks share one backtracked Lipschitz estimate L, one θ
sequence and one restart test (lambda lives in the prox, so the smooth parts
have essentially one Lipschitz constant). They therefore converge together,
paced by the slowest task.
"""

from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from .gradient import Gradient
from .updater import (ElasticNetUpdater, FreeTailUpdater, SimpleUpdater,
                      SquaredL2Updater, Updater)


class MultiTaskGradient(Gradient):
    """R binary problems sharing one shard: task r minimises the mean of
    ``base``'s loss over the rows with ``fold_id != holdout[r]``
    (``holdout[r] = -1``, or no ``fold_id`` at all: every row).

    Weights are the flattened [d, R] block (feature-major, tasks
    contiguous); margins are the padded [n, KC] flats of the multinomial
    path, so margin tracking works as for softmax. ``eval`` returns
    ``count = N = sum_i mask_i s_i`` and scales column r by ``N / N_r``
    (full-data totals, all-reduced over ``comm`` at construction): after the
    optimizer's division by the all-reduced count every task carries its own
    mean loss and gradient, and the reported loss is the sum of the R means.

    ``sample_weight`` must be the shard's ``sample_weight`` when it has one:
    the fold totals N_r are weighted sums. Dense and CSR shards only; direct
    solver only.
    """

    IS_MULTICLASS = True  # [n, KC] margins, shard left raw by the pack policy
    IS_MULTITASK = True

    def __init__(self, base: Gradient, num_tasks: int,
                 fold_id: Optional[torch.Tensor] = None,
                 holdout: Optional[Sequence[int]] = None, comm=None,
                 sample_weight: Optional[torch.Tensor] = None):
        if getattr(base, "IS_MULTICLASS", False) or getattr(base, "LOSS_TYPE", -1) < 0:
            raise ValueError("base must be one of the binary gradients")
        if num_tasks < 1:
            raise ValueError("num_tasks must be >= 1")
        self.base = base
        self.LOSS_TYPE = base.LOSS_TYPE
        self.num_tasks = int(num_tasks)
        self.num_classes = self.num_tasks
        self.fold_id = None
        self.holdout = None
        self._weighted = sample_weight is not None
        if holdout is not None:
            h = torch.as_tensor(holdout, dtype=torch.int64).reshape(-1).cpu()
            if h.numel() != self.num_tasks:
                raise ValueError("holdout must have one entry per task")
            if bool((h < -1).any()):
                raise ValueError("holdout entries are fold ids or -1")
            if bool((h >= 0).any()) and fold_id is None:
                raise ValueError("a held-out fold needs fold_id")
            self.holdout = h.to(torch.int32)
        n_train = None
        if fold_id is not None:
            if fold_id.ndim != 1 or fold_id.dtype.is_floating_point:
                raise ValueError("fold_id must be an integer [n] tensor")
            if fold_id.numel() and int(fold_id.min()) < 0:
                raise ValueError("fold ids must be >= 0")
            if sample_weight is not None and sample_weight.numel() != fold_id.numel():
                raise ValueError("sample_weight must be [n] like fold_id")
            self.fold_id = fold_id.to(torch.int32).contiguous()
            n_train = self._train_totals(fold_id, sample_weight, comm)
        if n_train is None:
            scale = torch.ones(self.num_tasks, dtype=torch.float64)
        else:
            total, per_task = n_train
            empty = [r for r in range(self.num_tasks) if per_task[r] <= 0.0]
            if empty:
                raise ValueError(
                    f"tasks {empty} have no training rows (N_r = 0): every "
                    "row lies in their held-out fold")
            scale = torch.tensor([total / v for v in per_task],
                                 dtype=torch.float64)
        #: N / N_r per task (f64, host)
        self.task_scale = scale
        #: unscaled per-task loss sums of the last evaluation (f64 [R], local)
        self.last_task_loss: Optional[torch.Tensor] = None
        self._dev_cache = {}

    def _train_totals(self, fold_id, sample_weight, comm):
        """(N, [N_r]) from the f64 bincount of fold_id weighted by
        sample_weight, all-reduced over ``comm``."""
        from ..parallel.comm import Communicator

        comm = comm or Communicator()
        h = (self.holdout.to(torch.int64) if self.holdout is not None
             else torch.full((self.num_tasks,), -1, dtype=torch.int64))
        nf = torch.tensor(
            [max(int(fold_id.max()) + 1 if fold_id.numel() else 0,
                 int(h.max()) + 1, 1)], dtype=torch.int64)
        comm.allreduce_(nf, op="max")
        f = fold_id.to(device="cpu", dtype=torch.int64)
        wts = (sample_weight.to(device="cpu", dtype=torch.float64)
               if sample_weight is not None
               else torch.ones(f.numel(), dtype=torch.float64))
        per_fold = torch.bincount(f, weights=wts, minlength=int(nf[0]))
        comm.allreduce_(per_fold)
        total = float(per_fold.sum())
        per_task = [total - float(per_fold[int(hr)]) if hr >= 0 else total
                    for hr in h.tolist()]
        return total, per_task

    # --- shard plumbing ---
    def _check_shard(self, shard):
        kind = getattr(shard, "kind", None)
        if kind not in ("dense", "csr"):
            raise ValueError(
                "MultiTaskGradient trains on dense and CSR shards only; got "
                f"{type(shard).__name__} (kind={kind!r}). Intercept, mixed "
                "and host-streamed shards are not supported")
        if self.fold_id is not None and self.fold_id.numel() != shard.n:
            raise ValueError(
                f"fold_id has {self.fold_id.numel()} entries, the shard "
                f"{shard.n} rows")
        if (shard.sample_weight is not None) != self._weighted:
            raise ValueError(
                "MultiTaskGradient must be built with the shard's "
                "sample_weight (and without one for an unweighted shard): "
                "the fold totals N_r are weighted sums")

    def _on(self, device):
        """(fold_id, holdout, task_scale) placed on ``device`` (cached)."""
        t = self._dev_cache.get(device)
        if t is None:
            scale = self.task_scale.to(
                device=device,
                dtype=torch.float32 if device.type == "cuda" else torch.float64)
            t = (None if self.fold_id is None else self.fold_id.to(device),
                 None if self.holdout is None else self.holdout.to(device),
                 scale)
            self._dev_cache[device] = t
        return t

    def rounds_margin_weights(self, shard) -> bool:
        """True when the training ``margins`` pass rounds its weight operand:
        a bf16 dense shard on the GPU runs it as a bf16 x bf16 GEMM. Margins
        tracked through such a pass carry 2^-9 of every INCREMENT of z, not
        of z itself; where a column's shrink 1 - step*lambda leaves (-1, 1)
        that error is not damped, and a mixed sweep shares one step among
        columns with very different lambdas."""
        return (shard.kind == "dense" and shard.features.is_cuda
                and shard.features.dtype == torch.bfloat16)

    def margins(self, shard, v, scoring=False):
        """Padded margins [n*KC] of the weight block ``v``. ``scoring=True``
        keeps the f32 weights of a bf16 dense shard (split into two bf16
        GEMM operands) where the training route rounds them to bf16."""
        from ..ops import multiclass as mc
        from ..ops import multitask as mt

        self._check_shard(shard)
        if shard.kind == "csr":
            return mc.csr_margins_multi(shard, v, self.num_tasks)
        if scoring:
            return mt.dense_margins_scoring(shard.features, v, self.num_tasks)
        return mc.margins_multi(shard.features, v, self.num_tasks)

    def task_losses(self, shard, margins, mask=None, invert=False):
        """(task_loss f64 [R], loss_count f64 [2]) of the local rows from
        padded margins — the loss-only multiplier call; ``invert=True`` sums
        each task's HELD-OUT rows instead of its training rows."""
        from ..ops import multitask as mt

        self._check_shard(shard)
        fold, hold, scale = self._on(margins.device)
        _, task_loss, lc = mt.multiplier_tasks(
            margins, shard.labels, self.LOSS_TYPE, self.num_tasks, scale, mask,
            shard.sample_weight, fold, hold, invert, need_mult=False)
        return task_loss, lc

    def multiplier_loss(self, shard, margins, mask=None):
        """(padded multiplier flat [n*KC], loss_count) from padded margins —
        the n-space stage (zero data passes)."""
        from ..ops import multitask as mt

        self._check_shard(shard)
        fold, hold, scale = self._on(margins.device)
        m, task_loss, lc = mt.multiplier_tasks(
            margins, shard.labels, self.LOSS_TYPE, self.num_tasks, scale, mask,
            shard.sample_weight, fold, hold)
        self.last_task_loss = task_loss
        return m, lc

    def eval_from_margins(self, shard, margins, mask=None, need_grad=True):
        from ..ops import multitask as mt

        if not need_grad:
            task_loss, lc = self.task_losses(shard, margins, mask)
            self.last_task_loss = task_loss
            return None, lc
        m, lc = self.multiplier_loss(shard, margins, mask)
        if shard.kind == "csr":
            return mt.csr_grad_tasks(shard, m, self.num_tasks), lc
        return mt.dense_grad_tasks(shard.features, m, self.num_tasks), lc

    def eval(self, shard, w, mask=None, need_grad=True):
        return self.eval_from_margins(shard, self.margins(shard, w), mask,
                                      need_grad)

    def compute(self, features, label, weights, cum_gradient):
        raise NotImplementedError(
            "the per-example MLlib API is that of the base gradient")


class PerTaskUpdater(Updater):
    """``base``'s prox with a regularisation strength per task: column r of
    the flat [d, R] weights is regularised by ``reg_param * lambdas[r]``
    (``ElasticNetUpdater`` splits it by its ``l1_ratio``); the regularisation
    value is the sum over the tasks.

    ``AFFINE_PROX`` stays False: that flag promises ONE (pz, pg) pair for the
    whole margin vector (the scalar fused update, the Gram solver), and here
    the shrink differs per column. A ``SimpleUpdater`` or ``SquaredL2Updater``
    base is still affine column by column, which the instance attribute
    ``COLUMN_AFFINE_PROX`` says: the optimizer then tracks the margins of a
    ``MultiTaskGradient`` run through ``prox_margins_tasks`` (two shard
    streams per step, as with one lambda; on a bf16 dense GPU shard only with
    ``track_margins=True``, see ``MultiTaskGradient.rounds_margin_weights``).
    L1 and elastic-net bases are not affine and run untracked."""

    AFFINE_PROX = False

    def __init__(self, base: Updater, lambdas: Sequence[float]):
        if isinstance(base, (PerTaskUpdater, FreeTailUpdater)) or base.PROX_KIND < 0:
            raise ValueError("base must be one of the four plain updaters")
        lam = torch.as_tensor(lambdas, dtype=torch.float64).reshape(-1).cpu()
        if lam.numel() < 1 or bool((lam < 0).any()) or not bool(torch.isfinite(lam).all()):
            raise ValueError("lambdas must be finite and >= 0, one per task")
        self.base = base
        self.PROX_KIND = base.PROX_KIND
        self.lambdas = lam
        self.num_tasks = lam.numel()
        #: the prox is affine in (w, g) column by column (see the class doc)
        self.COLUMN_AFFINE_PROX = type(base) in (SimpleUpdater, SquaredL2Updater)
        self._cache = {}

    def _lams(self, reg_param: float, device):
        """(lam, lam2) f64 [R] on ``device`` for this reg_param (cached: the
        optimizer passes the same reg_param every step)."""
        key = (float(reg_param), device)
        t = self._cache.get(key)
        if t is None:
            eff = self.lambdas * float(reg_param)
            if isinstance(self.base, ElasticNetUpdater):
                lam, lam2 = self.base.l1_ratio * eff, (1.0 - self.base.l1_ratio) * eff
            elif isinstance(self.base, SimpleUpdater):
                # no regulariser: the prox ignores lam, the margin update
                # must see zeros
                lam, lam2 = torch.zeros_like(eff), torch.zeros_like(eff)
            else:
                lam, lam2 = eff, torch.zeros_like(eff)
            t = (lam.to(device), lam2.to(device))
            self._cache = {key: t}
        return t

    def compute(self, weights_old, gradient, step_size, iter, reg_param):  # noqa: A002
        from ..ops import multitask as mt

        if weights_old.numel() % self.num_tasks != 0:
            raise ValueError(
                f"weights [{weights_old.numel()}] are not a [d, "
                f"{self.num_tasks}] block")
        lam, lam2 = self._lams(reg_param, weights_old.device)
        return mt.prox_tasks(self.PROX_KIND, weights_old, gradient,
                             step_size / math.sqrt(iter), lam, lam2)

    def prox_margins_tasks(self, zm_old, xm_old, gm, step, reg_param, theta):
        """(zm', xm') of the padded [n*KC] margins after the prox step
        ``compute`` takes at ``step`` and the AT interpolation at ``theta``;
        only valid when ``COLUMN_AFFINE_PROX``. The lambdas are the cached
        device vector of ``compute``: the step copies nothing to the device."""
        from ..ops import multitask as mt

        if not self.COLUMN_AFFINE_PROX:
            raise NotImplementedError(
                f"PerTaskUpdater({type(self.base).__name__}) has no affine prox")
        lam, _ = self._lams(reg_param, zm_old.device)
        return mt.at_margin_update_tasks(zm_old, xm_old, gm, step, lam, theta,
                                         self.num_tasks)

    def reg_value(self, weights, reg_param):
        return self.compute(weights, torch.zeros_like(weights), 0.0, 1,
                            reg_param)[1]
