"""Multi-task ops: R independent binary problems that share one shard.

A sweep over regularisation strengths scored by k-fold cross-validation is
R = (#lambda x #folds) binary GLMs on the same rows. Stacked as the columns
of one W [d, R] (flattened feature-major, tasks contiguous — the multinomial
layout) they form one separable problem

  F(W) = sum_r [ (1/N_r) sum_{i in train_r} s_i l(z_ir, y_i) + reg_r(w_r) ]

whose margins Z = A·W and gradient Aᵀ·M are exactly the multinomial data
passes (``ops.multiclass``: one stream of A serves every task). What differs
lives here:

* the n-space multiplier: a binary loss per column, with a per-column
  training set given by ``fold_id`` [n] and ``holdout`` [R]
  (task r trains on the rows with ``fold_id != holdout[r]``; ``holdout[r] =
  -1`` trains on every row), and a per-column scale ``task_scale[r] = N/N_r``
  so that the optimizer's division by the shared count N leaves every task
  its own mean;
* the prox with a per-column lambda.

One-vs-rest multiclass is the same stack with a target class per column:
``target`` [R] turns the shard's class-index labels into the binary label
``y_ir = [label_i == target[r]]`` inside the multiplier.

Padding is that of ``multiclass.padded_k``; pad columns of M are exact zeros.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _use_hip, hiplib, reference as _ref
from .multiclass import _pad_classes, padded_k


# --- oracle (plain torch; CPU tier + GPU-kernel ground truth) ---

def ref_multiplier_tasks(
    z: torch.Tensor,  # [n, R] logical margins
    labels: torch.Tensor,
    loss_type: int,
    task_scale: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
    fold_id: Optional[torch.Tensor] = None,
    holdout: Optional[torch.Tensor] = None,
    invert: bool = False,
    target: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(M [n, R], task_loss f64 [R], loss_count f64 [2]) in z's dtype.

    ``a_ir = mask_i · [fold_i != holdout_r]`` (``invert``: ``[fold_i ==
    holdout_r]``, the held-out rows); ``M = a · s · scale · m``;
    ``task_loss[r] = sum_i a_ir s_i l`` (unscaled); ``loss_count = (sum_r
    scale_r · task_loss[r], sum_i mask_i s_i)``. Without ``fold_id`` no row
    is in any fold; without ``holdout`` every task has ``holdout = -1``.

    One-vs-rest: with ``target`` [R] (a class id per task) ``labels`` are
    class indices and task r sees the binary label ``[labels_i ==
    target[r]]`` (1 / 0, the convention of all four binary losses)."""
    n, r = z.shape
    acc = z.dtype
    dev = z.device
    if target is None:
        y = labels.reshape(n, 1)
    else:
        y = (labels.long()[:, None]
             == target.to(device=labels.device, dtype=torch.int64)[None, :])
    m, loss = _ref._multiplier_and_loss(z, y, loss_type)
    row = torch.ones(n, dtype=acc, device=dev)
    if mask is not None:
        row = row * mask.to(acc)
    if sample_weight is not None:
        row = row * sample_weight.to(acc)
    f = (fold_id.to(torch.int64) if fold_id is not None
         else torch.full((n,), -2, dtype=torch.int64, device=dev))
    h = (holdout.to(device=dev, dtype=torch.int64) if holdout is not None
         else torch.full((r,), -1, dtype=torch.int64, device=dev))
    active = f.unsqueeze(1) != h.unsqueeze(0)
    if invert:
        active = ~active
    aw = active.to(acc) * row.unsqueeze(1)
    scale = task_scale.to(device=dev)
    mult = m * aw * scale.to(acc).unsqueeze(0)
    task_loss = (loss * aw).to(torch.float64).sum(dim=0)
    if mask is None and sample_weight is None:
        count = torch.tensor(float(n), dtype=torch.float64, device=dev)
    else:
        count = row.to(torch.float64).sum()
    total = (scale.to(torch.float64) * task_loss).sum()
    return mult, task_loss, torch.stack([total, count])


def ref_prox_tasks(kind: int, w: torch.Tensor, g: torch.Tensor, step: float,
                   lam: torch.Tensor, lam2: torch.Tensor
                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``reference.prox`` applied per column of the flat feature-major
    [d, R] block with (lam[r], lam2[r]); the regularisation value is the sum
    over the tasks (f64 scalar)."""
    r = lam.numel()
    W = w.reshape(-1, r)
    G = g.reshape(-1, r)
    lt = lam.to(device=w.device, dtype=w.dtype)
    lt2 = lam2.to(device=w.device, dtype=w.dtype)
    l64 = lam.to(device=w.device, dtype=torch.float64)
    l64_2 = lam2.to(device=w.device, dtype=torch.float64)
    if kind == _ref.PROX_SIMPLE:
        w_new = W - step * G
        reg = torch.zeros((), dtype=torch.float64, device=w.device)
    elif kind == _ref.PROX_L1:
        w1 = W - step * G
        w_new = torch.sign(w1) * torch.clamp(w1.abs() - lt * step, min=0.0)
        reg = (l64 * w_new.abs().to(torch.float64).sum(dim=0)).sum()
    elif kind == _ref.PROX_SQUARED_L2:
        w_new = W * (1.0 - step * lt) - step * G
        reg = (0.5 * l64 * (w_new.to(torch.float64) ** 2).sum(dim=0)).sum()
    elif kind == _ref.PROX_ELASTIC_NET:
        w1 = W - step * G
        wsoft = torch.sign(w1) * torch.clamp(w1.abs() - lt * step, min=0.0)
        w_new = wsoft / (1.0 + step * lt2)
        reg = ((l64 * w_new.abs().to(torch.float64).sum(dim=0)).sum()
               + (0.5 * l64_2 * (w_new.to(torch.float64) ** 2).sum(dim=0)).sum())
    else:
        raise ValueError(f"unknown prox kind {kind}")
    return w_new.reshape(-1), reg


def ref_at_margin_update_tasks(zm_old: torch.Tensor, xm_old: torch.Tensor,
                               gm: torch.Tensor, step: float,
                               lam: torch.Tensor, theta: float,
                               num_tasks: int
                               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """AT margin update of the padded [n*KC] flats with a shrink per task:

        zm'[:, r] = (1 - step*lam[r])*zm[:, r] - step*gm[:, r]
        xm'       = (1 - theta)*xm + theta*zm'

    for r < num_tasks, the coefficient formed in f64 and cast to the margins'
    dtype. Pad columns of both outputs are exact zeros and are never read."""
    kc = padded_k(num_tasks)
    n = zm_old.numel() // kc
    dt = zm_old.dtype
    pz = (1.0 - step * lam.to(device=zm_old.device, dtype=torch.float64)).to(dt)
    live = slice(0, num_tasks)
    zm_new = torch.zeros((n, kc), dtype=dt, device=zm_old.device)
    xm_new = torch.zeros((n, kc), dtype=dt, device=zm_old.device)
    zn = (pz.unsqueeze(0) * zm_old.reshape(n, kc)[:, live]
          - step * gm.reshape(n, kc)[:, live])
    zm_new[:, live] = zn
    xm_new[:, live] = (1.0 - theta) * xm_old.reshape(n, kc)[:, live] + theta * zn
    return zm_new.reshape(-1), xm_new.reshape(-1)


def ref_colsum_multi(m_padded_flat: torch.Tensor, num_tasks: int
                     ) -> torch.Tensor:
    """f64 [R] column sums of the padded [n*KC] multiplier."""
    kc = padded_k(num_tasks)
    return (m_padded_flat.reshape(-1, kc)[:, :num_tasks]
            .to(torch.float64).sum(dim=0))


def ref_add_bias_cols(z_padded_flat: torch.Tensor, coef: float,
                      src: torch.Tensor, idx0: int, num_tasks: int
                      ) -> torch.Tensor:
    """In place Z[:, c] += coef * src[idx0 + c] for c < R, the product
    rounded in Z's dtype; pad columns are not touched."""
    kc = padded_k(num_tasks)
    z = z_padded_flat.view(-1, kc)
    b = src[idx0:idx0 + num_tasks].to(z.dtype)
    z[:, :num_tasks] += (coef * b).unsqueeze(0)
    return z_padded_flat


def ref_at_margin_update_tasks_off(zm_old: torch.Tensor, xm_old: torch.Tensor,
                                   gm: torch.Tensor, step: float,
                                   lam: torch.Tensor, theta: float,
                                   num_tasks: int, z_old: torch.Tensor,
                                   idx0: int
                                   ) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ref_at_margin_update_tasks`` with a free bias row:

        zm'[:, r] = pz_r*zm[:, r] - step*gm[:, r] + (1 - pz_r)*z_old[idx0 + r]

    with pz_r = 1 - step*lam[r] and 1 - pz_r formed in f64 and cast."""
    kc = padded_k(num_tasks)
    n = zm_old.numel() // kc
    dt = zm_old.dtype
    pz64 = 1.0 - step * lam.to(device=zm_old.device, dtype=torch.float64)
    pz = pz64.to(dt)
    omp = (1.0 - pz64).to(dt)
    zb = z_old[idx0:idx0 + num_tasks].to(dt)
    live = slice(0, num_tasks)
    zm_new = torch.zeros((n, kc), dtype=dt, device=zm_old.device)
    xm_new = torch.zeros((n, kc), dtype=dt, device=zm_old.device)
    zn = (pz.unsqueeze(0) * zm_old.reshape(n, kc)[:, live]
          - step * gm.reshape(n, kc)[:, live] + (omp * zb).unsqueeze(0))
    zm_new[:, live] = zn
    xm_new[:, live] = (1.0 - theta) * xm_old.reshape(n, kc)[:, live] + theta * zn
    return zm_new.reshape(-1), xm_new.reshape(-1)


def ref_prox_tasks_free(kind: int, w: torch.Tensor, g: torch.Tensor,
                        step: float, lam: torch.Tensor, lam2: torch.Tensor,
                        n_free: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``ref_prox_tasks`` on all but the last ``n_free`` elements, which take
    ``w - step*g`` and add nothing to the regularisation value."""
    n_reg = w.numel() - n_free
    head, reg = ref_prox_tasks(kind, w[:n_reg], g[:n_reg], step, lam, lam2)
    return torch.cat([head, w[n_reg:] - step * g[n_reg:]]), reg


# --- dispatch (GPU -> HIP kernels via hiplib; CPU -> oracle) ---

def multiplier_tasks(
    margins_padded_flat: torch.Tensor,
    labels: torch.Tensor,
    loss_type: int,
    num_tasks: int,
    task_scale: torch.Tensor,
    mask: Optional[torch.Tensor] = None,
    sample_weight: Optional[torch.Tensor] = None,
    fold_id: Optional[torch.Tensor] = None,
    holdout: Optional[torch.Tensor] = None,
    invert: bool = False,
    need_mult: bool = True,
    target: Optional[torch.Tensor] = None,
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(M padded flat [n*KC] or None, task_loss f64 [R], loss_count f64 [2])
    from padded margins [n*KC] — zero data passes. ``need_mult=False`` is the
    loss-only call (no M is written). ``target`` [R]: one-vs-rest, task r
    against the label ``[labels == target[r]]``."""
    kc = padded_k(num_tasks)
    if target is not None and target.numel() != num_tasks:
        raise ValueError("target must be [num_tasks]")
    if _use_hip(margins_padded_flat):
        return hiplib.multiplier_tasks(
            margins_padded_flat, labels, loss_type, num_tasks, kc, task_scale,
            mask, sample_weight, fold_id, holdout, invert, need_mult, target)
    n = margins_padded_flat.numel() // kc
    z = margins_padded_flat.reshape(n, kc)[:, :num_tasks]
    m, task_loss, lc = ref_multiplier_tasks(
        z, labels, loss_type, task_scale, mask, sample_weight, fold_id,
        holdout, invert, target)
    if not need_mult:
        return None, task_loss, lc
    return _pad_classes(m, kc).reshape(-1), task_loss, lc


def prox_tasks(kind: int, w: torch.Tensor, g: torch.Tensor, step: float,
               lam: torch.Tensor, lam2: torch.Tensor, n_free: int = 0
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One proximal step of every task + the summed regularisation value;
    ``lam`` / ``lam2`` are [R] (f64). ``n_free``: the last ``n_free`` elements
    of the flat block (the bias row of a [(d+1), R] block: ``n_free = R``)
    take the plain step ``w - step*g`` and are not regularised."""
    if not 0 <= n_free <= w.numel() or (w.numel() - n_free) % lam.numel():
        raise ValueError(
            f"prox_tasks: [{w.numel()}] weights with {n_free} free elements "
            f"are not a [d, {lam.numel()}] block")
    if _use_hip(w):
        return hiplib.prox_tasks(kind, w, g, step, lam, lam2, n_free)
    if n_free:
        return ref_prox_tasks_free(kind, w, g, step, lam, lam2, n_free)
    return ref_prox_tasks(kind, w, g, step, lam, lam2)


def at_margin_update_tasks(zm_old: torch.Tensor, xm_old: torch.Tensor,
                           gm: torch.Tensor, step: float, lam: torch.Tensor,
                           theta: float, num_tasks: int,
                           offset: Optional[Tuple[torch.Tensor, int]] = None
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused AT margin update of a multi-task run whose prox is affine per
    column (simple: ``lam`` zeros; squared L2): (zm', xm') from the padded
    [n*KC] margins of z, x and the gradient in one pass; ``lam`` is [R]
    (f64). Pad columns of the outputs are exact zeros. ``offset = (z_old,
    idx0)``: the weights carry an unpenalised bias row at ``idx0`` and column
    r gains ``step*lam[r] * z_old[idx0 + r]``, read on the device."""
    if lam.numel() != num_tasks:
        raise ValueError(f"lam has {lam.numel()} entries for {num_tasks} tasks")
    if _use_hip(zm_old):
        return hiplib.at_margin_update_tasks(zm_old, xm_old, gm, step, lam,
                                             theta, num_tasks,
                                             padded_k(num_tasks), offset)
    if offset is not None:
        return ref_at_margin_update_tasks_off(zm_old, xm_old, gm, step, lam,
                                              theta, num_tasks, offset[0],
                                              int(offset[1]))
    return ref_at_margin_update_tasks(zm_old, xm_old, gm, step, lam, theta,
                                      num_tasks)


def colsum_multi(m_padded_flat: torch.Tensor, num_tasks: int,
                 tail: Optional[torch.Tensor] = None, want_f64: bool = True
                 ) -> Optional[torch.Tensor]:
    """``sum_i M[i, c]`` for c < R of the padded [n*KC] multiplier,
    accumulated in f64: the bias row of the gradient. ``tail`` (a contiguous
    [R] view, the last row of the gradient block) receives the sums in its
    dtype; the f64 [R] sums are returned when ``want_f64``."""
    if _use_hip(m_padded_flat):
        return hiplib.colsum_multi(m_padded_flat, num_tasks,
                                   padded_k(num_tasks), tail, want_f64)
    sums = ref_colsum_multi(m_padded_flat, num_tasks)
    if tail is not None:
        tail.copy_(sums)
    return sums if want_f64 else None


def add_bias_cols(z_padded_flat: torch.Tensor, coef: float, src: torch.Tensor,
                  idx0: int, num_tasks: int) -> torch.Tensor:
    """In place ``Z[i, c] += coef * src[idx0 + c]`` for c < R on the padded
    [n*KC] margins; ``src`` is the weight vector the biases live in. Pad
    columns are left as they are."""
    if idx0 < 0 or idx0 + num_tasks > src.numel():
        raise IndexError(
            f"biases [{idx0}, {idx0 + num_tasks}) outside [0, {src.numel()})")
    if _use_hip(z_padded_flat):
        return hiplib.add_bias_cols_(z_padded_flat, coef, src, idx0,
                                     num_tasks, padded_k(num_tasks))
    return ref_add_bias_cols(z_padded_flat, coef, src, idx0, num_tasks)
