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

Padding is that of ``multiclass.padded_k``; pad columns of M are exact zeros.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _use_hip, reference as _ref
from .multiclass import _pad_classes, padded_k, ref_csr_grad_multi


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
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(M [n, R], task_loss f64 [R], loss_count f64 [2]) in z's dtype.

    ``a_ir = mask_i · [fold_i != holdout_r]`` (``invert``: ``[fold_i ==
    holdout_r]``, the held-out rows); ``M = a · s · scale · m``;
    ``task_loss[r] = sum_i a_ir s_i l`` (unscaled); ``loss_count = (sum_r
    scale_r · task_loss[r], sum_i mask_i s_i)``. Without ``fold_id`` no row
    is in any fold; without ``holdout`` every task has ``holdout = -1``."""
    n, r = z.shape
    acc = z.dtype
    dev = z.device
    m, loss = _ref._multiplier_and_loss(z, labels.reshape(n, 1), loss_type)
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
) -> Tuple[Optional[torch.Tensor], torch.Tensor, torch.Tensor]:
    """(M padded flat [n*KC] or None, task_loss f64 [R], loss_count f64 [2])
    from padded margins [n*KC] — zero data passes. ``need_mult=False`` is the
    loss-only call (no M is written)."""
    kc = padded_k(num_tasks)
    if _use_hip(margins_padded_flat):
        from . import hiplib

        return hiplib.multiplier_tasks(
            margins_padded_flat, labels, loss_type, num_tasks, kc, task_scale,
            mask, sample_weight, fold_id, holdout, invert, need_mult)
    n = margins_padded_flat.numel() // kc
    z = margins_padded_flat.reshape(n, kc)[:, :num_tasks]
    m, task_loss, lc = ref_multiplier_tasks(
        z, labels, loss_type, task_scale, mask, sample_weight, fold_id,
        holdout, invert)
    if not need_mult:
        return None, task_loss, lc
    return _pad_classes(m, kc).reshape(-1), task_loss, lc


def prox_tasks(kind: int, w: torch.Tensor, g: torch.Tensor, step: float,
               lam: torch.Tensor, lam2: torch.Tensor
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """One proximal step of every task + the summed regularisation value;
    ``lam`` / ``lam2`` are [R] (f64)."""
    if _use_hip(w):
        from . import hiplib

        return hiplib.prox_tasks(kind, w, g, step, lam, lam2)
    return ref_prox_tasks(kind, w, g, step, lam, lam2)


def at_margin_update_tasks(zm_old: torch.Tensor, xm_old: torch.Tensor,
                           gm: torch.Tensor, step: float, lam: torch.Tensor,
                           theta: float, num_tasks: int
                           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Fused AT margin update of a multi-task run whose prox is affine per
    column (simple: ``lam`` zeros; squared L2): (zm', xm') from the padded
    [n*KC] margins of z, x and the gradient in one pass; ``lam`` is [R]
    (f64). Pad columns of the outputs are exact zeros."""
    if lam.numel() != num_tasks:
        raise ValueError(f"lam has {lam.numel()} entries for {num_tasks} tasks")
    if _use_hip(zm_old):
        from . import hiplib

        return hiplib.at_margin_update_tasks(zm_old, xm_old, gm, step, lam,
                                             theta, num_tasks,
                                             padded_k(num_tasks))
    return ref_at_margin_update_tasks(zm_old, xm_old, gm, step, lam, theta,
                                      num_tasks)


def dense_margins_scoring(features: torch.Tensor, wflat: torch.Tensor,
                          k: int) -> torch.Tensor:
    """Flat padded margins [n*KC] for SCORING returned weights. The training
    route of a bf16 shard (``multiclass.margins_multi``) rounds W to bf16 for
    its GEMM, a 2^-9 relative change of every weight: harmless inside the
    iteration, but a score must belong to the weights the caller gets back.
    Here W goes in as bf16(W) + bf16(W - bf16(W)), two accumulating
    hipBLASLt GEMMs (2^-17 per weight) at about twice the one-GEMM cost — the
    exact-f32 VALU kernel would cost ~12 A-streams. Every other shard dtype
    already multiplies the exact weights."""
    from .multiclass import margins_multi

    if not (_use_hip(features) and features.dtype == torch.bfloat16):
        return margins_multi(features, wflat, k)
    from . import hiplib

    kc = padded_k(k)
    n, d = features.shape
    wt = torch.zeros((kc, d), dtype=torch.float32, device=features.device)
    wt[:k] = wflat.reshape(d, k).T
    hi = wt.to(torch.bfloat16)
    lo = (wt - hi.to(torch.float32)).to(torch.bfloat16)
    z = torch.empty((n, kc), dtype=torch.float32, device=features.device)
    hiplib.gemm_bf16f32_nt(features, hi, z)
    hiplib.gemm_bf16f32_nt(features, lo, z, beta=1.0)
    return z.reshape(-1)


def dense_grad_tasks(features: torch.Tensor, m_padded_flat: torch.Tensor,
                     k: int) -> torch.Tensor:
    """grad flat [d*k] = Aᵀ·M on a dense shard: ``grad_from_mult_multi``,
    plus the rocBLAS route the multinomial path takes for an f32 shard with
    more than 32 columns (no VALU kernel above the KC=32 template)."""
    from .multiclass import grad_from_mult_multi

    kc = padded_k(k)
    if (_use_hip(features) and kc > 32
            and features.dtype == torch.float32):
        n = features.shape[0]
        return (features.T @ m_padded_flat.reshape(n, kc)[:, :k]).reshape(-1)
    return grad_from_mult_multi(features, m_padded_flat, k)


def csr_grad_tasks(shard, m_padded_flat: torch.Tensor, k: int) -> torch.Tensor:
    """grad flat [d*k] = Aᵀ·M on a CSR shard from the padded multiplier: the
    deterministic CSC gather (k_csc_grad_multi; 32-column chunks above
    KC = 32), the index_add oracle on CPU."""
    kc = padded_k(k)
    n = shard.n
    if not _use_hip(shard.val):
        m = m_padded_flat.reshape(n, kc)[:, :k]
        return ref_csr_grad_multi(shard.rowptr, shard.col, shard.val, m, shard.d)
    from . import hiplib

    if shard.csc is None:
        raise RuntimeError(
            "CSR multi-task gradient needs the deterministic CSC copy "
            "(CSRShard(..., deterministic=True))")
    colptr, crow, cval = shard.csc
    heavy = getattr(shard, "csc_heavy", None)
    if kc <= 32:
        gradp = hiplib.csc_grad_multi(colptr, crow, cval, m_padded_flat,
                                      shard.d, kc, heavy)
        if kc != k:
            return gradp.reshape(shard.d, kc)[:, :k].reshape(-1).contiguous()
        return gradp
    m2d = m_padded_flat.reshape(n, kc)[:, :k]
    grad = torch.empty((shard.d, k), dtype=torch.float32,
                       device=shard.val.device)
    for lo in range(0, k, 32):
        hi = min(lo + 32, k)
        kcc = padded_k(hi - lo)
        chunk = torch.zeros((n, kcc), dtype=torch.float32,
                            device=shard.val.device)
        chunk[:, : hi - lo] = m2d[:, lo:hi]
        gc = hiplib.csc_grad_multi(colptr, crow, cval, chunk.reshape(-1),
                                   shard.d, kcc, heavy)
        grad[:, lo:hi] = gc.reshape(shard.d, kcc)[:, : hi - lo]
    return grad.reshape(-1).contiguous()
